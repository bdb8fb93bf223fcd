"""What `IrsLqrBatch` and `IrsLqrQuasistaticBatch` have in common: the per-problem results stacked along a leading
problem dimension, and the per-problem seeds as the batched sample passes take them."""
import numpy as np
import torch


class StackedResults:
    """`x_trj` (B,T+1,n), `u_trj` (B,T,m) and `cost` (B) of a class that keeps one single-class object per problem in
    `self.problems`."""

    @property
    def x_trj(self):
        return np.stack([np.asarray(pr.x_trj, float) for pr in self.problems])

    @property
    def u_trj(self):
        return np.stack([np.asarray(pr.u_trj, float) for pr in self.problems])

    @property
    def cost(self):
        return np.array([pr.cost for pr in self.problems])


def seed_bits(seeds, device):
    """(B) int64 on `device` holding the uint64 bits of the problems' seeds (any Python ints, taken modulo 2^64)."""
    bits = np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], dtype=np.uint64)
    return torch.as_tensor(bits.view(np.int64)).to(device)

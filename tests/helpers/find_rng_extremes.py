"""Finds the extreme draws of the smoothing generator's stream that tests/golden/rng_extremes.json records: among the
first 2^24 sample indices of (seed, iteration, t = 0, block 0) those with the smallest and the largest u1 word and those
whose u2 word lies nearest each k/8 (the quadrant boundaries k/4 and the ties (2k+1)/8 of rintf(4 u2)).
    python -m tests.helpers.find_rng_extremes          # rewrites the file (a few seconds)
tests/test_functors_cpu.py re-derives a few of its entries."""
import json

from tests.helpers import functor_reference as fr

if __name__ == "__main__":
    found = fr.scan_rng_extremes()
    with open(fr.RNG_GOLDEN, "w") as f:
        json.dump(found, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", fr.RNG_GOLDEN, len(fr.rng_extreme_indices(found)), "indices")

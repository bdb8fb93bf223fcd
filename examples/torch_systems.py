"""Systems written as torch callables (irs_mpc_amd.TorchDynamicalSystem): what a user with a model of their own writes.

TorchCartPole has no device functor; TorchPendulum and TorchQuadrotor restate two compiled models
(examples/pendulum/pendulum_dynamics.py, examples/quadrotor/quadrotor_dynamics.py of the reference), so that
tools/time_values_pass.py can put the callable's cost beside the functor's.
"""
import torch

import irs_mpc_amd as amd


class TorchCartPole(amd.TorchDynamicalSystem):
    """Cart-pole, explicit Euler.  x = (cart position, pole angle from the downward vertical, their rates), u = the
    force on the cart."""

    def __init__(self, h, m_cart=1.0, m_pole=0.1, length=0.5, gravity=9.81):
        super().__init__()
        self.h, self.dim_x, self.dim_u = h, 4, 1
        self.mc, self.mp, self.l, self.g = m_cart, m_pole, length, gravity

    def dynamics_batch_torch(self, x, u):
        th, xd, thd, f = x[:, 1], x[:, 2], x[:, 3], u[:, 0]
        s, c = torch.sin(th), torch.cos(th)
        den = self.mc + self.mp * s * s
        xdd = (f + self.mp * s * (self.l * thd * thd + self.g * c)) / den
        thdd = (-f * c - self.mp * self.l * thd * thd * c * s - (self.mc + self.mp) * self.g * s) / (self.l * den)
        return x + self.h * torch.stack([xd, thd, xdd, thdd], dim=1)


class TorchPendulum(amd.TorchDynamicalSystem):
    """pendulum_dynamics.py:62-81: semi-implicit Euler."""

    def __init__(self, h):
        super().__init__()
        self.h, self.dim_x, self.dim_u = h, 2, 1

    def dynamics_batch_torch(self, x, u):
        next_speed = x[:, 1] + self.h * (-torch.sin(x[:, 0]) + u[:, 0])
        next_angle = x[:, 0] + self.h * next_speed
        return torch.stack([next_angle, next_speed], dim=1)


class TorchQuadrotor(amd.TorchDynamicalSystem):
    """quadrotor_dynamics.py:40-77: explicit Euler on a roll-pitch-yaw rigid body, the matrices written out."""

    def __init__(self, h):
        super().__init__()
        self.h, self.dim_x, self.dim_u = h, 12, 4
        self.m, self.L, self.g, self.kF, self.kM = 0.775, 0.15, 9.81, 1.0, 0.0245
        self.I = (0.0015, 0.0025, 0.0035)

    def dynamics_batch_torch(self, x, u):
        uF, uM = self.kF * u, self.kM * u
        Fz = uF.sum(dim=1)
        M0 = self.L * (-uF[:, 0] - uF[:, 1] + uF[:, 2] + uF[:, 3])
        M1 = self.L * (-uF[:, 0] - uF[:, 3] + uF[:, 1] + uF[:, 2])
        M2 = -uM[:, 0] + uM[:, 1] - uM[:, 2] + uM[:, 3]
        sr, cr = torch.sin(x[:, 3]), torch.cos(x[:, 3])
        sp, cp = torch.sin(x[:, 4]), torch.cos(x[:, 4])
        sy, cy = torch.sin(x[:, 5]), torch.cos(x[:, 5])
        rd0, rd1, rd2 = x[:, 9], x[:, 10], x[:, 11]
        # R_WB [0, 0, Fz]' = Fz times the third column of Rz Ry Rx
        xdd = Fz * (cy * sp * cr + sy * sr) / self.m
        ydd = Fz * (sy * sp * cr - cy * sr) / self.m
        zdd = (Fz * cp * cr - self.m * self.g) / self.m
        # body rates pqr = PhiInv rpy_d and their derivative
        p = rd0 - sp * rd2
        q = cr * rd1 + sr * cp * rd2
        r = -sr * rd1 + cr * cp * rd2
        I0, I1, I2 = self.I
        pd = (M0 - (q * I2 * r - r * I1 * q)) / I0
        qd = (M1 - (r * I0 * p - p * I2 * r)) / I1
        rd = (M2 - (p * I1 * q - q * I0 * p)) / I2
        tp, cp2 = sp / cp, cp * cp
        # rpy_dd = Phi pqr_d + (dPhi/drpy . rpy_d) pqr
        a0 = pd + sr * tp * qd + cr * tp * rd + (cr * tp * rd0 + sr / cp2 * rd1) * q + (-sr * tp * rd0 + cr / cp2 * rd1) * r
        a1 = cr * qd - sr * rd + (-sr * rd0) * q + (-cr * rd0) * r
        a2 = sr / cp * qd + cr / cp * rd + (cr / cp * rd0 + sr * sp / cp2 * rd1) * q \
            + (-sr / cp * rd0 + cr * sp / cp2 * rd1) * r
        xdot = torch.stack([x[:, 6], x[:, 7], x[:, 8], rd0, rd1, rd2, xdd, ydd, zdd, a0, a1, a2], dim=1)
        return x + self.h * xdot

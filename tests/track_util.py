"""Shared by the surface-track GPU tests: the cases, their points, the fp64 / fp32 oracles and the error budget of DESIGN.md 7h."""
import numpy as np
import torch

import weightgen
from oracle import endosurf_oracle as O

from endosurf_amd import tracking

CASES = [(21, "init"), (11, "trained"), (23, "trained")]          # the cases of tests/test_track_host.py
RHO = 0.75          # the contraction bound asserted on every test's points
TOL = 1e-5
FLT_MAX = float(np.finfo(np.float32).max)


def oracle_net(state, dtype):
    return O.OracleNet({k: torch.tensor(v, dtype=dtype) for k, v in state.items()}, True)


def deform_fn(net):
    def fn(y, t):
        with torch.no_grad():
            return net.deform(y, t, with_jac=False)[0]
    return fn


def draw(seed, M):
    """x [M,3] uniform in [-0.8, 0.8]^3, t_from, t_to [M] uniform in [0, 1): fp32 values (the device's inputs) from default_rng(100 + seed)."""
    rng = np.random.default_rng(100 + seed)
    x = torch.from_numpy(rng.uniform(-0.8, 0.8, size=(M, 3)).astype(np.float32))
    t_from, t_to = (torch.from_numpy(rng.uniform(size=(M,)).astype(np.float32)) for _ in range(2))
    return x, t_from, t_to


def assert_contraction(net64, x, *times):
    """The condition on the inputs: max |J - I|_2 < 0.75 of the fp64 oracle at ``x`` (fp32 values) and each of ``times``."""
    with torch.no_grad():
        J = torch.cat([net64.deform(x.double(), t.double().expand(x.shape[0]) if t.numel() == 1 else t.double())[1] for t in times])
    rho = float(torch.linalg.matrix_norm(J - torch.eye(3, dtype=torch.float64), ord=2).max())
    assert rho < RHO, rho
    return rho


def budget(e_fwd, tol=TOL):
    """How far a row that froze at step <= tol may be from the fixed point of the exact map when D is evaluated with error e_fwd and
    rho < 0.75: (rho tol + e_fwd) / (1 - rho)  (Contract)."""
    return (RHO * tol + e_fwd) / (1.0 - RHO)


def fixed_point64(net64, c, t):
    """y* of the fp64 oracle for fp32 inputs (c, t): tol 1e-13, 200 evaluations; every row must get there."""
    y, step, iters = tracking.inverse_deform(deform_fn(net64), c.double(), t.double(), max_iters=200, tol=1e-13)
    assert bool((step <= 1e-13).all())
    return y


def rownorm(a):
    return torch.linalg.norm(a, dim=-1)

"""Test points for the comparisons with the fp64 oracle away from the golden shapes (test_gpu_backward_shapes.py,
test_gpu_forward_shapes.py): drawn like test_point_backward's, then screened so that no point sits on a ReLU kink."""
import contextlib

import numpy as np
import torch

import weightgen
from oracle import endosurf_oracle as O

SEED = 41
RELU_MARGIN = 1e-5
# Maximum error per row of the point forward's buffers against the fp64 oracle, on points that keep RELU_MARGIN from every ReLU kink.
# Measured on an MI355X over every case of test_gpu_forward_shapes.py (1 ... 68 608 rows, all launch layouts and point sources), worst
# row: x_c 9.1e-8, sdf 7.2e-7, g_c 1.6e-6, J d 3.1e-7, g_o 1.8e-6, feat 1.9e-6, rgb 6.2e-7, the time adjoint 5.6e-7 -- the oracle's own
# fp32 run is 7e-8, 4e-7, 1.1e-6, 2e-7, 1.2e-6, 9e-7, 5e-7, 2e-7 from its fp64 run on the same rows.  The gates sit ~8 x above the
# measurement, 2 to 17 times below the quantile budgets of test_point_forward (3e-6, 1e-5, 1e-4, 5e-5, 2e-4, 5e-5, 5e-5), which have to
# make room for flipped ReLU masks.
FORWARD_GATE = dict(xc=1e-6, sdf=5e-6, gc=1.5e-5, v=3e-6, go=1.5e-5, feat=1.5e-5, rgb=5e-6, tbar=5e-6)


def oracle_net(mode="trained", use_deform=True, seed=SEED, dtype=torch.float64):
    return O.OracleNet({k: torch.tensor(v, dtype=dtype) for k, v in weightgen.make_state(seed, mode, use_deform).items()}, use_deform)


def relu_margin(net, x, d, t):
    """Smallest |pre-activation| over the ReLU layers of the deformation and colour networks, per point (fp64, the oracle's weights).
    The Jacobian of both networks is discontinuous where one of them is 0: a point within fp32 rounding of such a kink can take the
    other branch in the kernels, which moves g_o / J d / rgb of that point (and a whole gradient tensor by ~1e-3 at these batch sizes)
    and says nothing about the kernels."""
    with torch.no_grad():
        pe = net.point_eval(x, d, t, with_color=True)
        ins = {"color_network": torch.cat([O.freq_encode(pe["x_c"], 10), pe["g_c"], O.freq_encode(pe["d_c"], 4), pe["feat"]], -1)}
        if net.use_deform:
            ins["deform_network"] = torch.cat([O.freq_encode(x, 6), O.freq_encode(t, 6)], -1)
        margin = torch.full((x.shape[0],), float("inf"), dtype=x.dtype)
        for name, e in ins.items():
            u = e
            for l in range(8):
                W, b = net._wb(name, l)
                if l == 4:
                    u = torch.cat([u, e], -1) / O.SQRT2
                a = u @ W.t() + b
                margin = torch.minimum(margin, a.abs().min(-1)[0])
                u = torch.relu(a)
    return margin


def inputs(M, seed, use_deform=True, screen=None, mode="trained", count=None):
    """Points, view directions, times and upstream adjoints of (sdf, g_o, rgb): the construction of test_point_backward.  Rows
    ``screen`` (default: all) are redrawn until they keep RELU_MARGIN from every ReLU kink of the ``mode`` weights; ``count`` (a
    one-element list) receives the number of redrawn points."""
    rng = np.random.default_rng(seed)

    def draw(n):
        x = rng.uniform(-0.7, 0.7, size=(n, 3)).astype(np.float32)
        d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=-1, keepdims=True)
        return torch.from_numpy(x), torch.from_numpy(d.astype(np.float32)), torch.from_numpy(rng.uniform(size=(n,)).astype(np.float32))
    x, d, t = draw(M)
    rows = torch.arange(M) if screen is None else torch.as_tensor(np.asarray(screen, np.int64))
    net = oracle_net(mode, use_deform)
    redrawn = 0
    for _ in range(64):
        near = rows[relu_margin(net, x[rows].double(), d[rows].double(), t[rows].double()[:, None]) < RELU_MARGIN]
        if near.numel() == 0:
            break
        redrawn += near.numel()
        x[near], d[near], t[near] = draw(near.numel())
    else:
        raise AssertionError("could not place the points away from the ReLU kinks")
    if count is not None:
        count[0] = redrawn
    ws, wg, wc = (torch.from_numpy(rng.normal(size=s).astype(np.float32)) for s in ((M, 1), (M, 3), (M, 3)))
    return x, d, t, ws, wg, wc


@contextlib.contextmanager
def split_chain(eng, split=True, infer_min=1):
    """The opt-in split-precision family for the calls inside: ``eng.split_precision = True`` and (unless ``infer_min`` is None: the
    shipped threshold stays) ``eng.x3_infer_min = infer_min``, both restored on the way out.  ``split=False`` changes nothing."""
    old = (eng.split_precision, eng.x3_infer_min)
    if split:
        eng.split_precision = True
        if infer_min is not None:
            eng.x3_infer_min = infer_min
    try:
        yield
    finally:
        eng.split_precision, eng.x3_infer_min = old


def routes_split(eng, M, save):
    """The routing condition of Engine.point_forward (fp32_only aside) on the engine's current settings."""
    return bool(eng.split_precision and M >= eng.x3_infer_min and (eng.x3_train_chain or not save))

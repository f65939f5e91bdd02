"""The OPT-IN split-precision TRAINING chain (csrc/infer_x3r.hip with saves, train_x3r.hip, the k_wgrad_x3 tasks of wgrad.hip) through
section A and B of test_gpu_backward_shapes.py: es_point_forward_x3 + es_point_backward_x3 against autograd on the fp64 oracle at the
shapes where the family's launch geometry changes (a wave owns 16 points in k_deform_jvp_x3r, 32 in the VJP / colour kernels; whole
[256 x 256] weight-gradient tasks with staged zero rows; the two-segment launches k_deform_jvp_x3r_tail / k_deform_bwd_x3r_tail).

Helpers, seeds and point sets are those of test_gpu_backward_shapes.py (``split=True``: Engine.split_precision on and x3_infer_min = 1
for the call), so the oracle's passes are the same computation.  Gates: POINT_TOL["fp32"] (5e-4 per tensor, median 1e-4, loss 2e-3),
which DESIGN 2 states for both families; >= 20 live gradient tensors; the pad rows of the x_c adjoint exact zeros.  Every case asserts
that the context came from the split chain (``ctx.x3_chain``).  The gradient tables go to the log directory as shapes_x3_*."""
import pytest

import test_gpu_backward_shapes as B

pytestmark = pytest.mark.gpu

DENSE = B.DENSE + [(16, True), (17, True), (33, True)]


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("M,color", DENSE)
def test_point_backward_pad_rows(use_deform, M, color):
    """The pad-row counts of the fp32 sweep + one row on / behind a jvp wave's 16 points and behind a vjp wave's 32."""
    B._dense(use_deform, M, color, split=True)


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("M", [1024, 1100, 1400])
def test_point_backward_row_chunks(M, deterministic):
    """8 / 16, 9 / 18 and 11 / 22 row chunks of 128 rows: the k_wgrad_x3 tasks and their staged zero rows, atomic and deterministic."""
    B._dense(True, M, True, deterministic=deterministic, split=True)


@pytest.mark.parametrize("poison", [None, float("nan")])
def test_point_backward_workspace_history(poison):
    """M = 65 right behind M = 1400 on one engine, both on the split chain: recycled memory, or a workspace filled with NaN."""
    r = B._renderer(True)
    x, d, t, ws, wg, wc = B._inputs(1400, 2400, screen=[])
    B._hip_point_grads(r, x, d, t, ws, wg, wc, True, split=True)
    B._dense(True, 65, True, poison=poison, r=r, split=True)


@pytest.mark.parametrize("use_deform", [True, False])
@pytest.mark.parametrize("tail", [64, 192])
def test_point_backward_tail_dense(use_deform, tail):
    """m_color = 256 < M = 256 + 64 / 256 + 192: deform_jvp_x3r_with_tail / deform_bwd_x3r_with_tail with a 64- and a 192-row tail."""
    B._tail_dense(use_deform, tail, split=True)


@pytest.mark.parametrize("name,deterministic", [("ragged_20031", False), ("train_68608_deform", False), ("train_68608_nodeform", False),
                                                ("train_68608_deform", True)])
def test_point_backward_sparse_seeds(name, deterministic):
    """20 031 rows and the fused training launch 65 536 + 3 072 (what the split headline runs), adjoint seeds on the fp32 case's rows."""
    B._sparse_seeds(name, deterministic, split=True)

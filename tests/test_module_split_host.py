"""CPU: Engine and EndoSurfRenderer are assembled from mixins (engine_mesh, engine_eval, renderer_mesh) -- no name may be defined twice
along either chain -- and the renderer's one lattice helper evaluates the expressions every extraction path used to spell out itself."""
import pytest
import torch


def _chain(cls, stop):
    out = []
    for c in cls.__mro__:
        if c is stop:
            break
        out.append(c)
    return out


def test_no_name_is_defined_twice_along_the_mixin_chains():
    """A method a mixin and its class both define would silently shadow one of them: every non-dunder name lives in exactly one class."""
    import torch.nn as nn
    from endosurf_amd.engine import Engine
    from endosurf_amd.renderer import EndoSurfRenderer
    for cls, stop, n_classes in ((Engine, object, 3), (EndoSurfRenderer, nn.Module, 2)):
        chain = _chain(cls, stop)
        assert len(chain) == n_classes, chain
        owner = {}
        for c in chain:
            for name in vars(c):
                if name.startswith("__") and name.endswith("__"):
                    continue
                assert name not in owner, f"{name} is defined in {owner[name].__name__} and in {c.__name__}"
                owner[name] = c
        assert len(owner) > 40          # (the walk saw the methods)


BOUNDS = [((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), ((-0.3, 0.1, -1.7), (0.9, 1.3, 0.2))]


@pytest.mark.parametrize("R", [2, 33, 129])
@pytest.mark.parametrize("bound_min,bound_max", BOUNDS)
def test_lattice_helper_restates_the_extraction_paths_expressions(bound_min, bound_max, R):
    """``renderer_mesh._Lattice`` on the CPU against the expressions of the dense field, the band field, the index -> world map and the
    refinement's half cell as they stood before they were folded, operand for operand: ``torch.equal``."""
    from endosurf_amd.renderer import EndoSurfRenderer
    from endosurf_amd.renderer_mesh import _Lattice
    lat = _Lattice(bound_min, bound_max, R, "cpu")
    # the axes: Python floats of the fp32 CPU bounds into torch.linspace
    lo = torch.as_tensor(bound_min, dtype=torch.float32).cpu()
    hi = torch.as_tensor(bound_max, dtype=torch.float32).cpu()
    want_ax = [torch.linspace(float(lo[i]), float(hi[i]), R, device="cpu") for i in range(3)]
    axes = lat.axes()
    assert len(axes) == 3 and all(torch.equal(a, w) and a.dtype == torch.float32 for a, w in zip(axes, want_ax))
    # the bounds as [1,3] tensors and the map of index-space vertices, in fp32
    bmin = torch.as_tensor(bound_min, dtype=torch.float32).to("cpu").reshape(1, 3)
    bmax = torch.as_tensor(bound_max, dtype=torch.float32).to("cpu").reshape(1, 3)
    assert torch.equal(lat.bmin, bmin) and torch.equal(lat.bmax, bmax)
    verts = torch.rand(1000, 3, generator=torch.Generator().manual_seed(R)) * (R - 1)
    got = lat.to_world(verts)
    assert got.dtype == torch.float32 and torch.equal(got, verts / (R - 1.0) * (bmax - bmin) + bmin)
    assert torch.equal(lat.half_cell(), 0.5 * (bmax - bmin) / (R - 1.0))
    # simplify="grid" keeps its own fp64 expression
    cell, origin = EndoSurfRenderer._simplify_arg("grid", bound_min, bound_max, R)
    lo64, hi64 = lo.double().reshape(3), hi.double().reshape(3)
    assert cell == float(((hi64 - lo64) / (float(R) - 1.0)).max()) and origin == tuple(float(b) for b in lo64)

"""Surface tracing of ``renderer.EndoSurfRenderer`` (a mixin): ``tracing.trace_surface`` with the model's own networks under it -- rays
to surface hits in one launch (csrc/trace.hip) -- and the surface rendering that follows from it: one point evaluation at the hits
through the path ``renderondepth`` uses."""
from __future__ import annotations

import torch

from . import tracing
from ._device import _on_device, f32


class RendererTraceMixin:
    def _trace_rays(self, rays):
        """``rays`` (tensor or numpy array, anywhere, [..., 9]) as the library reads them: fp32 [N, 9], contiguous, on this device."""
        r = torch.as_tensor(rays)
        if r.dim() < 1 or r.shape[-1] != 9:
            raise ValueError(f"rays must be [..., 9] (got {tuple(r.shape)})")
        return f32(r.to(device=self.device, dtype=torch.float32)).reshape(-1, 9)

    @_on_device
    def trace_surface(self, rays, tau=0.0, eps=1e-5, relax=1.0, min_step=1e-3, max_iters=128):
        """Where each of ``rays`` [N,9] meets the surface sdf = ``tau``: ``tracing.trace_surface``'s dict (depth [N,1], status, iters [N]
        int32, residual [N], points [N,3]) as device tensors plus ``valid`` [N] bool (``status == tracing.HIT``), no grad, no read-back,
        one launch, fp32 whatever ``engine.split_precision`` says.  ``depth`` holds ``ray_marching``'s three kinds of value (z, 0 for an
        occupied origin, inf for no hit), so ``renderondepth(rays, depth)`` takes it as it is; ``out["points"][out["valid"]]`` with the
        rays' times ``rays[:, 8]`` is what ``track_points`` and ``to_canonical`` take."""
        rays = self._trace_rays(rays)
        weff, packed = self._weights()
        with torch.no_grad():
            out = self.engine.trace_surface(rays, weff.detach(), packed, self.use_deform, tau, eps, relax, min_step, max_iters)
            out["valid"] = out["status"] == tracing.HIT
        return out

    @_on_device
    def render_surface(self, rays, **trace_args):
        """Surface rendering of ``rays`` [N,9]: ``trace_surface(rays, **trace_args)``, then ``renderondepth`` at the traced depth -- one
        point evaluation, fixed shape, masked.  dict(color [N,3], normal [N,3] = the unit gradient in the observed space, zero where not
        valid, gradient [N,3], depth [N,1], valid [N] bool, status, iters [N] int32); ``color`` and ``gradient`` are
        ``renderondepth(rays, depth)``'s, bit for bit."""
        rays = self._trace_rays(rays)
        with torch.no_grad():
            tr = self.trace_surface(rays, **trace_args)
            color, grad, _ = self.renderondepth(rays, tr["depth"])
            unit = grad / (torch.linalg.norm(grad, ord=2, dim=-1, keepdim=True) + 1e-10)
            normal = torch.where(tr["valid"][:, None], unit, torch.zeros_like(unit))
        return {"color": color, "normal": normal, "gradient": grad, "depth": tr["depth"], "valid": tr["valid"], "status": tr["status"],
                "iters": tr["iters"]}

    @_on_device
    def render_surface_frames(self, rays, ray_chunk=65536, background=1.0, **trace_args):
        """Surface-render ``rays`` [..., 9] in chunks of ``ray_chunk`` rays, no grad: the dict ``render_frames`` returns (color [n,3],
        depth [n,1], normal [n,3]) plus ``valid`` [n] bool, on the device, so ``evaluate_rendered`` takes it unchanged.  Pixels whose ray
        is not valid get ``background`` colour, depth 0 and a zero normal."""
        flat = self._trace_rays(rays)
        n, C = flat.shape[0], int(ray_chunk)
        if C < 1:
            raise ValueError(f"ray_chunk must be at least 1 (got {ray_chunk})")
        out = {"color": self.engine.empty(n, 3), "depth": self.engine.empty(n, 1), "normal": self.engine.empty(n, 3),
               "valid": self.engine.empty(n, dtype=torch.bool)}
        with torch.no_grad():
            for i in range(0, n, C):
                r = self.render_surface(flat[i:i + C], **trace_args)
                v = r["valid"][:, None]
                out["color"][i:i + C] = torch.where(v, r["color"], torch.full_like(r["color"], float(background)))
                out["depth"][i:i + C] = torch.where(v, r["depth"], torch.zeros_like(r["depth"]))
                out["normal"][i:i + C] = r["normal"]
                out["valid"][i:i + C] = r["valid"]
        return out

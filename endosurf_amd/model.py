"""The parameter container and the reference-named network modules (reference ``EndoSurfNet`` and its four networks,
endosurf.py:524-852): same module tree, parameter names and shapes, so reference checkpoints load unchanged.

Every parameter is a view into ONE flat fp32 device buffer whose layout is owned by csrc/arch.h; the modules' forwards and the
model's query methods run the fused HIP kernels through the renderer the model belongs to (reached through a weak reference:
nothing here imports the renderer).
"""
from __future__ import annotations

import math
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _lib, params as P
from .engine import PointCtx, f32
from .functions import _NetForwardFn, _PointEvalFn

# architecture every reference EndoSurf config uses (configs/endosurf/**: only ``use_deform`` varies)
_ARCH = {
    "deform_network": dict(n_layers=9, hidden_dim=256, skips=[4], out_dim=3,
                           enc_pos_cfg=dict(enc_type="frequency", input_dim=3, multires=6),
                           enc_time_cfg=dict(enc_type="frequency", input_dim=1, multires=6)),
    "sdf_network": dict(n_layers=9, hidden_dim=256, skips=[4], out_dim=257,
                        enc_pos_cfg=dict(enc_type="frequency", input_dim=3, multires=6)),
    "color_network": dict(n_layers=9, hidden_dim=256, skips=[4], out_dim=3, feat_dim=256,
                          enc_pos_cfg=dict(enc_type="frequency", input_dim=3, multires=10),
                          enc_dir_cfg=dict(enc_type="frequency", input_dim=3, multires=4)),
}


def _check_arch(net_cfg: dict):
    """The kernels are specialised for the one architecture the reference ships; anything else fails loudly."""
    for net, want in _ARCH.items():
        if net == "deform_network" and not net_cfg.get("use_deform", True):
            continue
        got = net_cfg[net]
        for k, v in want.items():
            g = got.get(k, v)
            if isinstance(v, dict):
                g = {kk: g.get(kk) for kk in v}
            if g != v:
                raise NotImplementedError(
                    f"endosurf_amd kernels are specialised for net.{net}.{k} = {v!r} (all reference EndoSurf configs); got {g!r}")


# ---------------------------------------------------------------------------------------------------------------
# parameter holders (views into one flat fp32 device buffer whose layout is owned by csrc/arch.h)
# ---------------------------------------------------------------------------------------------------------------
class WNLinear(nn.Module):
    """Parameters of one weight-normed nn.Linear, reference names/shapes: bias[N], weight_g[N,1], weight_v[N,K]."""

    def __init__(self, flat: torch.Tensor, lay: dict, prefix: str):
        super().__init__()
        for name in ("bias", "weight_g", "weight_v"):
            off, shape = lay[f"{prefix}.{name}"]
            n = int(np.prod(shape))
            self.register_parameter(name, nn.Parameter(flat[off:off + n].view(shape)))

    replaced = 0          # bumped when a registered parameter is assigned anew: EndoSurfNet drops its cached parameter walk

    def __setattr__(self, name, value):
        if name in ("bias", "weight_g", "weight_v") and name in self.__dict__.get("_parameters", {}):
            WNLinear.replaced += 1
        super().__setattr__(name, value)

    def forward(self, x):
        """One weight-normed linear layer on its own, y = x (g v / |v|_row)^T + b: what ``model.<net>.net[l](x)`` gives in the reference
        (nn.utils.weight_norm(nn.Linear), utils.py:57-58 / :108-109).  Not part of the hot path -- the fused kernels evaluate whole
        networks -- so this is plain torch arithmetic on the parameter views, differentiable like the reference's."""
        v = self.weight_v
        w = self.weight_g * v / torch.linalg.norm(v, dim=1, keepdim=True)
        return torch.nn.functional.linear(x.to(v.dtype), w, self.bias)


class _MLP(nn.Module):
    def __init__(self, flat, lay, net_name):
        super().__init__()
        self.net = nn.ModuleList([WNLinear(flat, lay, f"{net_name}.net.{l}") for l in range(9)])
        self._model = None          # weakref to the owning EndoSurfNet (set there): the forwards below run the fused kernels

    def _ctx(self):
        m = self._model() if self._model is not None else None
        if m is None:
            raise RuntimeError("this network is not attached to an EndoSurfNet / EndoSurfRenderer")
        return m, m._r()


class DeformNetwork(_MLP):
    def forward(self, x, t):
        """Displacement field delta x(x, t) [M,3] (reference DeformNetwork.forward, endosurf.py:724-738), no grad: x_c of the fused
        point evaluation minus x."""
        m, r = self._ctx()
        with torch.cuda.device(r.device), torch.no_grad():
            x, t = m._xt(x, t)
            weff, packed = r._weights()
            pctx = r.engine.point_forward(r.engine.points(x=x, t=t), weff.detach(), packed, _lib.PF_DEFORM)
            return pctx.view("xc") - x


class SDFNetwork(_MLP):
    def forward(self, x):
        """[sdf | 256 geometry features] [M,257] at CANONICAL points (reference SDFNetwork.forward, endosurf.py:773-786), no grad."""
        m, r = self._ctx()
        with torch.cuda.device(r.device), torch.no_grad():
            x, t = m._xt(x, torch.zeros(1, device=x.device))
            weff, packed = r._weights()
            d = torch.zeros_like(x)
            d[:, 2] = 1.0
            pctx = r.engine.point_forward(r.engine.points(x=x, t=t, dirs=d), weff.detach(), packed, _lib.PF_COLOR)   # features need the colour path's buffers
            return torch.cat([pctx.view("sdf"), pctx.view("feat")], -1)

    def sdf(self, x):
        """sdf [M,1] at canonical points (endosurf.py:788-791)."""
        return self.forward(x)[..., :1]


class ColorNetwork(_MLP):
    def forward(self, x, n, d, geo_feat):
        """sigmoid rgb [M,3] of the colour MLP on EXPLICIT inputs (reference ColorNetwork.forward, endosurf.py:828-842): position x
        (encoded with L = 10), normal n (used as given), view direction d (encoded with L = 4, used as given: EndoSurfNet.forward
        normalises J d before this call, :684-685) and the 256 geometry features.  One launch of the fused chain's colour body on a
        workspace whose x_c / g_c / feature buffers hold the inputs (es_color_forward).  No grad, like the other per-network forwards."""
        m, r = self._ctx()
        with torch.cuda.device(r.device), torch.no_grad():
            f = lambda a, w: a.detach().to(device=r.device, dtype=torch.float32).reshape(-1, w).contiguous()
            x, n, d, feat = f(x, 3), f(n, 3), f(d, 3), f(geo_feat, 256)
            M = x.shape[0]
            if not (n.shape[0] == d.shape[0] == feat.shape[0] == M):
                raise ValueError("x, n, d and geo_feat must hold one row per point")
            if M == 0:
                return torch.zeros(0, 3, device=r.device)
            weff, packed = r._weights()
            eng = r.engine
            pts = eng.points(x=x, t=torch.zeros(1, device=r.device), dirs=d)
            pctx = PointCtx(eng, pts, _lib.PF_COLOR)
            pctx.view("xc").copy_(x); pctx.view("gc").copy_(n); pctx.view("feat").copy_(feat)
            eng.color_forward(pctx, weff.detach(), packed)
            return pctx.view("rgb").clone()


class SingleVarianceNetwork(nn.Module):
    def __init__(self, flat, lay):
        super().__init__()
        off, _ = lay["deviation_network.variance"]
        self.register_parameter("variance", nn.Parameter(flat[off:off + 1].view(())))

    def forward(self, x):
        """inv_s broadcast to [len(x), 1] (endosurf.py:850-852); plain torch, differentiable w.r.t. the variance."""
        return torch.ones([len(x), 1], device=self.variance.device) * torch.exp(self.variance * 10.0)


def _reference_style_init(flat: torch.Tensor, lay: dict, net_cfg: dict):
    """Same initial distributions (and, under the same torch seed, the same draws in the same order) as the reference:
    build_mlp_idr / build_mlp_nerf (utils.py:11-111) -> nn.Linear default init, geometric init for the SDF network
    (bias 0.8), then weight_norm's g = ||W||_row, v = W; SingleVarianceNetwork init_val (endosurf.py:845-848)."""
    sdf_bias = float(net_cfg["sdf_network"].get("geometric_init_bias", 0.8))
    geometric = bool(net_cfg["sdf_network"].get("geometric_init", True))
    order = (["deform_network"] if net_cfg.get("use_deform", True) else []) + ["sdf_network", "color_network"]
    with torch.no_grad():
        for net in order:
            for l in range(9):
                _, (n_out, n_in) = lay[f"{net}.net.{l}.weight_v"]
                lin = nn.Linear(n_in, n_out)
                W, b = lin.weight.data, lin.bias.data
                if net == "sdf_network" and geometric:
                    in_dim = 39
                    if l == 8:
                        nn.init.normal_(W, mean=math.sqrt(math.pi) / math.sqrt(n_in), std=1e-4)
                        nn.init.constant_(b, -sdf_bias)
                    elif l == 0:
                        nn.init.constant_(b, 0.0)
                        nn.init.constant_(W[:, 3:], 0.0)
                        nn.init.normal_(W[:, :3], 0.0, math.sqrt(2) / math.sqrt(n_out))
                    elif l == 4:
                        nn.init.constant_(b, 0.0)
                        nn.init.normal_(W, 0.0, math.sqrt(2) / math.sqrt(n_out))
                        nn.init.constant_(W[:, -(in_dim - 3):], 0.0)
                    else:
                        nn.init.constant_(b, 0.0)
                        nn.init.normal_(W, 0.0, math.sqrt(2) / math.sqrt(n_out))
                for name, val in (("bias", b), ("weight_g", W.norm(dim=1, keepdim=True)), ("weight_v", W)):
                    off, shape = lay[f"{net}.net.{l}.{name}"]
                    flat[off:off + val.numel()].copy_(val.reshape(-1))
        off, _ = lay["deviation_network.variance"]
        flat[off] = float(net_cfg["deviation_network"]["init_val"])


class EndoSurfNet(nn.Module):
    """Parameter container mirroring the reference EndoSurfNet (endosurf.py:524-568)."""

    def __init__(self, net_cfg: dict, device):
        super().__init__()
        _check_arch(net_cfg)
        self._renderer = self._pack_cache = self._flat_grad = None          # (_renderer: a weakref, set by the EndoSurfRenderer that owns the model)
        self._epoch = 0            # bumped by in-place updates that bypass torch's version counters (trainer.FlatAdam)
        self.bound = net_cfg["bound"]
        self.use_deform = bool(net_cfg["use_deform"])
        lay = P.layout()
        n = int(_lib.load().es_param_floats())
        flat_cpu = torch.zeros(n)
        _reference_style_init(flat_cpu, lay, net_cfg)
        self._flat = flat_cpu.to(device)
        if self.use_deform:
            self.deform_network = DeformNetwork(self._flat, lay, "deform_network")
        self.sdf_network = SDFNetwork(self._flat, lay, "sdf_network")
        self.color_network = ColorNetwork(self._flat, lay, "color_network")
        self.deviation_network = SingleVarianceNetwork(self._flat, lay)
        self._layout = lay
        for net in ((self.deform_network,) if self.use_deform else ()) + (self.sdf_network, self.color_network):
            net._model = weakref.ref(self)

    def get_train_params(self):
        out = {}
        if self.use_deform:
            out["deform_network"] = list(self.deform_network.parameters())
        out["sdf_network"] = list(self.sdf_network.parameters())
        out["color_network"] = list(self.color_network.parameters())
        out["deviation_network"] = list(self.deviation_network.parameters())
        return out

    def load_checkpoints(self, ckpt):
        if self.use_deform:
            self.deform_network.load_state_dict(ckpt["deform_network"])
        self.sdf_network.load_state_dict(ckpt["sdf_network"])
        self.color_network.load_state_dict(ckpt["color_network"])
        self.deviation_network.load_state_dict(ckpt["deviation_network"])

    def save_checkpoint(self):
        ckpt = {}
        if self.use_deform:
            ckpt["deform_network"] = self.deform_network.state_dict()
        ckpt["sdf_network"] = self.sdf_network.state_dict()
        ckpt["color_network"] = self.color_network.state_dict()
        ckpt["deviation_network"] = self.deviation_network.state_dict()
        return ckpt

    def ordered_params(self):
        """(key, Parameter) in flat-buffer order, variance excluded.  (Built once: the modules and the identity of their Parameters are
        fixed for the life of the model -- ``_rebind`` / ``_apply`` only re-point ``.data`` -- and the renderer's ``_weights()`` walks this
        list several times per call of every public method.)"""
        cached = self.__dict__.get("_ordered")
        if cached is not None and self.__dict__.get("_ordered_at") == WNLinear.replaced:
            return list(cached)
        out = []
        for net in P.NET_NAMES:
            if net == "deform_network" and not self.use_deform:
                continue
            mod = getattr(self, net)
            for l in range(9):
                for name in ("bias", "weight_g", "weight_v"):
                    out.append((f"{net}.net.{l}.{name}", getattr(mod.net[l], name)))
        self.__dict__["_ordered"] = tuple(out)
        self.__dict__["_ordered_at"] = WNLinear.replaced
        self.__dict__["_plist"] = tuple(p for _, p in out)
        var = self.deviation_network.variance
        base = self._layout
        self.__dict__["_view_slots"] = tuple((p, 4 * base[k][0]) for k, p in out) + ((var, 4 * base["deviation_network.variance"][0]),)
        return out

    # ---- flat-buffer binding -------------------------------------------------------------------------------------------
    def _rebind(self):
        """Point every nn.Parameter back at its slot of the flat buffer (Parameter identity is kept, so optimisers stay valid)."""
        with torch.no_grad():
            for key, p in self.ordered_params() + [("deviation_network.variance", self.deviation_network.variance)]:
                off, shape = self._layout[key]
                p.data = self._flat[off:off + max(1, int(np.prod(shape)))].view(tuple(shape))
        self._pack_cache = None
        self._epoch += 1

    def _apply(self, fn, recurse=True):
        """``.to() / .cuda() / .float()``: move the FLAT buffer and rebuild the parameter views (nn.Module._apply would give
        every parameter its own storage and the kernels would keep reading the stale flat buffer)."""
        new = fn(self._flat)
        if new.dtype != torch.float32 or new.device.type != "cuda":
            raise TypeError(f"endosurf_amd parameters live in one fp32 buffer on an AMD GPU (got {new.dtype} on {new.device}); "
                            "the HIP kernels compute in fp32 only")
        if new.device != self._flat.device:
            raise RuntimeError(f"an EndoSurfRenderer is bound to the GPU it was constructed on ({self._flat.device}: engine, constant tables, "
                               f"streams); construct a new one on {new.device} and load_checkpoint(save_checkpoint()) instead of .to()")
        self._flat = new.contiguous()
        self._rebind()
        return self

    def _check_views(self, spot: bool = False):
        """Every parameter must still be a view of the flat buffer; anything that re-bound parameter storage (``p.data = ...``
        loaders, DDP/FSDP flattening, ...) is folded back into it.  ``spot``: look at the first and the last tensor only (the renderer
        does the full walk once per parameter version and this one at every other call)."""
        base = self._flat.data_ptr()
        slots = self.__dict__.get("_view_slots")
        if slots is None or self.__dict__.get("_ordered_at") != WNLinear.replaced:
            self.ordered_params()
            slots = self.__dict__["_view_slots"]
        if spot:
            (p0, o0), (p1, o1) = slots[0], slots[-1]
            if p0.data_ptr() == base + o0 and p1.data_ptr() == base + o1:
                return
        if all(p.data_ptr() == base + o for p, o in slots):
            return
        pairs = self.ordered_params() + [("deviation_network.variance", self.deviation_network.variance)]
        with torch.no_grad():
            for k, p in pairs:
                off, shape = self._layout[k]
                if p.data_ptr() != base + 4 * off:
                    if p.dtype != torch.float32:
                        raise TypeError(f"parameter {k} was converted to {p.dtype}; endosurf_amd computes in fp32 only")
                    self._flat[off:off + p.numel()].copy_(p.data.reshape(-1).to(self._flat.device))
        self._rebind()

    # ---- reference query surface (endosurf.py:570-689), evaluated by the fused HIP kernels -------------------------------------
    # Differentiable w.r.t. the network PARAMETERS (hand-written backward) when grad mode is on, and w.r.t. the query points / inputs where the
    # reference's are: the sdf query (its derivative IS g_o), the two gradient queries (second order: es_point_vjp) and forward() (position,
    # view direction and time: _NetForwardFn).
    def _r(self):
        r = self._renderer() if self._renderer is not None else None
        if r is None:
            raise RuntimeError("this EndoSurfNet is not attached to an EndoSurfRenderer")
        return r

    @staticmethod
    def _xt(x, t):
        x = f32(x).reshape(-1, 3)
        t = torch.as_tensor(t, device=x.device).detach().to(torch.float32).reshape(-1)
        if t.numel() not in (1, x.shape[0]):
            raise ValueError("t must hold one time per point (or a single shared time)")
        return x, (t.expand(x.shape[0]) if t.numel() == 1 else t).contiguous()

    @staticmethod
    def _wrt_points(x):
        """``x`` if autograd should track the query points (a tensor that requires grad, with grad mode on), else None."""
        return x if (torch.is_tensor(x) and x.requires_grad and torch.is_grad_enabled()) else None

    def get_sdf_from_observed_space(self, x, t):
        """sdf(x + deform(x, t)) [M,1]  (endosurf.py:570-579).

        If ``x`` requires grad (the reference's own pattern around this call is ``autograd.grad(sdf, x, create_graph=True)``,
        endosurf.py:585-600) the result is differentiable w.r.t. the points: d sdf / d x is the kernels' g_o = J^T g_c, attached as
        ``sdf + <x - x.detach(), g_o>`` (value unchanged).  g_o itself carries the hand-written backward to the parameters AND (round 5)
        to the points -- the Hessian-vector product of the query (Engine.point_input_adjoint) -- so a loss on
        ``autograd.grad(sdf, x, create_graph=True)`` back-propagates to both, like the reference's."""
        r = self._r()
        with torch.cuda.device(r.device):
            x_in = self._wrt_points(x)
            x, t = self._xt(x, t)
            weff, _ = r._weights()
            if x_in is not None or (weff.requires_grad and torch.is_grad_enabled()):
                sdf, g_o = r._point_eval(x, t, x_in=x_in)
                if x_in is not None:
                    xr = x_in.to(torch.float32).reshape(-1, 3)
                    sdf = sdf + ((xr - xr.detach()) * g_o).sum(-1, keepdim=True)
                return sdf
            return r.sdf_observed(x, t)

    def get_sdf_grad_from_observed_space(self, x, t):
        """d sdf / d x at observed points [M,3] = J^T g_c  (endosurf.py:581-601).  Differentiable w.r.t. the parameters and -- like the
        reference's create_graph=True result -- w.r.t. the points (``autograd.grad(g.sum(), x)`` = the Hessian of the query times the
        incoming adjoint: one more reverse sweep of the deformation network on the SDF backward's x_c adjoint, plus the deformation
        network's own curvature term)."""
        r = self._r()
        with torch.cuda.device(r.device):
            x_in = self._wrt_points(x)
            x, t = self._xt(x, t)
            return r._point_eval(x, t, x_in=x_in)[1]

    def get_sdf_grad_from_canonical_space(self, x):
        """d sdf / d x_c at canonical points [M,3]  (endosurf.py:603-619): the SDF network alone.  Differentiable w.r.t. the parameters and
        the points (the SDF network's Hessian-vector product comes out of its backward as the adjoint of x_c)."""
        r = self._r()
        with torch.cuda.device(r.device):
            x_in = self._wrt_points(x)
            x, t = self._xt(x, torch.zeros(1, device=x.device))
            return r._point_eval(x, t, canonical=True, x_in=x_in)[1]

    def get_deform_grad_from_observed_space(self, x, t):
        """Jacobian d x_c / d x [M,3,3] (dim_out, dim_in)  (endosurf.py:621-658): three forward-mode tangents (J e_j), no grad."""
        r = self._r()
        with torch.cuda.device(r.device):
            x, t = self._xt(x, t)
            M = x.shape[0]
            if not self.use_deform:
                return torch.eye(3, device=x.device).expand(M, 3, 3).clone()
            weff, packed = r._weights()
            cols = []
            with torch.no_grad():
                for j in range(3):
                    e = torch.zeros(M, 3, device=x.device)
                    e[:, j] = 1.0
                    pctx = r.engine.point_forward(r.engine.points(x=x, t=t, dirs=e), weff.detach(), packed, _lib.PF_DEFORM)
                    cols.append(pctx.view("v").clone())
            return torch.stack(cols, dim=-1)

    def forward(self, inputs):
        """cat([sdf, rgb]) [M,4] for inputs [x, d, t] [M,7]  (endosurf.py:660-689).  Differentiable w.r.t. the parameters and -- when
        ``inputs`` requires grad -- w.r.t. the inputs (position, view direction and time: ``_NetForwardFn``)."""
        r = self._r()
        with torch.cuda.device(r.device):
            weff, packed = r._weights()
            if self._wrt_points(inputs) is not None:
                flags = (_lib.PF_DEFORM if self.use_deform else 0) | _lib.PF_COLOR | _lib.PF_SAVE
                sdf, rgb = _NetForwardFn.apply(weff, packed, r.engine, inputs, flags)
                return torch.cat([sdf, rgb], -1).reshape(*inputs.shape[:-1], 4)
            inp = inputs.detach().to(torch.float32).reshape(-1, 7)
            x, t = self._xt(inp[:, :3], inp[:, 6])
            d = inp[:, 3:6].contiguous()
            pts = r.engine.points(x=x, t=t, dirs=d)
            sdf, _, rgb = _PointEvalFn.apply(weff, packed, r.engine, pts, r._flags(weff) | _lib.PF_COLOR)
            return torch.cat([sdf, rgb], -1)

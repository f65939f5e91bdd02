"""Autograd glue: the ``torch.autograd.Function``s that give the library's launches their hand-written backward -- weight-norm +
packing (``_PackFn``), the variance's scalar epilogue (``_SValFn``), the fused point evaluation (``_PointEvalFn``, ``_NetForwardFn``), the
reductions of the two auxiliary losses (``_EodLossFn``, ``_SnLossFn``) and the render itself (``_RenderFn``).

No arithmetic and no policy here: a forward issues its launches through ``Engine`` and keeps on ``ctx`` what the backward needs (inputs
and workspaces, never its own outputs); a ``_RenderFn`` that hosts a tail (tail._Tail) opens, finishes and closes it, no more.
"""
from __future__ import annotations

import torch

from . import _lib
from .engine import Engine, PointCtx, f32, u8

class _PackFn(torch.autograd.Function):
    """(bias, weight_g, weight_v)* -> effective-weight buffer (+ packed MFMA fragments as a side product).

    ctx never references the Function's own outputs (directly or through the model's cache): such a cycle runs through
    C++ autograd nodes and is not collectable, which would leak the buffers every step."""

    @staticmethod
    def forward(ctx, model_ref, eng: Engine, *plist):
        model = model_ref()
        weff, packed = eng.weightnorm_pack(model._flat, model.use_deform)
        ctx.model_ref, ctx.eng, ctx.flat, ctx.use_deform = model_ref, eng, model._flat, model.use_deform
        ctx.slots = [(model._layout[key][0], p.numel(), tuple(p.shape)) for key, p in model.ordered_params()]
        ctx.mark_non_differentiable(packed)
        ctx.set_materialize_grads(False)      # (otherwise autograd zero-fills a 17 MB adjoint for ``packed`` at every backward)
        return weff, packed

    @staticmethod
    def backward(ctx, dweff, _dpacked):
        model = ctx.model_ref()
        if model is not None:
            model._pack_cache = None
        if dweff is None:
            return (None, None, *[None for _ in ctx.slots])
        pipe = getattr(ctx.eng, "_grad_pipeline", None)
        if pipe is not None and pipe.get("dflat") is not None and pipe.get("dweff_ptr") == dweff.data_ptr() and pipe.get("buffers") == 1:
            pipe["adopted"] = True
            # a pipelined data-parallel step (trainer.Trainer overlap_allreduce): the hooks behind the weight-gradient launches have
            # already written (and are all-reducing) the finished layers' slices; the rest -- whatever the hooks left -- is done here
            dflat = pipe["dflat"]
            for first, n in pipe["remaining"]:
                ctx.eng.weightnorm_backward_layers(ctx.flat, dweff, dflat, first, n)
        else:
            dflat = ctx.eng.weightnorm_backward(ctx.flat, dweff.contiguous(), ctx.use_deform)
        if model is not None:
            model._flat_grad = dflat          # the parameters' .grad are views of this buffer (used by trainer.FlatAdam)
        return (None, None, *[dflat[off:off + n].view(shape) for off, n, shape in ctx.slots])


class _SValFn(torch.autograd.Function):
    """s_val = 1 / clip(exp(10 variance), 1e-6, 1e6) (endosurf.py:168, :205) in one launch; differentiable like the reference's."""

    @staticmethod
    def forward(ctx, variance, eng: Engine):
        s = eng.variance_terms(variance.detach())
        ctx.save_for_backward(s)
        ctx.shape = variance.shape
        return s.reshape(variance.shape)

    @staticmethod
    def backward(ctx, g):
        s, = ctx.saved_tensors
        inside = ((s > 1e-6) & (s < 1e6)).to(s.dtype)          # d/dvar exp(-10 var) = -10 s_val inside the clip range
        return (g.reshape(1) * -10.0 * s * inside).reshape(ctx.shape), None


class _PointEvalFn(torch.autograd.Function):
    """Fused per-point evaluation (sdf, g_o[, rgb]) with hand-written backward to the effective weights."""

    @staticmethod
    def forward(ctx, weff, packed, eng: Engine, pts, flags: int, x_in=None):
        """``x_in`` (optional): the caller's point tensor, so that autograd routes the adjoint of the POINTS through g_o back to it
        (colour-less evaluations on the fp32 kernels; ``flags`` must carry PF_SAVE)."""
        # grad mode is disabled inside Function.forward; the caller passes the save decision through ``flags``
        pctx = eng.point_forward(pts, weff, packed, flags, fp32_only=x_in is not None)
        ctx.pctx, ctx.eng, ctx.weff, ctx.packed = pctx, eng, weff, packed
        ctx.pts, ctx.flags = pts, flags
        ctx.set_materialize_grads(False)
        ctx.wrt_x = x_in is not None
        ctx.x_shape = tuple(x_in.shape) if x_in is not None else None
        ctx.x_dtype = x_in.dtype if x_in is not None else None
        outs = [pctx.view("sdf").clone(), pctx.view("go").clone()]     # own storage: outputs must not pin the workspace
        if flags & _lib.PF_COLOR:
            outs.append(pctx.view("rgb").clone())
        return tuple(outs)

    @staticmethod
    def backward(ctx, d_sdf, d_go, d_rgb=None):
        eng, pctx = ctx.eng, ctx.pctx
        if not (ctx.flags & _lib.PF_SAVE):
            raise RuntimeError("point evaluation was run without PF_SAVE; cannot backpropagate")
        if ctx.wrt_x and d_go is None and d_rgb is None and not ctx.needs_input_grad[0]:
            # the reference's first pass, autograd.grad(sdf, x, create_graph=True) (endosurf.py:585-600): only the adjoint of the POINTS is
            # asked for, and through g_o alone that is identically zero (d sdf / d x = g_o is attached by the caller) -- no launch, and the
            # workspace stays whole for the loss.backward() that follows
            return None, None, None, None, None, torch.zeros(ctx.x_shape, device=eng.device, dtype=ctx.x_dtype)
        if pctx is None:
            # (the re-evaluation reads ctx.weff / ctx.packed: the buffers of THIS forward, which later parameter updates never touch)
            # second backward through the same node (retain_graph / the reference's autograd.grad(sdf, x, create_graph=True) followed by
            # loss.backward(): with point-differentiable outputs the first pass already went through here).  The backward kernels consume
            # the workspace, so the forward is evaluated again -- same kernels, same inputs, same values.
            with torch.no_grad():
                pctx = eng.point_forward(ctx.pts, ctx.weff.detach(), ctx.packed, ctx.flags, fp32_only=ctx.wrt_x)
        dweff = eng.point_backward(pctx, ctx.weff, ctx.packed, d_sdf, d_go, d_rgb)
        xbar = None
        if ctx.wrt_x and ctx.needs_input_grad[5]:
            if d_go is None:          # through g_o alone the points' adjoint is zero (see above): no VJP launch
                xbar = torch.zeros(ctx.x_shape, device=eng.device, dtype=ctx.x_dtype)
            else:
                xbar = eng.point_input_adjoint(pctx, ctx.weff, ctx.packed, d_sdf, d_go).reshape(ctx.x_shape).to(ctx.x_dtype)
        ctx.pctx = None
        return dweff, None, None, None, None, xbar


class _NetForwardFn(torch.autograd.Function):
    """EndoSurfNet.forward (reference endosurf.py:660-689) as a function of the network parameters AND of its inputs [x, d, t]:
    (sdf [M,1], rgb [M,3]).  The backward to the effective weights is es_point_backward; the adjoint of the inputs is assembled from what
    that backward leaves in the workspace -- xcbar, the adjoint of x_c over all paths (colour encodings, geometry features, sdf, and the
    second-order path through the canonical normal g_c), and vbar, the adjoint of v = J d -- with two more reverse sweeps of the
    deformation network (es_point_vjp):
        xbar = J^T xcbar - d * curv(vbar)        (curv: the encodings' second derivative against the sweep's adjoint, ES_WS_CURV; the
        dbar = J^T vbar                           deformation MLP is piecewise linear in its encodings, so d(J d)/dx is this diagonal
        tbar = <xcbar, d x_c / d t>               and d(J d)/dt = 0 almost everywhere)
    Without a deformation network x_c = x, v = d: xbar = xcbar, dbar = vbar, tbar = 0."""

    @staticmethod
    def forward(ctx, weff, packed, eng: Engine, inputs, flags: int):
        inp = inputs.detach().to(torch.float32).reshape(-1, 7)
        x, d, t = inp[:, :3].contiguous(), inp[:, 3:6].contiguous(), inp[:, 6].contiguous()
        pts = eng.points(x=x, t=t, dirs=d)
        pctx = eng.point_forward(pts, weff, packed, flags, fp32_only=True)
        ctx.pctx, ctx.eng, ctx.weff, ctx.packed, ctx.pts, ctx.flags, ctx.d = pctx, eng, weff, packed, pts, flags, d
        ctx.in_shape, ctx.in_dtype = tuple(inputs.shape), inputs.dtype
        ctx.set_materialize_grads(False)
        return pctx.view("sdf").clone(), pctx.view("rgb").clone()

    @staticmethod
    def backward(ctx, d_sdf, d_rgb):
        eng, pctx = ctx.eng, ctx.pctx
        if not (ctx.flags & _lib.PF_SAVE):
            raise RuntimeError("EndoSurfNet.forward was evaluated without saved activations; cannot backpropagate")
        if pctx is None:          # a second backward through the node: the kernels consumed the workspace, evaluate again
            with torch.no_grad():
                pctx = eng.point_forward(ctx.pts, ctx.weff.detach(), ctx.packed, ctx.flags, fp32_only=True)
        M = pctx.M
        dweff = eng.point_backward(pctx, ctx.weff, ctx.packed, d_sdf, None, d_rgb)
        gin = None
        if ctx.needs_input_grad[3]:
            gin = eng.empty(M, 7)
            xcbar, vbar = pctx.view("xcbar").clone(), pctx.view("vbar").clone()
            if ctx.flags & _lib.PF_DEFORM:
                def sweep(c):          # J^T c, the curvature sums and the time adjoint of one reverse sweep of the deformation network
                    pctx.view("gc").copy_(c)
                    eng.point_vjp(pctx, ctx.weff.detach(), ctx.packed)
                    return pctx.view("go").clone(), pctx.view("curv").clone(), pctx.view("tbar").clone()
                jx, _, tb = sweep(xcbar)
                jv, cv, _ = sweep(vbar)
                gin[:, :3] = jx - ctx.d * cv
                gin[:, 3:6] = jv
                gin[:, 6:7] = tb
            else:
                gin[:, :3], gin[:, 3:6] = xcbar, vbar
                gin[:, 6] = 0.0
            gin = gin.reshape(ctx.in_shape).to(ctx.in_dtype)
        ctx.pctx = None
        return dweff, None, None, gin, None


class _EodLossFn(torch.autograd.Function):
    """errorondepth's reductions (reference endosurf.py:302-317) as one launch, backward one launch (es_eod_loss / es_eod_loss_backward)."""

    @staticmethod
    def forward(ctx, sdf, g_o, eng: Engine, rays, pts, mask):
        N = rays.shape[0]
        sdf_, go_, rays_, pts_, mask_ = f32(sdf), f32(g_o), f32(rays), f32(pts), f32(mask)
        if not (sdf_.numel() == N and go_.numel() == 3 * N and pts_.numel() == 3 * N and mask_.numel() == N):
            raise ValueError("errorondepth expects one point, one sdf, one gradient and one mask value per ray")
        out, inside = eng.empty(3), eng.empty(N, 1)
        eng.eod_loss(rays_, pts_, mask_, sdf_, go_, N, out, inside)
        ctx.eng, ctx.saved, ctx.n = eng, (rays_, inside, sdf_, go_, out), N
        ctx.shapes = (tuple(sdf.shape), tuple(g_o.shape))
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(inside)
        return out[0], out[1], inside

    @staticmethod
    def backward(ctx, g_sdf_err, g_ang_err, _g_inside):
        if g_sdf_err is None and g_ang_err is None:
            return None, None, None, None, None, None
        eng, N = ctx.eng, ctx.n
        rays_, inside, sdf_, go_, out = ctx.saved
        f = lambda g: None if g is None else g.detach().to(torch.float32).reshape(1)
        ga, gb = f(g_sdf_err), f(g_ang_err)
        d_sdf, d_go = eng.empty(N, 1), eng.empty(N, 3)
        eng.eod_loss_backward(rays_, inside, sdf_, go_, out, ga, gb, N, d_sdf, d_go)
        return d_sdf.view(ctx.shapes[0]), d_go.view(ctx.shapes[1]), None, None, None, None


class _SnLossFn(torch.autograd.Function):
    """surface_neighbour_error's reduction (reference endosurf.py:334-339) as one launch, backward one launch."""

    @staticmethod
    def forward(ctx, g, eng: Engine, valid):
        N = valid.numel()
        g_ = f32(g)
        if g_.numel() != 6 * N:
            raise ValueError("surface_neighbour_error expects the gradients of N surface points followed by their N neighbours")
        v8 = u8(valid)
        out = eng.empty(2)
        eng.sn_loss(g_, v8, N, out)
        ctx.eng, ctx.saved, ctx.n, ctx.shape = eng, (g_, v8, out), N, tuple(g.shape)
        ctx.set_materialize_grads(False)
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        if g_loss is None:
            return None, None, None
        eng, N = ctx.eng, ctx.n
        g_, v8, out = ctx.saved
        gl = g_loss.detach().to(torch.float32).reshape(1)
        d_g = eng.empty(2 * N, 3)
        eng.sn_loss_backward(g_, v8, out, gl, N, d_g)
        return d_g.view(ctx.shape), None, None


class _RenderFn(torch.autograd.Function):
    """render_core (reference endosurf.py:134-213) on fixed sample depths: fused point evaluation + compositing.
    Optionally evaluates ``aux_x/aux_t`` (colour-less points: errorondepth / surface-neighbour points of a training step)
    in the SAME kernel launches and returns their (sdf, g_o).  ctx keeps inputs and the workspace only, never outputs.

    ``chunk_rays`` < N with saving enabled: the rays are processed in chunks WITHOUT keeping activations and every chunk is
    re-evaluated (with saving) in the backward, its weight gradients accumulated: bounded memory for any batch size at the price
    of one extra forward (the reference bounds memory with run_fn_split's net_chunk, utils.py:114-126, but autograd still keeps
    every chunk's graph alive; here the bound is real)."""

    @staticmethod
    def forward(ctx, weff, packed, variance, eng: Engine, rays, z, sample_dist: float, cos_anneal: float, flags: int, aux_x, aux_t,
                chunk_rays: int, tail=None):
        """``tail`` (a fresh ``_Tail``; only without ``aux_x`` / chunking): lay the workspace out with ``tail.cap`` extra colour-less rows for
        the point evaluations of later calls; the last output (``token``) ties their autograd nodes to this one."""
        N, S = z.shape
        P_ = N * S
        ctx.tail = None
        ctx.set_materialize_grads(False)          # unused outputs (weights, cdf, ...) arrive as None, not as zero-filled tensors
        var1 = variance.detach().reshape(1)
        ctx.eng, ctx.weff, ctx.packed, ctx.variance = eng, weff, packed, variance
        ctx.geom = (rays, z, float(sample_dist), cos_anneal if torch.is_tensor(cos_anneal) else float(cos_anneal))
        ctx.flags = flags
        if (flags & _lib.PF_SAVE) and 0 < chunk_rays < N:
            ctx.chunk_rays, ctx.pctx, ctx.n_aux = int(chunk_rays), None, 0
            outs = {k: [] for k in ("color", "depth", "weights", "weight_max", "cdf", "wmax_idx", "go")}
            eik_acc = eng.zeros(2)
            for i in range(0, N, chunk_rays):
                r_, z_ = rays[i:i + chunk_rays], z[i:i + chunk_rays]
                n_ = r_.shape[0]
                mid = eng.mid_z(z_, sample_dist)
                # the SAME launches as the re-evaluation in the backward (saving into a workspace that is dropped right away: one chunk's
                # worth, what the backward will allocate anyway): the loss adjoints are then taken at exactly the outputs the backward
                # differentiates, whichever kernel family the engine selects for a saving evaluation
                pctx = eng.point_forward(eng.points(rays=r_, z=mid, n_per_ray=S, ldz=S), weff, packed, flags | _lib.PF_COLOR)
                a = eng.composite_args(r_, z_, pctx.view("sdf").view(-1), pctx.view("go"), pctx.view("rgb"), var1, sample_dist, cos_anneal)
                out = eng.composite_forward(a, eik_acc=eik_acc)
                for k in ("color", "depth", "weights", "weight_max", "cdf", "wmax_idx"):
                    outs[k].append(out[k])
                outs["go"].append(pctx.view("go")[:n_ * S].view(n_, S, 3).clone())
            cat = {k: torch.cat(v, 0) for k, v in outs.items()}
            ctx.eik_den = (eik_acc[1] + 1e-6).reshape(1)
            eik = eik_acc[0] / ctx.eik_den[0]
            den_out = ctx.eik_den.clone()
            ctx.mark_non_differentiable(cat["wmax_idx"], den_out)
            return (cat["color"], cat["depth"], cat["go"], eik, cat["weights"], cat["weight_max"], cat["cdf"], cat["wmax_idx"],
                    eng.zeros(0, 1), eng.zeros(0, 3), den_out, eng.empty(1))
        ctx.chunk_rays = 0
        mid = eng.mid_z(z, sample_dist)
        fused = aux_x is not None and aux_x.shape[0] > 0 and P_ % 64 == 0
        if tail is not None and not fused and (flags & _lib.PF_SAVE) and P_ % 64 == 0 and P_ > 0:
            # the colour part of a workspace laid out for P + cap rows; the tail's rows are evaluated by the calls that claim them
            pts = eng.points(rays=rays, z=mid, n_per_ray=S, ldz=S, x=tail.aux_x, t=tail.aux_t)
            pctx = PointCtx(eng, pts, flags | _lib.PF_COLOR, m_color=P_)
            eng.point_forward_rows(pctx, weff, packed, 0, P_)
            tail.open(pctx, weff, flags)
            ctx.tail = tail
        else:
            pts = eng.points(rays=rays, z=mid, n_per_ray=S, ldz=S, x=aux_x if fused else None, t=aux_t if fused else None)
            pctx = eng.point_forward(pts, weff, packed, flags | _lib.PF_COLOR, m_color=P_ if fused else 0)
        sdf_all, go_all = pctx.view("sdf"), pctx.view("go")
        a = eng.composite_args(rays, z, sdf_all.view(-1), go_all, pctx.view("rgb"), var1, sample_dist, cos_anneal)
        # own storage for every output (the 6.7 GB workspace must not outlive the backward): the compositing launch writes the samples'
        # g_o rows a second time, es_render_finish forms gradient_o_error and its normaliser from the two batch sums and copies the
        # auxiliary rows -- one launch where there were three clones, an add and a divide
        out = eng.composite_forward(a, go_copy=True)
        n_aux = aux_x.shape[0] if fused else 0
        eik, den2 = eng.empty(1), eng.empty(2)
        aux_sdf, aux_go = eng.empty(n_aux, 1), eng.empty(n_aux, 3)
        eng.render_finish(out["eik_acc"], sdf_all[P_:] if n_aux else None, go_all[P_:] if n_aux else None, n_aux, eik, den2,
                          aux_sdf if n_aux else None, aux_go if n_aux else None)
        eik_den, den_out = den2[0:1], den2[1:2]      # the eikonal term's normaliser: kept for the backward / handed out (exact data-parallel mode)
        ctx.pctx, ctx.eik_den = pctx, eik_den
        ctx.n_aux = n_aux
        ctx.mark_non_differentiable(out["wmax_idx"], den_out)
        return (out["color"], out["depth"], out["go"], eik.reshape(()), out["weights"], out["weight_max"], out["cdf"], out["wmax_idx"], aux_sdf,
                aux_go, den_out, eng.empty(1))

    @staticmethod
    def backward(ctx, g_color, g_depth, g_go, g_eik, g_weights, g_wmax, g_cdf, _, g_aux_sdf, g_aux_go, _g_den=None, _g_token=None):
        eng = ctx.eng
        tail = ctx.tail
        if tail is not None:
            # the later calls' points behind the samples: every row defined, their adjoints in the tail's buffers
            tail.finish(eng, ctx.weff, ctx.packed)
            ctx.n_aux, g_aux_sdf, g_aux_go = tail.cap, tail.g_sdf, tail.g_go
            if ctx.pctx is None:          # a second backward through this node: re-evaluate everything (main rows + the whole tail)
                rays_, zs_, sd_, _ = ctx.geom
                mid = eng.mid_z(zs_, sd_)
                pts = eng.points(rays=rays_, z=mid, n_per_ray=zs_.shape[1], ldz=zs_.shape[1], x=tail.aux_x, t=tail.aux_t)
                ctx.pctx = eng.point_forward(pts, ctx.weff, ctx.packed, ctx.flags | _lib.PF_COLOR, m_color=zs_.numel(), fp32_only=True)
        if not (ctx.flags & _lib.PF_SAVE):
            raise RuntimeError("render was run without saved activations; cannot backpropagate")
        rays, zs, sample_dist, cos_anneal = ctx.geom
        N, S = zs.shape
        var = ctx.variance.detach()
        var1 = var.reshape(1)
        z = lambda g, *shape: (g.contiguous() if g is not None else eng.zeros(*shape))
        opt = lambda g: g.contiguous() if g is not None else None
        g_color, g_depth, g_eik = z(g_color, N, 3), z(g_depth, N, 1).view(-1), z(g_eik, 1).reshape(1)
        g_weights, g_cdf, g_go = opt(g_weights), opt(g_cdf), opt(g_go)
        g_wmax = g_wmax.contiguous().view(-1) if g_wmax is not None else None
        sl = lambda g, i, j: g[i:j] if g is not None else None
        d_invs_acc = eng.zeros(1)
        dweff = eng.zeros(eng.n_weff) if N == 0 else None       # an empty batch has a zero gradient, not a missing one
        C = max(1, ctx.chunk_rays if ctx.chunk_rays else N)
        for i in range(0, N, C):
            j = min(i + C, N)
            if ctx.chunk_rays:          # re-evaluate this chunk with saving
                r_, z_ = rays[i:j], zs[i:j]
                mid = eng.mid_z(z_, sample_dist)
                pctx = eng.point_forward(eng.points(rays=r_, z=mid, n_per_ray=S, ldz=S), ctx.weff, ctx.packed, ctx.flags | _lib.PF_COLOR)
            else:
                r_, z_, pctx = rays, zs, ctx.pctx
            a = eng.composite_args(r_, z_, pctx.view("sdf").view(-1), pctx.view("go"), pctx.view("rgb"), var1, sample_dist, cos_anneal)
            # (the auxiliary points' adjoint rows are appended by the compositing launch itself: no concatenation)
            bw = eng.composite_backward(a, g_color[i:j], g_depth[i:j], g_eik, ctx.eik_den, g_weights=sl(g_weights, i, j), g_cdf=sl(g_cdf, i, j),
                                        g_wmax=sl(g_wmax, i, j), g_gradients_o=sl(g_go, i, j), d_invs_acc=d_invs_acc, n_aux=ctx.n_aux,
                                        g_aux_sdf=opt(g_aux_sdf), g_aux_go=opt(g_aux_go))
            d_sdf, d_go = bw["d_sdf"].view(-1, 1), bw["d_go"]
            dweff = eng.point_backward(pctx, ctx.weff, ctx.packed, d_sdf, d_go, bw["d_rgb"], dweff=dweff, staged=not ctx.chunk_rays)
            del pctx
        # inv_s = clip(exp(10 var), 1e-6, 1e6)  (endosurf.py:168, :852): d var = d inv_s * 10 exp(10 var) inside the clip range
        dvar = eng.variance_terms(var, d_invs_acc=d_invs_acc).reshape(ctx.variance.shape)
        ctx.pctx = None                                           # release the workspace as soon as it has been consumed
        if tail is not None:
            tail.close(eng)
        return dweff, None, dvar, None, None, None, None, None, None, None, None, None, None

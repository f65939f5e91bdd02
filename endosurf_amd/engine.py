"""Thin torch <-> C-ABI plumbing: allocates device buffers with torch, hands raw pointers to libendosurf_hip
on torch's current HIP stream.  No arithmetic happens here; every method is one or a few kernel launches."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import check, es_composite_args, es_points, ptr, stream_ptr


def f32(t: torch.Tensor) -> torch.Tensor:
    """``t`` as the library reads it: detached, fp32, contiguous (no copy when it already is fp32 and contiguous)."""
    return t.detach().to(torch.float32).contiguous()


def u8(valid: torch.Tensor) -> torch.Tensor:
    """A per-ray validity mask as the bytes the library reads (a bool tensor is reinterpreted, not converted)."""
    return (valid.view(torch.uint8) if valid.dtype == torch.bool else valid.to(torch.uint8)).contiguous()


class PointCtx:
    """Workspace of one fused point evaluation + typed views of its outputs."""
    _OUT = {"xc": (_lib.WS_XC, 3), "v": (_lib.WS_V, 3), "sdf": (_lib.WS_SDF, 1), "feat": (_lib.WS_FEAT, 256),
            "gc": (_lib.WS_GC, 3), "go": (_lib.WS_GO, 3), "rgb": (_lib.WS_RGB, 3), "curv": (_lib.WS_CURV, 3), "xcbar": (_lib.WS_XCBAR, 3),
            "tbar": (_lib.WS_TBAR, 1), "vbar": (_lib.WS_VBAR, 3)}

    def __init__(self, eng: "Engine", pts, flags: int, m_color: int = 0):
        self.eng, self.pts, self.flags, self.M, self.m_color = eng, pts, flags, pts.M, int(m_color)
        self.x3_chain, self.px3 = False, None      # set by Engine.point_forward when the split-precision training chain produced it
        self.Mp = (self.M + 127) // 128 * 128        # csrc/workspace.h round_up_rows
        n = int(eng.lib.es_point_workspace_floats(self.M, flags))
        self.ws = eng.empty(max(n, 1))

    def view(self, name):
        buf, width = self._OUT[name]
        off = int(self.eng.lib.es_point_workspace_offset(self.M, self.flags, buf))
        v = self.ws[off:off + self.Mp * width].view(self.Mp, width)[:self.M]
        return v


class Engine:
    """Per-device handle (stateless apart from the loaded library)."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.EndoSurfHipError(
                f"endosurf_amd runs its hot path on an AMD GPU through HIP only (got device {device!r}); there is no CPU path")
        self.lib = _lib.load()
        with torch.cuda.device(self.device):
            check(self.lib.es_init(), "es_init")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_param = int(self.lib.es_param_floats())
        self.n_weff = int(self.lib.es_weff_floats())
        self.n_packed = int(self.lib.es_packed_floats())
        import os
        # Supported environment variables (README): ES_SPLIT_BF16, ES_DETERMINISTIC (here), ES_WORKSPACE_GB (renderer).  Everything else
        # below is an attribute only -- measurement code sets ``renderer.engine.<name>``, nothing reads development switches from the
        # environment any more.
        # ray marching evaluates its proposals in blocks of this many steps with early exit (0: one launch over all proposals)
        self.march_block = 32
        # deterministic mode: batch sums and weight gradients are reduced in a fixed order instead of with fp32 atomics
        # (bit-identical results from run to run; a few % slower).  Also settable per renderer: ``renderer.engine.deterministic = True``
        self.deterministic = os.environ.get("ES_DETERMINISTIC", "0") not in ("0", "", "false", "False")
        self._wg_scratch = None
        # opt-in split-precision mode (csrc/query_x3.hip, wgrad.hip): the large no-grad SDF queries (coarse samples, ray-marching
        # proposals, field extraction) and the weight-gradient GEMMs run on the bf16 matrix pipes with every fp32 operand split
        # exactly into three bf16 planes (six partial products, fp32 accumulation): fp32-class accuracy at ~2.7x the fp32 MFMA rate.
        # NOT the default; also settable per renderer through render_cfg["split_precision"] / ``renderer.engine.split_precision = True``
        self.split_precision = os.environ.get("ES_SPLIT_BF16", "0") not in ("0", "", "false", "False")
        self._x3 = None
        self.x3_query_min = 8193
        self.x3_infer_min = 16384      # points: below this a launch of 64/128-point tiles does not fill the chip
        # split-precision mode: grad-enabled evaluations run the split-precision TRAINING chain (infer_x3r.hip with saves +
        # train_x3r.hip); False keeps the fp32 chain kernels under the split-precision queries / weight gradients (round-2 behaviour)
        self.x3_train_chain = True
        # (the SDF network stays on the fp32 kernels in the training chain: csrc/infer_x3r.hip)
        # step arena (round 4): inside Trainer's step ``zeros`` hands out slices of ONE buffer that one memset cleared (arena_begin)
        self._arena, self._arena_off, self._arena_on = None, 0, False
        self._ones1 = None
        self._rng_calls = 0
        self._rng_step_calls = 0          # draws of the current step with a device-resident step counter (uniform)
        # set by a data-parallel Trainer with overlap_allreduce: called as hook(stage, dweff) behind each weight-gradient launch of a step
        self.wgrad_stage_hook = None
        self._grad_pipeline = None          # state of a pipelined data-parallel step (trainer.Trainer._train_step_pipelined)

    def st(self):
        """torch's current HIP stream ON THIS ENGINE'S DEVICE.  The library launches on the current HIP device, so the caller must
        be inside ``torch.cuda.device(engine.device)`` (the renderer's public methods and autograd's backward are)."""
        if torch.cuda.current_device() != self.device.index:
            raise _lib.EndoSurfHipError(
                f"engine for {self.device} used while the current device is cuda:{torch.cuda.current_device()}; "
                f"wrap the call in torch.cuda.device({self.device.index})")
        return stream_ptr(self.device)

    def wg_scratch(self):
        """Scratch of the deterministic weight-gradient reduction (allocated once, ~80 MB), or None in the default mode."""
        if not self.deterministic:
            return None
        if self._wg_scratch is None:
            self._wg_scratch = self.empty(int(self.lib.es_wgrad_scratch_floats()))
        return self._wg_scratch

    # ---- buffers ----------------------------------------------------------------------------------
    def empty(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, device=self.device, dtype=dtype)

    def zeros(self, *shape, dtype=torch.float32):
        if self._arena_on and dtype == torch.float32:
            shp = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
            n = 1
            for s in shp:
                n *= int(s)
            off = self._arena_off
            if 0 < n and off + n <= self._arena.numel():
                self._arena_off = off + (n + 63) // 64 * 64          # 256-byte aligned slices
                return self._arena[off:off + n].view(shp)
        return torch.zeros(*shape, device=self.device, dtype=dtype)

    # ---- step arena / step plumbing (csrc/step.hip) --------------------------------------------------
    def arena_begin(self, extra_floats: int = 0):
        """Start of a training step: every ``zeros`` until ``arena_end`` is a slice of one buffer cleared by ONE memset (the eikonal
        sums, the inv_s adjoint, the effective-weight and parameter gradient buffers, the marching scratch ...) instead of a fill
        launch each.  The slices are valid until the next ``arena_begin`` (the flat gradient of a step lives here: it is consumed by the
        optimiser within the step; ``.grad`` views read as zeros once the next step has begun)."""
        need = self.n_weff + self.n_param + 4096 + int(extra_floats) + 64 * 32
        need = (need + 4095) // 4096 * 4096          # (a 16-KB multiple: the runtime clears it with one fill kernel, not body + remainder)
        if self._arena is None or self._arena.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.EndoSurfHipError("the step arena must exist before a step is captured (run one eager step first)")
            self._arena = self.empty(need)
        self.zero(self._arena)
        self._arena_off, self._arena_on = 0, True
        self._rng_step_calls = 0

    def arena_end(self):
        self._arena_on = False

    @property
    def ones1(self) -> torch.Tensor:
        """A persistent device [1] holding 1.0: the seed of a step's backward pass (``loss.backward(gradient=...)``: no fill launch, and
        the loss node recognises it by address and hands its adjoints on unscaled)."""
        if self._ones1 is None:
            self._ones1 = torch.ones(1, device=self.device)
        return self._ones1

    def uniform(self, n: int, step_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
        """n uniform draws in [0, 1) in ONE launch (Philox4x32-10 keyed by torch's seed).  Eager steps: subsequence = this engine's call
        index.  Graph-mode steps: subsequence = 2^63 + the device-resident step counter, so that replays draw new numbers."""
        out = self.empty(int(n))
        seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        if step_dev is not None:
            # graph-mode steps (the two eager warm-up calls and every replay) draw from subsequences 2^63 + (k << 40) + step counter, k = the
            # index of the call within its step (reset by arena_begin): a space disjoint from the eager steps' call index below, so that
            # mixing train_step and train_step_graph never repeats a stream, and two draws of one step never share one
            sub = (1 << 63) + (self._rng_step_calls << 40)
            self._rng_step_calls += 1
        else:
            sub = self._rng_calls
            self._rng_calls += 1
        check(self.lib.es_uniform(ptr(out), int(n), seed, sub, ptr(step_dev) if step_dev is not None else None, self.st()), "es_uniform")
        return out

    # ---- weights ----------------------------------------------------------------------------------
    def weightnorm_pack(self, flat_params: torch.Tensor, use_deform: bool):
        weff = self.empty(self.n_weff)
        packed = self.empty(self.n_packed)
        if not use_deform:
            self.zero(weff)
        check(self.lib.es_weightnorm_pack(ptr(flat_params), ptr(weff), ptr(packed), int(use_deform), self.st()), "es_weightnorm_pack")
        return weff, packed

    def weightnorm_backward_layers(self, flat_params, dweff, dparams, first_layer: int, n_layers: int):
        """Layers [first_layer, first_layer + n_layers) of the 27 (9 * network + layer) into their slices of ``dparams``."""
        check(self.lib.es_weightnorm_backward_layers(ptr(flat_params), ptr(dweff), ptr(dparams), int(first_layer), int(n_layers), self.st()),
              "es_weightnorm_backward_layers")

    def weightnorm_backward(self, flat_params, dweff, use_deform: bool):
        dparams = self.zeros(self.n_param)
        check(self.lib.es_weightnorm_backward(ptr(flat_params), ptr(dweff), ptr(dparams), int(use_deform), self.st()),
              "es_weightnorm_backward")
        return dparams

    # ---- point sources ----------------------------------------------------------------------------
    @staticmethod
    def points(x=None, t=None, dirs=None, rays=None, z=None, n_per_ray=1, ldz=None, M=None) -> es_points:
        """mode 0: explicit (x, t[, dirs]); mode 1: ray samples (rays, z); mode 2: ray samples followed by explicit (x, t)."""
        p = es_points()
        if rays is not None:
            p.rays, p.z = ptr(rays), ptr(z)
            p.n_per_ray = int(n_per_ray)
            p.ldz = int(ldz if ldz is not None else z.shape[-1])
            n_ray_pts = rays.shape[0] * n_per_ray
            if x is not None:
                p.mode, p.M_split = 2, n_ray_pts
                p.x, p.t = ptr(x), ptr(t)
                p.t_scalar = 0
                p.M = n_ray_pts + x.shape[0]
            else:
                p.mode = 1
                p.M = int(M if M is not None else n_ray_pts)
            p._keep = (rays, z, x, t)
        else:
            p.mode = 0
            p.x, p.t = ptr(x), ptr(t)
            p.dirs = ptr(dirs) if dirs is not None else None
            p.t_scalar = 1 if t.numel() == 1 and x.shape[0] != 1 else 0
            p.n_per_ray, p.ldz = 1, 1
            p.M = int(M if M is not None else x.shape[0])
            p._keep = (x, t, dirs)
        return p

    def packed_x3(self, weff, use_deform: bool):
        """The split-precision packing of ``weff``, one entry per ``use_deform`` (a deform model also evaluates canonical-space points
        with the deformation network switched off), rebuilt when a new effective-weight buffer shows up.  An entry keeps its source
        buffer alive (so that its address cannot be recycled for other weights) and the event recorded behind the packing launch:
        a consumer on ANOTHER stream waits for it (the sampling chain of a training step runs on a side stream)."""
        if self._x3 is None or self._x3["ptr"] != weff.data_ptr():
            self._x3 = {"ptr": weff.data_ptr(), "src": weff.detach(), "packs": {}}
        packs = self._x3["packs"]
        cur = torch.cuda.current_stream(self.device)
        e = packs.get(bool(use_deform))
        if e is None:
            buf = torch.empty(int(self.lib.es_packed_x3_bytes()), device=self.device, dtype=torch.uint8)
            check(self.lib.es_pack_x3(ptr(weff), ptr(buf), int(use_deform), self.st()), "es_pack_x3")
            ev = torch.cuda.Event()
            ev.record(cur)
            e = packs[bool(use_deform)] = (buf, ev, cur)
        elif e[2] != cur:
            cur.wait_event(e[1])
            if not torch.cuda.is_current_stream_capturing():
                e[0].record_stream(cur)
        return e[0]

    def x3_buffers(self):
        """The split-precision packings currently cached (a captured hipGraph keeps them alive: it holds their raw pointers)."""
        return [] if self._x3 is None else [self._x3["src"]] + [e[0] for e in self._x3["packs"].values()]

    def _use_x3(self, M: int) -> bool:
        # small batches (the 1024-point secant queries, the 8 192-point up-sampling queries) are latency-bound chains: they stay on the
        # 16-point fp32 tiles.  The library's split-precision query runs 128-point register-resident blocks whatever the batch size: 64
        # blocks at 8 192 points leave most of the chip idle, and a 32-point split tile built for these sizes measured SLOWER than fp32
        # (0.27 vs 0.21 ms at 8 192 points, 0.27 vs 0.17 at 1 024: DEAD_ENDS B4), so the threshold stays above them
        return self.split_precision and M >= self.x3_query_min

    def query_sdf(self, pts: es_points, weff, packed, use_deform: bool, tile_points: int = 0) -> torch.Tensor:
        """``tile_points``: 16 / 32 / 64 points per workgroup, 0 = the library's choice by batch size (es_query_sdf_tiles)."""
        out = self.empty(pts.M)
        if self._use_x3(pts.M):
            check(self.lib.es_query_sdf_x3(C.byref(pts), ptr(self.packed_x3(weff, use_deform)), ptr(weff), ptr(out), 0, None, int(use_deform),
                                           self.st()), "es_query_sdf_x3")
            return out
        if tile_points:
            check(self.lib.es_query_sdf_tiles(C.byref(pts), ptr(packed), ptr(weff), ptr(out), int(use_deform), int(tile_points), self.st()),
                  "es_query_sdf_tiles")
            return out
        check(self.lib.es_query_sdf(C.byref(pts), ptr(packed), ptr(weff), ptr(out), int(use_deform), self.st()), "es_query_sdf")
        return out

    # ---- per-ray kernels --------------------------------------------------------------------------
    def ray_setup(self, rays, u, n, sample_dist, lin_mode, z, want_bounds=False):
        N = rays.shape[0]
        near = self.empty(N) if want_bounds else None
        far = self.empty(N) if want_bounds else None
        check(self.lib.es_ray_setup(ptr(rays), ptr(u) if u is not None else None, N, n, float(sample_dist), lin_mode, ptr(z),
                                    z.shape[1], ptr(near), ptr(far), self.st()), "es_ray_setup")
        return near, far

    def sample_z(self, rays, u_perturb, weff, packed, use_deform, n_samples, n_importance, up_sample_steps, upsample: bool,
                 trace: Optional[list] = None, racing: bool = False):
        """Coarse sampling + SDF-guided hierarchical up-sampling (reference render_rays, endosurf.py:71-110).
        Returns z [N, S] (S = n_samples (+ up_sample_steps * (n_importance // up_sample_steps))).  ``racing``: this chain shares the GPU
        with another chain of small launches (the secant iterations of a training step): its coarse query runs on 32-point tiles
        (es_query_sdf_tiles)."""
        N = rays.shape[0]
        n = n_samples
        sample_dist = 2.0 / n_samples
        do_up = upsample and n_importance > 0 and up_sample_steps > 0
        n_imp = n_importance // up_sample_steps if do_up else 0
        if do_up and n_imp == 0:
            raise ValueError(f"n_importance = {n_importance} gives no new sample in any of the {up_sample_steps} up-sampling steps")
        # what the steps really add: up_sample_steps * (n_importance // up_sample_steps) columns, like the reference's loop
        # (endosurf.py:95-110) -- fewer than n_importance when it is not a multiple of up_sample_steps
        S = n + up_sample_steps * n_imp
        if do_up and not racing and trace is None and N > 0 and n_importance % up_sample_steps == 0 and not self._use_x3(N * n):
            # the same launches in the same order, issued by ONE library call (es_sample_z) instead of ~15: a step that ends in a host
            # sync (the reference trainer's loss.item()) starts with an empty queue, and this chain of small launches is where the GPU
            # would wait for the host
            z_out = self.empty(N, S)
            scratch = self.empty(int(self.lib.es_sample_scratch_floats(N, n_samples, n_importance, up_sample_steps)))
            check(self.lib.es_sample_z(ptr(rays), ptr(u_perturb) if u_perturb is not None else None, N, n_samples, n_importance, up_sample_steps, 1,
                                       ptr(packed), ptr(weff), int(use_deform), ptr(z_out), ptr(scratch), self.st()), "es_sample_z")
            return z_out
        zc = self.empty(N, S)
        self.ray_setup(rays, u_perturb, n, sample_dist, 0, zc)
        if trace is not None:
            trace.append(zc[:, :n].clone())
        if not do_up:
            return zc
        zn = self.empty(N, S)
        # (racing: never TALLER than 32 points -- a batch the library would give 16- or 32-point tiles anyway keeps the library's choice)
        sdf_c = self.query_sdf(self.points(rays=rays, z=zc, n_per_ray=n, ldz=S), weff, packed, use_deform,
                               tile_points=_lib.QUERY_TILE_RACING if racing and N * n > 16384 else 0).view(N, n)
        ld_sdf = n
        sdf_a, sdf_b = self.empty(N, S), self.empty(N, S)
        src = self.empty(N, S, dtype=torch.int32)
        z_new = self.empty(N, n_imp)
        for i in range(up_sample_steps):
            self.upsample_step(rays, zc, S, sdf_c, ld_sdf, N, n, n_imp, 64 * 2 ** i, z_new, zn, S, src)
            if i + 1 != up_sample_steps:
                sdf_new = self.query_sdf(self.points(rays=rays, z=z_new, n_per_ray=n_imp, ldz=n_imp), weff, packed, use_deform)
                dst = sdf_a if sdf_c.data_ptr() != sdf_a.data_ptr() else sdf_b
                self.merge_sdf(sdf_c, ld_sdf, sdf_new, n_imp, src, S, N, n, dst)
                sdf_c, ld_sdf = dst, S
            zc, zn = zn, zc
            n += n_imp
            if trace is not None:
                trace.append(zc[:, :n].clone())
        return zc

    def mid_z(self, z, sample_dist):
        N, S = z.shape
        mid = self.empty(N, S)
        check(self.lib.es_mid_z(ptr(z), S, N, S, float(sample_dist), ptr(mid), self.st()), "es_mid_z")
        return mid

    def composite_args(self, rays, z, sdf, g_o, rgb, variance, sample_dist, cos_anneal) -> es_composite_args:
        a = es_composite_args()
        N, S = z.shape
        a.rays, a.z, a.ldz = ptr(rays), ptr(z), S
        a.sdf, a.g_o, a.rgb, a.variance = ptr(sdf), ptr(g_o), ptr(rgb), ptr(variance)
        a.N, a.S, a.sample_dist = N, S, float(sample_dist)
        if torch.is_tensor(cos_anneal):          # device scalar (a captured training step updates it between replays)
            a.cos_anneal, a.cos_anneal_dev = 0.0, ptr(cos_anneal)
        else:
            a.cos_anneal, a.cos_anneal_dev = float(cos_anneal), None
        a._keep = [rays, z, sdf, g_o, rgb, variance, cos_anneal]
        if self.deterministic:
            part = self.empty(N, 2)
            a.ray_part = ptr(part)
            a._keep.append(part)
        return a

    def composite_forward(self, a: es_composite_args, eik_acc=None, go_copy: bool = False):
        """``eik_acc`` [2] (optional): accumulate the eikonal sums into an existing buffer (chunked renders).  ``go_copy``: the kernel
        also writes the samples' g_o rows into storage of their own (out["go"] [N,S,3]: the renderer's ``gradients_o``)."""
        N, S = a.N, a.S
        out = dict(color=self.empty(N, 3), depth=self.empty(N, 1), weights=self.empty(N, S), cdf=self.empty(N, S),
                   weight_max=self.empty(N, 1), eik_acc=eik_acc if eik_acc is not None else self.zeros(2),
                   wmax_idx=self.empty(N, dtype=torch.int32))
        for k, v in out.items():
            setattr(a, k, ptr(v))
        if go_copy:
            out["go"] = self.empty(N, S, 3)
            a.go_copy = ptr(out["go"])
        a._keep.append(out)
        check(self.lib.es_composite_forward(C.byref(a), self.st()), "es_composite_forward")
        return out

    def composite_backward(self, a: es_composite_args, g_color, g_depth, g_eik, eik_den, g_weights=None, g_cdf=None, g_wmax=None,
                           g_gradients_o=None, d_invs_acc=None, n_aux: int = 0, g_aux_sdf=None, g_aux_go=None):
        """``n_aux`` > 0: d_sdf / d_go get n_aux extra rows behind the N*S sample rows, filled by the same launch with the auxiliary
        points' adjoints (None = zeros): the row order of the fused point evaluation, no concatenation."""
        N, S = a.N, a.S
        out = dict(d_sdf=self.empty(N * S + n_aux), d_go=self.empty(N * S + n_aux, 3), d_rgb=self.empty(N * S, 3),
                   d_invs_acc=d_invs_acc if d_invs_acc is not None else self.zeros(1))
        keep = [g_color, g_depth, g_eik, eik_den, g_weights, g_cdf, g_wmax, g_gradients_o, g_aux_sdf, g_aux_go]
        a.n_aux = int(n_aux)
        a.g_aux_sdf = ptr(g_aux_sdf) if (n_aux and g_aux_sdf is not None) else None
        a.g_aux_go = ptr(g_aux_go) if (n_aux and g_aux_go is not None) else None
        a.g_color, a.g_depth, a.g_eik, a.eik_den = ptr(g_color), ptr(g_depth), ptr(g_eik), ptr(eik_den)
        a.g_weights = ptr(g_weights) if g_weights is not None else None
        a.g_cdf = ptr(g_cdf) if g_cdf is not None else None
        a.g_wmax = ptr(g_wmax) if g_wmax is not None else None
        a.g_gradients_o = ptr(g_gradients_o) if g_gradients_o is not None else None
        for k, v in out.items():
            setattr(a, k, ptr(v))
        a._keep += keep + [out]
        check(self.lib.es_composite_backward(C.byref(a), self.st()), "es_composite_backward")
        return out

    # ---- ray marching ------------------------------------------------------------------------------
    def variance_terms(self, variance, d_invs_acc=None):
        """SingleVarianceNetwork's scalar epilogue: s_val = 1 / inv_s, or (with ``d_invs_acc``) the gradient of the variance."""
        out = self.empty(1)
        v = f32(variance).reshape(1)
        if d_invs_acc is None:
            check(self.lib.es_variance_terms(ptr(v), None, ptr(out), None, self.st()), "es_variance_terms")
        else:
            check(self.lib.es_variance_terms(ptr(v), ptr(d_invs_acc), None, ptr(out), self.st()), "es_variance_terms")
        return out

    def march_begin(self, rays, weff, packed, use_deform, n_steps=128, tau=0.0):
        """First half of ray_marching (reference endosurf.py:352-406): SDF at n_steps proposals per ray (one big launch) and the
        first sign change -> secant bracket. Returns the state consumed by march_refine."""
        N = rays.shape[0]
        dprop = self.empty(N, n_steps)
        self.ray_setup(rays, None, n_steps, 0.0, 1, dprop)
        B = self.march_block
        if B and n_steps % B == 0 and n_steps > B and N * B >= 16384:
            # proposals in blocks of B steps; a ray is finished at its first sign change (nothing behind it can change the
            # reference's result), and tiles whose rays are all finished return at once
            sdf = self.zeros(N, n_steps)                 # skipped proposals read as 0: no sign change
            done = self.empty(N, dtype=torch.int32)
            for b in range(n_steps // B):
                p = self.points(rays=rays, z=dprop, n_per_ray=B, ldz=n_steps)
                p.z = C.c_void_p(dprop.data_ptr() + 4 * b * B)
                if self._use_x3(p.M):
                    check(self.lib.es_query_sdf_x3(C.byref(p), ptr(self.packed_x3(weff, use_deform)), ptr(weff),
                                                   C.c_void_p(sdf.data_ptr() + 4 * b * B), n_steps, ptr(done) if b else None, int(use_deform),
                                                   self.st()), "es_query_sdf_x3")
                else:
                    check(self.lib.es_query_sdf_rays(C.byref(p), ptr(packed), ptr(weff), C.c_void_p(sdf.data_ptr() + 4 * b * B), n_steps,
                                                     ptr(done) if b else None, int(use_deform), self.st()), "es_query_sdf_rays")
                if b + 1 < n_steps // B:
                    check(self.lib.es_march_progress(ptr(sdf), N, n_steps, (b + 1) * B, float(tau), ptr(done), self.st()), "es_march_progress")
        else:
            sdf = self.query_sdf(self.points(rays=rays, z=dprop, n_per_ray=n_steps, ldz=n_steps), weff, packed, use_deform)
        state = self.empty(N, 4)
        flags = self.empty(N, dtype=torch.int32)
        d_pred = self.empty(N)
        check(self.lib.es_march_find(ptr(sdf), ptr(dprop), N, n_steps, float(tau), ptr(state), ptr(flags), ptr(d_pred), self.st()),
              "es_march_find")
        return dict(rays=rays, weff=weff, packed=packed, use_deform=use_deform, tau=float(tau), state=state, flags=flags, d_pred=d_pred,
                    keep=(dprop, sdf))

    def march_refine(self, ms, n_secant_steps=8):
        """Second half (endosurf.py:410-449): n_secant_steps dependent secant iterations (latency-bound small launches)."""
        rays, N = ms["rays"], ms["rays"].shape[0]
        x = self.empty(N, 3)
        t = self.empty(N)
        for _ in range(n_secant_steps):
            self.secant_points(rays, ms["d_pred"], N, x, t)
            f_mid = self.query_sdf(self.points(x=x, t=t), ms["weff"], ms["packed"], ms["use_deform"])
            self.secant_update(f_mid, N, ms["tau"], ms["state"], ms["d_pred"])
        d_out = self.empty(N, 1)
        check(self.lib.es_march_finish(ptr(ms["d_pred"]), ptr(ms["flags"]), N, ptr(d_out), self.st()), "es_march_finish")
        return d_out

    def ray_marching(self, rays, weff, packed, use_deform, n_steps=128, n_secant_steps=8, tau=0.0):
        """ray_marching + secant (reference endosurf.py:344-449), fixed shape. Returns d_pred [N,1]."""
        N = rays.shape[0]
        B = self.march_block
        blocks = bool(B and n_steps % B == 0 and n_steps > B and N * B >= 16384)
        if N > 0 and not self._use_x3(N * (B if blocks else n_steps)):
            # ONE library call (es_ray_marching) issues the proposals' queries, the bracket search and the secant iterations (~30 launches)
            d_out = self.empty(N, 1)
            scratch = self.empty(int(self.lib.es_march_scratch_floats(N, n_steps)))
            check(self.lib.es_ray_marching(ptr(rays), N, int(n_steps), int(n_secant_steps), float(tau), int(B) if blocks else 0, ptr(packed), ptr(weff),
                                           int(use_deform), ptr(d_out), ptr(scratch), self.st()), "es_ray_marching")
            return d_out
        return self.march_refine(self.march_begin(rays, weff, packed, use_deform, n_steps, tau), n_secant_steps)

    # ---- fused point evaluation --------------------------------------------------------------------
    def point_forward(self, pts, weff, packed, flags: int, m_color: int = 0, fp32_only: bool = False) -> PointCtx:
        """``fp32_only``: keep the evaluation on the fp32 kernels in split-precision mode too (the point adjoint reads their mask words)."""
        ctx = PointCtx(self, pts, flags, m_color)
        save = bool(flags & _lib.PF_SAVE)
        if self.split_precision and pts.M >= self.x3_infer_min and (self.x3_train_chain or not save) and not fp32_only:
            # opt-in: the launches of a large evaluation in split precision -- csrc/infer_x3r.hip without PF_SAVE; with PF_SAVE the
            # split-precision TRAINING chain, whose workspace must go through es_point_backward_x3 (``ctx.x3_chain``)
            px3 = self.packed_x3(weff, bool(flags & _lib.PF_DEFORM))
            check(self.lib.es_point_forward_x3(C.byref(pts), ptr(packed), ptr(px3), ptr(weff), ptr(ctx.ws), flags, int(m_color),
                                               self.st()), "es_point_forward_x3")
            ctx.x3_chain = save
            ctx.px3 = px3
        else:
            check(self.lib.es_point_forward(C.byref(pts), ptr(packed), ptr(weff), ptr(ctx.ws), flags, int(m_color), self.st()), "es_point_forward")
        return ctx

    def point_forward_rows(self, ctx: PointCtx, weff, packed, row0: int, nrows: int):
        """Rows [row0, row0 + nrows) of a workspace that is filled piece by piece (es_point_forward_rows): the colour part of a render whose
        workspace has room for the colour-less points of later calls, or one of those calls' pieces of the tail.  fp32 kernels."""
        check(self.lib.es_point_forward_rows(C.byref(ctx.pts), ptr(packed), ptr(weff), ptr(ctx.ws), ctx.flags, ctx.m_color, int(row0), int(nrows),
                                             self.st()), "es_point_forward_rows")

    def point_backward(self, ctx: PointCtx, weff, packed, d_sdf, d_go, d_rgb=None, dweff=None, staged: bool = False):
        """Adjoints of (sdf [M,1], g_o [M,3], rgb [M,3]) -> gradient w.r.t. the effective-weight buffer (accumulated into
        ``dweff`` if given).  ``staged``: this call produces the WHOLE gradient of a step (not one chunk of several), so
        ``engine.wgrad_stage_hook(stage, dweff)`` -- if set -- may be called behind every network's weight-gradient launch."""
        M = ctx.M
        z = lambda g, w: (f32(g) if g is not None else self.zeros(M, w))
        d_sdf, d_go = z(d_sdf, 1), z(d_go, 3)
        color = bool(ctx.flags & _lib.PF_COLOR)
        if color:
            mc = ctx.m_color if ctx.m_color > 0 else M
            d_rgb = f32(d_rgb) if d_rgb is not None else self.zeros(mc, 3)
            assert d_rgb.shape[0] == mc
        if dweff is None:
            dweff = self.zeros(self.n_weff)
            if self._grad_pipeline is not None:          # a pipelined data-parallel step counts the gradient buffers of its weff consumers
                self._grad_pipeline["buffers"] = self._grad_pipeline.get("buffers", 0) + 1
        if ctx.x3_chain:      # the workspace of the split-precision training chain: that family's backward kernels
            check(self.lib.es_point_backward_x3(C.byref(ctx.pts), ptr(packed), ptr(ctx.px3), ptr(weff), ptr(ctx.ws), ctx.flags, ctx.m_color, ptr(d_sdf),
                                                ptr(d_go), ptr(d_rgb) if color else None, ptr(dweff), ptr(self.wg_scratch()), self.st()),
                  "es_point_backward_x3")
            return dweff
        flags = ctx.flags | (_lib.PF_X3 if self.split_precision else 0)      # opt-in: weight-gradient GEMMs in split precision
        hook = self.wgrad_stage_hook if staged else None
        if hook is not None:
            # the same launches in four calls, with the caller's hook between them: a data-parallel trainer starts the all-reduce of a
            # network's gradient while the next network's weight-gradient launch runs (Trainer(overlap_allreduce=True))
            for stage in (_lib.BWD_CHAINS, _lib.BWD_WGRAD_DEFORM, _lib.BWD_WGRAD_SDF, _lib.BWD_WGRAD_COLOR):
                check(self.lib.es_point_backward_stages(C.byref(ctx.pts), ptr(packed), ptr(weff), ptr(ctx.ws), flags, ctx.m_color, ptr(d_sdf), ptr(d_go),
                                                        ptr(d_rgb) if color else None, ptr(dweff), ptr(self.wg_scratch()), stage, self.st()),
                      "es_point_backward_stages")
                if stage != _lib.BWD_CHAINS:
                    hook(stage, dweff)
            return dweff
        check(self.lib.es_point_backward_det(C.byref(ctx.pts), ptr(packed), ptr(weff), ptr(ctx.ws), flags, ctx.m_color, ptr(d_sdf), ptr(d_go),
                                             ptr(d_rgb) if color else None, ptr(dweff), ptr(self.wg_scratch()), self.st()), "es_point_backward")
        return dweff

    def point_input_adjoint(self, ctx: PointCtx, weff, packed, d_sdf, d_go):
        """The adjoint of the QUERY POINTS through g_o (and only through g_o: callers that expose sdf as a function of the points attach
        d sdf / d x = g_o themselves, model.EndoSurfNet.get_sdf_from_observed_space) -- the reference's create_graph=True second
        derivative (endosurf.py:581-601, :603-619).  Call right after point_backward on the same context:
            xbar = J^T xcbar - d_go * curv(g_c) - d_sdf * g_o        (include/endosurf_hip.h es_point_vjp; without a deformation network J = I)
        where xcbar (the backward's adjoint of x_c) carries the Hessian-vector product of the SDF network along J d_go, the curvature term is
        the deformation network's own second derivative, and the last term removes the sdf path's share of xcbar.  Overwrites the
        workspace's g_c / g_o / curvature buffers."""
        M = ctx.M
        if ctx.x3_chain:
            raise _lib.EndoSurfHipError("the point adjoint needs a workspace of the fp32 kernels (point_forward(..., fp32_only=True))")
        xcbar = ctx.view("xcbar")
        go = ctx.view("go").clone()
        if ctx.flags & _lib.PF_DEFORM:
            curv = ctx.view("curv").clone()
            ctx.view("gc").copy_(xcbar)
            self.point_vjp(ctx, weff, packed)
            xbar = ctx.view("go").clone()
            if d_go is not None:
                xbar -= d_go.detach().to(torch.float32).reshape(M, 3) * curv
        else:
            xbar = xcbar.clone()
        if d_sdf is not None:
            xbar -= d_sdf.detach().to(torch.float32).reshape(M, 1) * go
        return xbar

    # ---- single launches ----------------------------------------------------------------------------
    # One method per library entry point that the renderer, its autograd functions and the trainer call: the pointer marshalling and the
    # status check, nothing else (tensors or None in; the caller allocates, converts and owns every buffer).  Arguments in the order of
    # include/endosurf_hip.h, which documents them -- except that ``weff`` comes before ``packed``, as everywhere in this class.
    def copy2(self, dst_a, src_a, n_a, dst_b, src_b, n_b):
        check(self.lib.es_copy2(ptr(dst_a), ptr(src_a), int(n_a), ptr(dst_b), ptr(src_b), int(n_b), self.st()), "es_copy2")
    def zero(self, buf):
        check(self.lib.es_zero(ptr(buf), 4 * buf.numel(), self.st()), "es_zero")
    def scale(self, out, src, n, factor_dev):
        check(self.lib.es_scale(ptr(out), ptr(src), int(n), ptr(factor_dev), self.st()), "es_scale")

    def color_forward(self, ctx: PointCtx, weff, packed):
        check(self.lib.es_color_forward(C.byref(ctx.pts), ptr(packed), ptr(weff), ptr(ctx.ws), self.st()), "es_color_forward")
    def point_vjp(self, ctx: PointCtx, weff, packed):
        check(self.lib.es_point_vjp(C.byref(ctx.pts), ptr(packed), ptr(weff), ptr(ctx.ws), ctx.flags, self.st()), "es_point_vjp")
    def render_finish(self, eik_acc, aux_sdf_src, aux_go_src, n_aux, eik, den2, aux_sdf, aux_go):
        check(self.lib.es_render_finish(ptr(eik_acc), ptr(aux_sdf_src), ptr(aux_go_src), int(n_aux), ptr(eik), ptr(den2), ptr(aux_sdf), ptr(aux_go),
                                        self.st()), "es_render_finish")

    def upsample_step(self, rays, z, ldz, sdf, ld_sdf, N, n, n_imp, inv_s, z_new, z_out, ld_out, src):
        check(self.lib.es_upsample_step(ptr(rays), ptr(z), ldz, ptr(sdf), ld_sdf, N, n, n_imp, float(inv_s), ptr(z_new), ptr(z_out), ld_out, ptr(src),
                                        self.st()), "es_upsample_step")
    def merge_sdf(self, sdf, ld_sdf, sdf_new, n_new, src, ld_src, N, n, out):
        check(self.lib.es_merge_sdf(ptr(sdf), ld_sdf, ptr(sdf_new), n_new, ptr(src), ld_src, N, n, ptr(out), self.st()), "es_merge_sdf")

    def secant_points(self, rays, d_pred, N, x, t):
        check(self.lib.es_secant_points(ptr(rays), ptr(d_pred), N, ptr(x), ptr(t), self.st()), "es_secant_points")
    def secant_update(self, f_mid, N, tau, state, d_pred):
        check(self.lib.es_secant_update(ptr(f_mid), N, float(tau), ptr(state), ptr(d_pred), self.st()), "es_secant_update")

    def eod_points(self, rays, d_gt, mask, N, x, t, inside):
        check(self.lib.es_eod_points(ptr(rays), ptr(d_gt), ptr(mask), N, ptr(x), ptr(t), ptr(inside), self.st()), "es_eod_points")
    def eod_loss(self, rays, pts, mask, sdf, go, N, out, inside):
        check(self.lib.es_eod_loss(ptr(rays), ptr(pts), ptr(mask), ptr(sdf), ptr(go), N, ptr(out), ptr(inside), self.st()), "es_eod_loss")
    def eod_loss_backward(self, rays, inside, sdf, go, out, g_sdf_err, g_ang_err, N, d_sdf, d_go):
        check(self.lib.es_eod_loss_backward(ptr(rays), ptr(inside), ptr(sdf), ptr(go), ptr(out), ptr(g_sdf_err), ptr(g_ang_err), N, ptr(d_sdf),
                                            ptr(d_go), self.st()), "es_eod_loss_backward")
    def sn_points(self, rays, mask, d_i, u, neighbour_rad, N, x, t, valid):
        check(self.lib.es_sn_points(ptr(rays), ptr(mask), ptr(d_i), ptr(u), float(neighbour_rad), N, ptr(x), ptr(t), ptr(valid), self.st()), "es_sn_points")
    def sn_loss(self, g, valid8, N, out):
        check(self.lib.es_sn_loss(ptr(g), ptr(valid8), N, ptr(out), self.st()), "es_sn_loss")
    def sn_loss_backward(self, g, valid8, out, g_loss, N, d_g):
        check(self.lib.es_sn_loss_backward(ptr(g), ptr(valid8), ptr(out), ptr(g_loss), N, ptr(d_g), self.st()), "es_sn_loss_backward")

    def train_aux_points(self, rays, depth_gt, mask, d_i, u, neighbour_rad, N, x, t, valid):
        check(self.lib.es_train_aux_points(ptr(rays), ptr(depth_gt), ptr(mask), ptr(d_i), ptr(u), float(neighbour_rad), N, ptr(x), ptr(t), ptr(valid),
                                           self.st()), "es_train_aux_points")
    def train_loss(self, args):          # a filled es_loss_args (trainer._LossFn)
        check(self.lib.es_train_loss(C.byref(args), self.st()), "es_train_loss")
    def train_schedule(self, state, lr_init, n_iter, warm_up_end, lr_alpha, beta1, beta2, grad_scale, anneal_end, scalars):
        check(self.lib.es_train_schedule(ptr(state), float(lr_init), float(n_iter), float(warm_up_end), float(lr_alpha), float(beta1), float(beta2),
                                         grad_scale, float(anneal_end), ptr(scalars), self.st()), "es_train_schedule")
    def adam_step(self, flat, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, step_size, bc2_sqrt, grad_scale, grad_var, var_off):
        check(self.lib.es_adam_step(ptr(flat), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), n, beta1, beta2, eps, step_size, bc2_sqrt, float(grad_scale),
                                    ptr(grad_var), var_off, self.st()), "es_adam_step")
    def adam_step_dev(self, flat, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, scalars_dev, grad_var, var_off):
        check(self.lib.es_adam_step_dev(ptr(flat), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), n, beta1, beta2, eps, ptr(scalars_dev), ptr(grad_var),
                                        var_off, self.st()), "es_adam_step_dev")

    # ---- argument and scratch helpers of the geometry and evaluation entry points -----------------------
    def _scratch_bytes(self, fn_name, *dims):
        """What ``es_*_scratch_bytes`` answers for ``dims``; its -1 (sizes the library refuses) raises with the library's message."""
        nbytes = int(getattr(self.lib, fn_name)(*dims))
        if nbytes < 0:
            check(1, fn_name)
        return nbytes

    def _scratch(self, fn_name, *dims):
        return self.empty(self._scratch_bytes(fn_name, *dims), dtype=torch.uint8)

    def _tri_arg(self, tris, what):
        """``tris`` as the library reads it: int32 [T, 3], contiguous, on this device."""
        if tris.dim() != 2 or tris.shape[1] != 3 or tris.device != self.device or tris.dtype not in (torch.int32, torch.int64):
            raise _lib.EndoSurfHipError(f"{what} takes [T, 3] int32 / int64 triangles on {self.device} (got {tris.dtype} {tuple(tris.shape)} "
                                        f"on {tris.device})")
        return tris.detach().to(torch.int32).contiguous()

    def _rows3_arg(self, t, what, rows):
        """``t`` ([N, 3] on this device; ``rows`` names it in the message) as the library reads it: fp32, contiguous."""
        if t.dim() != 2 or t.shape[1] != 3 or t.device != self.device:
            raise _lib.EndoSurfHipError(f"{what} takes {rows} on {self.device} (got {tuple(t.shape)} on {t.device})")
        return f32(t)

    # ---- iso-surface extraction (csrc/iso.hip) -------------------------------------------------------
    def iso_surface(self, field: torch.Tensor, threshold: float = 0.0):
        """The level set ``field == threshold`` of a device field [nx, ny, nz] as a welded, oriented triangle mesh, triangulated like
        ``meshing.marching_tetrahedra``: (verts [V,3] fp32 in index coordinates, tris [T,3] int32, edge_ends [V,2] int32 = linear grid
        ids of each vertex's inside and outside end), all on the device.  The two counts are the only thing read back to the host."""
        if field.dim() != 3 or field.device != self.device:
            raise _lib.EndoSurfHipError(f"iso_surface takes a [nx, ny, nz] field on {self.device} (got {tuple(field.shape)} on {field.device})")
        u = f32(field)
        nx, ny, nz = (int(s) for s in u.shape)
        scratch = self._scratch("es_iso_scratch_bytes", nx, ny, nz)
        totals = self.empty(2, dtype=torch.int64)
        check(self.lib.es_iso_count(ptr(u), nx, ny, nz, float(threshold), ptr(scratch), ptr(totals), self.st()), "es_iso_count")
        V, T = (int(v) for v in totals.tolist())
        if max(V, T) >= 1 << 31:
            raise _lib.EndoSurfHipError(f"iso_surface: {V} vertices / {T} triangles do not fit int32 indices")
        verts, ends, tris = self.empty(V, 3), self.empty(V, 2, dtype=torch.int32), self.empty(T, 3, dtype=torch.int32)
        check(self.lib.es_iso_emit(ptr(u), nx, ny, nz, float(threshold), ptr(scratch), V, T, ptr(verts), ptr(ends), ptr(tris), self.st()), "es_iso_emit")
        return verts, tris, ends

    # ---- narrow-band field (csrc/band.hip) ---------------------------------------------------------------
    def band_field(self, sample, axes, threshold: float = 0.0, block: int = 8, lipschitz: float = 1.0, max_fraction: float = 0.5,
                   net_chunk: int = 1 << 22):
        """A device field [nx, ny, nz] on the lattice ``axes`` (three 1-D fp32 device tensors) whose ``iso_surface`` is the one of the
        densely sampled field, built from ``sample(x[M,3]) -> [M]`` (any device callable) evaluated near the level set only: the scheme,
        its exactness contract and its limit are those of ``meshing.band_field``, the numpy twin of this method (same block sets, same
        values; the kernels are csrc/band.hip).  ``sample`` sees at most ``net_chunk`` points per call and must give a point the same
        value whatever batch it arrives in.  The host reads two integers per round (the seeds, then each growth round).
        Returns (field, stats, block_round [nbx, nby, nbz] int32: 0 = never evaluated, 1 = seed, r = activated by growth round r - 1);
        ``stats``: dense_points, evaluated_points (coarse lattice and duplicated face points included), blocks, seed_blocks,
        active_blocks, rounds, fallback."""
        from .meshing import band_margin
        if len(axes) != 3 or any(a.dim() != 1 or a.device != self.device for a in axes):
            raise _lib.EndoSurfHipError(f"band_field takes three 1-D axes on {self.device}")
        ax = [f32(a) for a in axes]
        nx, ny, nz = (int(a.shape[0]) for a in ax)
        B, thr, chunk = int(block), float(threshold), max(1, int(net_chunk))
        scratch = self._scratch("es_band_scratch_bytes", nx, ny, nz, B)
        nb = [-(-(n - 1) // B) for n in (nx, ny, nz)]
        NB, N, Nc = nb[0] * nb[1] * nb[2], nx * ny * nz, (nb[0] + 1) * (nb[1] + 1) * (nb[2] + 1)
        ends = torch.stack([torch.stack([a[0], a[-1]]) for a in ax]).tolist()          # (one small read: the world size of a block)
        margin = band_margin(ends, (nx, ny, nz), B, lipschitz)
        totals = self.empty(2, dtype=torch.int64)
        axp, st = [ptr(a) for a in ax], self.st()

        def lattice(stride, total, out):          # sample the (coarse) lattice in runs of ``chunk`` points
            for p0 in range(0, total, chunk):
                c = min(chunk, total - p0)
                x = self.empty(c, 3)
                check(self.lib.es_band_lattice_points(*axp, nx, ny, nz, stride, p0, c, ptr(x), st), "es_band_lattice_points")
                out[p0:p0 + c] = sample(x).reshape(-1)

        coarse = self.empty(Nc)
        lattice(B, Nc, coarse)
        check(self.lib.es_band_seed(ptr(coarse), nx, ny, nz, B, thr, margin, ptr(scratch), ptr(totals), st), "es_band_seed")
        n_list, n_pts = (int(v) for v in totals.tolist())
        stats = {"dense_points": N, "evaluated_points": Nc, "blocks": NB, "seed_blocks": n_list, "active_blocks": n_list, "rounds": 0,
                 "fallback": False}
        field = self.empty(N)
        block_round = scratch[:4 * NB].view(torch.int32).view(*nb)
        if n_list > float(max_fraction) * NB:          # the band cannot win: sample the lattice itself
            lattice(1, N, field)
            stats.update(evaluated_points=Nc + N, active_blocks=NB, fallback=True)
            return field.view(nx, ny, nz), stats, block_round.clone()
        check(self.lib.es_band_fill(nx, ny, nz, B, ptr(scratch), ptr(field), st), "es_band_fill")
        r = 1
        while n_list:
            for m0 in range(0, n_pts, chunk):
                c = min(chunk, n_pts - m0)
                x = self.empty(c, 3)
                check(self.lib.es_band_points(*axp, nx, ny, nz, B, ptr(scratch), n_list, m0, c, ptr(x), st), "es_band_points")
                vals = f32(sample(x).reshape(-1))
                check(self.lib.es_band_scatter(ptr(vals), nx, ny, nz, B, ptr(scratch), n_list, m0, c, ptr(field), st), "es_band_scatter")
            stats["evaluated_points"] += n_pts
            check(self.lib.es_band_grow(ptr(field), nx, ny, nz, B, thr, r, ptr(scratch), ptr(totals), st), "es_band_grow")
            n_list, n_pts = (int(v) for v in totals.tolist())
            stats["active_blocks"] += n_list
            stats["rounds"] += 1 if n_list else 0
            r += 1
        return field.view(nx, ny, nz), stats, block_round.clone()

    def iso_surface_band(self, sample, axes, threshold: float = 0.0, block: int = 8, lipschitz: float = 1.0, max_fraction: float = 0.5,
                         net_chunk: int = 1 << 22):
        """``iso_surface`` of the field ``sample`` takes on the lattice ``axes``, sampled near the level set only (``band_field``):
        (verts, tris, edge_ends, stats).  The mesh holds, complete and bit-identical, every vertex-connected component of the dense
        lattice's mesh that crosses a seed block: all of it when |grad u| <= ``lipschitz`` holds in the blocks that were culled.  With
        a smaller ``lipschitz`` (0 = sign changes of the block corners only) a closed component smaller than a block that no block
        corner sees can be lost."""
        field, stats, _ = self.band_field(sample, axes, threshold, block, lipschitz, max_fraction, net_chunk)
        verts, tris, ends = self.iso_surface(field, threshold)
        return verts, tris, ends, stats

    # ---- connected components, largest-component filter, nearest neighbour (csrc/mesh.hip) ----------------------------
    def _mesh_args(self, tris, n_verts, what):
        """``tris`` as the library reads it (int32 [T, 3], contiguous, on this device) and V, checked: one read-back of the index range."""
        t32 = self._tri_arg(tris, what)
        V, T = int(n_verts), int(t32.shape[0])
        if V < 0 or V >= 1 << 31 or T >= 1 << 31:
            raise _lib.EndoSurfHipError(f"{what}: {V} vertices / {T} triangles do not fit int32 indices")
        if T:
            lo, hi = (int(v) for v in torch.stack([tris.min(), tris.max()]).tolist())
            if lo < 0 or hi >= V:
                raise _lib.EndoSurfHipError(f"{what}: triangle indices {lo}..{hi} outside [0, {V})")
        return t32, V, T

    def _mesh_components(self, t32, V, T, scratch):
        st = self.st()
        changed = self.empty(1, dtype=torch.int32)
        totals = self.empty(3, dtype=torch.int64)
        vlabel, tlabel, counts = (self.empty(n, dtype=torch.int32) for n in (V, T, V))
        check(self.lib.es_mesh_cc_begin(ptr(t32), V, T, ptr(scratch), st), "es_mesh_cc_begin")
        rounds = 0
        while True:          # the fixed point is reached in O(log V) rounds on meshes; V rounds always suffice (each joins two trees)
            check(self.lib.es_mesh_cc_round(ptr(t32), V, T, ptr(scratch), ptr(changed), st), "es_mesh_cc_round")
            rounds += 1
            if not int(changed.item()):
                break
            if rounds > V + 1:
                raise _lib.EndoSurfHipError(f"mesh_components did not reach its fixed point in {rounds} rounds")
        check(self.lib.es_mesh_cc_finish(ptr(t32), V, T, ptr(scratch), ptr(vlabel), ptr(tlabel), ptr(counts), ptr(totals), st),
              "es_mesh_cc_finish")
        ncomp, biggest, degenerate = (int(v) for v in totals.tolist())
        stats = {"components": ncomp, "max_triangles": biggest, "kept_triangles": T - degenerate, "degenerate": degenerate, "rounds": rounds}
        return vlabel, tlabel, counts, stats

    def mesh_components(self, tris: torch.Tensor, n_verts: int):
        """Connected components of a device mesh, by the rule of ``meshing.mesh_components`` (its numpy twin): vertex connectivity,
        degenerate triangles join nothing, label = the smallest vertex index of the component.  (vertex_label [V], triangle_label [T]
        (-1 = degenerate), component_triangles [V], stats), int32 device tensors; ``stats``: components (with a triangle),
        max_triangles, kept_triangles (= the non-degenerate ones here), degenerate, rounds.  The host reads one integer per round."""
        t32, V, T = self._mesh_args(tris, n_verts, "mesh_components")
        return self._mesh_components(t32, V, T, self._scratch("es_mesh_scratch_bytes", V, T))

    def keep_components(self, verts: torch.Tensor, tris: torch.Tensor, keep_ratio: float = 0.9, compact: bool = True):
        """The mesh without the triangles of small components (``meshing.keep_components`` is the numpy twin and the specification):
        a triangle stays iff it is not degenerate and its component has at least ``keep_ratio`` x the triangles of the largest one.
        (verts [V', 3], tris [T', 3] int32, vertex_map [V'] int64, stats); order is kept, ``vertex_map`` is the old index of each new
        vertex (``attr.index_select(0, vertex_map)`` moves per-vertex attributes along).  ``compact=False`` drops triangles only."""
        v32 = self._rows3_arg(verts, "keep_components", "[V, 3] vertices")
        ratio = float(keep_ratio)
        if not 0.0 <= ratio <= 1.0:
            raise _lib.EndoSurfHipError(f"keep_components: keep_ratio must be in [0, 1] (got {keep_ratio!r})")
        t32, V, T = self._mesh_args(tris, v32.shape[0], "keep_components")
        scratch, st = self._scratch("es_mesh_scratch_bytes", V, T), self.st()
        _, tlabel, counts, stats = self._mesh_components(t32, V, T, scratch)
        totals = self.empty(2, dtype=torch.int64)
        check(self.lib.es_mesh_keep_count(ptr(t32), V, T, ptr(tlabel), ptr(counts), ratio, stats["max_triangles"], int(bool(compact)),
                                          ptr(scratch), ptr(totals), st), "es_mesh_keep_count")
        V2, T2 = (int(v) for v in totals.tolist())
        verts_out, tris_out, vmap = self.empty(V2, 3), self.empty(T2, 3, dtype=torch.int32), self.empty(V2, dtype=torch.int64)
        check(self.lib.es_mesh_keep_emit(ptr(v32), ptr(t32), V, T, ptr(scratch), V2, T2, ptr(verts_out), ptr(tris_out), ptr(vmap), st),
              "es_mesh_keep_emit")
        stats["kept_triangles"] = T2
        return verts_out, tris_out, vmap, stats

    def nearest(self, query: torch.Tensor, points: torch.Tensor):
        """Exact nearest neighbour of each ``query`` row among the rows of ``points`` ([Q, 3], [P, 3] on this device): (dist [Q] fp32,
        index [Q] int32) by the rule of ``meshing.nearest`` (the numpy twin): fp32 squared distance, ties to the smallest index,
        non-finite rows never an answer, inf / -1 where there is none; bit-identical from call to call.  No read-back."""
        q, p = self._rows3_arg(query, "nearest", "[N, 3] query"), self._rows3_arg(points, "nearest", "[N, 3] points")
        Q, P = int(q.shape[0]), int(p.shape[0])
        scratch, st = self._scratch("es_nn_scratch_bytes", P), self.st()
        dist, index = self.empty(Q), self.empty(Q, dtype=torch.int32)
        check(self.lib.es_nn_build(ptr(p), P, ptr(scratch), st), "es_nn_build")
        check(self.lib.es_nn_query(ptr(q), Q, P, ptr(scratch), ptr(dist), ptr(index), st), "es_nn_query")
        return dist, index

    # ---- point-to-surface distance (csrc/surface.hip; contract: DESIGN.md 7f) ------------------------------------------------
    def point_to_mesh(self, points: torch.Tensor, vertices: torch.Tensor, triangles: torch.Tensor, return_work: bool = False):
        """Exact distance from each row of ``points`` [Q, 3] to the triangle mesh ``vertices`` [V, 3] / ``triangles`` [T, 3] (int32 or
        int64), all on this device: (dist [Q] fp32, triangle [Q] int32, closest [Q, 3] fp32) by the rule of ``meshing.point_to_mesh``
        (the numpy twin and the specification), evaluated in fp64.  A triangle with a repeated or out-of-range index or a non-finite
        corner is skipped, not an error; inf / -1 / nan where there is no answer (a non-finite query row, no triangle that takes
        part).  Bit-identical from call to call; no read-back.  ``return_work=True`` appends work [Q, 2] int32: the cell shells a
        query read and the triangles it measured."""
        q = self._rows3_arg(points, "point_to_mesh", "[N, 3] points")
        v = self._rows3_arg(vertices, "point_to_mesh", "[N, 3] vertices")
        if not torch.is_tensor(triangles) or triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.device != self.device \
                or triangles.dtype not in (torch.int32, torch.int64):
            raise _lib.EndoSurfHipError(f"point_to_mesh takes [T, 3] int32 / int64 triangles on {self.device}")
        Q, V, T = int(q.shape[0]), int(v.shape[0]), int(triangles.shape[0])
        t = triangles.detach()
        if t.dtype == torch.int64:          # an index beyond int32 must stay out of range, not wrap into it
            t = torch.where((t < 0) | (t >= V), torch.full_like(t, -1), t)
        t32 = t.to(torch.int32).contiguous()
        scratch, st = self._scratch("es_surf_scratch_bytes", V, T), self.st()
        dist, tri, closest = self.empty(Q), self.empty(Q, dtype=torch.int32), self.empty(Q, 3)
        work = self.empty(Q, 2, dtype=torch.int32) if return_work else None
        check(self.lib.es_surf_build(ptr(v), ptr(t32), V, T, ptr(scratch), st), "es_surf_build")
        check(self.lib.es_surf_query(ptr(q), Q, ptr(v), ptr(t32), V, T, ptr(scratch), ptr(dist), ptr(tri), ptr(closest), ptr(work), st),
              "es_surf_query")
        return (dist, tri, closest, work) if return_work else (dist, tri, closest)

    # ---- mesh export: clean-up, normals, clustering, PLY body (csrc/mesh.hip, csrc/export.hip; contract: DESIGN.md 7e) ------
    def _mesh_clean(self, v32, t32, V, T, compact):
        """``mesh_clean`` of checked arguments.  The two stable sorts order the triangles by (sorted corners, triangle index)."""
        st, scratch = self.st(), self._scratch("es_mesh_scratch_bytes", V, T)
        key_hi, key_lo = self.empty(T, dtype=torch.int32), self.empty(T, dtype=torch.int64)
        check(self.lib.es_mesh_clean_keys(ptr(t32), V, T, ptr(key_hi), ptr(key_lo), st), "es_mesh_clean_keys")
        by_lo = torch.sort(key_lo, stable=True).indices
        order = by_lo[torch.sort(key_hi[by_lo], stable=True).indices].contiguous()
        totals = self.empty(3, dtype=torch.int64)
        check(self.lib.es_mesh_clean_count(ptr(t32), V, T, ptr(order), int(bool(compact)), ptr(scratch), ptr(totals), st), "es_mesh_clean_count")
        V2, T2, degenerate = (int(v) for v in totals.tolist())
        verts_out, tris_out, vmap = self.empty(V2, 3), self.empty(T2, 3, dtype=torch.int32), self.empty(V2, dtype=torch.int64)
        check(self.lib.es_mesh_keep_emit(ptr(v32), ptr(t32), V, T, ptr(scratch), V2, T2, ptr(verts_out), ptr(tris_out), ptr(vmap), st),
              "es_mesh_keep_emit")
        return verts_out, tris_out, vmap, {"degenerate": degenerate, "duplicates": T - degenerate - T2, "kept_triangles": T2}

    def mesh_clean(self, vertices: torch.Tensor, triangles: torch.Tensor, compact: bool = False):
        """The mesh without its degenerate and duplicate triangles (``meshing.mesh_clean`` is the numpy twin and the specification; what
        Open3D's remove_degenerate_triangles + remove_duplicated_triangles do): a triangle with a repeated index goes, and of the
        triangles with the same three vertex indices, in any rotation or orientation, the one with the smallest triangle index stays.
        Survivors keep their order and their own orientation.  (verts [V', 3], tris [T', 3] int32, vertex_map [V'] int64, stats):
        ``compact=True`` also drops the vertices no surviving triangle uses and renumbers, ``vertex_map`` being the old index of each
        new vertex as in ``keep_components``; ``stats``: degenerate, duplicates, kept_triangles.  One read-back (three counts)."""
        v32 = self._rows3_arg(vertices, "mesh_clean", "[V, 3] vertices")
        t32, V, T = self._mesh_args(triangles, v32.shape[0], "mesh_clean")
        return self._mesh_clean(v32, t32, V, T, compact)

    def vertex_normals(self, vertices: torch.Tensor, triangles: torch.Tensor):
        """Area-weighted vertex normals [V, 3] fp32 of a device mesh, bit for bit those of ``meshing.vertex_normals`` (the numpy twin
        and the specification) for fp32 vertices: per vertex the fp64 sum of the un-normalised fp64 face cross products of its
        triangles, added in the twin's order (corner 0 of every triangle in triangle order, then corner 1, then corner 2), normalised;
        0 for a vertex of no triangle with an area.  No float atomics, no read-back."""
        v32 = self._rows3_arg(vertices, "vertex_normals", "[V, 3] vertices")
        t32, V, T = self._mesh_args(triangles, v32.shape[0], "vertex_normals")
        st, scratch = self.st(), self._scratch("es_vn_scratch_bytes", V)
        corner_vertex, normals = self.empty(3 * T, dtype=torch.int32), self.empty(V, 3)
        check(self.lib.es_vn_count(ptr(t32), V, T, ptr(corner_vertex), ptr(scratch), st), "es_vn_count")
        order = torch.sort(corner_vertex, stable=True).indices
        check(self.lib.es_vn_gather(ptr(v32), ptr(t32), V, T, ptr(order), ptr(scratch), ptr(normals), st), "es_vn_gather")
        return normals

    def cluster_vertices(self, vertices: torch.Tensor, triangles: torch.Tensor, cell: float, origin=(0.0, 0.0, 0.0), attributes=None):
        """Vertex clustering (``meshing.cluster_vertices`` is the numpy twin and the specification; the averaging variant of Open3D's
        simplify_vertex_clustering): the vertices of one cell floor((float64(v) - origin) / cell) become one vertex, their fp64 mean in
        ascending index rounded to fp32, numbered by ascending (ix, iy, iz); ``attributes`` [V, C <= 8] are averaged likewise; the
        triangles are renumbered and cleaned (``mesh_clean``: collapsed and duplicate triangles go, order kept).  Cell coordinates must
        lie in [-2^20, 2^20).  Returns (verts [V', 3], tris [T', 3] int32, attributes [V', C] or None, vertex_cluster [V] int32,
        stats: cells, largest_cell, degenerate, duplicates, kept_triangles).  Two read-backs (the cell counts, the clean-up's)."""
        from .meshing import RAST_MAX_ATTRS
        v32 = self._rows3_arg(vertices, "cluster_vertices", "[V, 3] vertices")
        t32, V, T = self._mesh_args(triangles, v32.shape[0], "cluster_vertices")
        org = [float(o) for o in origin]
        if len(org) != 3:
            raise _lib.EndoSurfHipError(f"cluster_vertices: origin must have three entries (got {origin!r})")
        att, Cn = None, 0
        if attributes is not None:
            if attributes.dim() != 2 or attributes.shape[0] != V or not 1 <= attributes.shape[1] <= RAST_MAX_ATTRS or attributes.device != self.device:
                raise _lib.EndoSurfHipError(f"cluster_vertices takes [V, 1..{RAST_MAX_ATTRS}] attributes on {self.device} (got {tuple(attributes.shape)})")
            att, Cn = f32(attributes), int(attributes.shape[1])
        st, scratch = self.st(), self._scratch("es_cluster_scratch_bytes", V)
        key = self.empty(V, dtype=torch.int64)
        check(self.lib.es_cluster_keys(ptr(v32), V, float(cell), *org, ptr(key), st), "es_cluster_keys")
        sorted_key, order = torch.sort(key, stable=True)
        totals = self.empty(3, dtype=torch.int64)
        check(self.lib.es_cluster_count(ptr(sorted_key), V, ptr(scratch), ptr(totals), st), "es_cluster_count")
        cells, bad, largest = (int(v) for v in totals.tolist())
        verts_out, cluster = self.empty(cells, 3), self.empty(V, dtype=torch.int32)
        att_out = self.empty(cells, Cn) if Cn else None
        check(self.lib.es_cluster_emit(ptr(v32), ptr(att), Cn, V, ptr(order), ptr(scratch), cells, bad, ptr(verts_out), ptr(att_out), ptr(cluster), st),
              "es_cluster_emit")
        remapped = self.empty(T, 3, dtype=torch.int32)
        check(self.lib.es_cluster_remap(ptr(t32), V, T, ptr(cluster), ptr(remapped), st), "es_cluster_remap")
        _, tris_out, _, cstats = self._mesh_clean(verts_out, remapped, cells, T, False)
        return verts_out, tris_out, att_out, cluster, dict(cells=cells, largest_cell=largest, **cstats)

    def ply_pack(self, vertices: torch.Tensor, triangles=None, colors=None, normals=None):
        """The body of a ``binary_little_endian 1.0`` PLY file as a uint8 device tensor (``data.ply_body`` is the numpy twin, and
        ``data.ply_header`` the text in front of it): per vertex ``float x y z``, then ``float nx ny nz`` with ``normals`` [V, 3], then
        ``uchar red green blue`` with ``colors`` [V, 3] -- floats quantised by the rule of ``data.to8b``, trunc(255 clip(c, 0, 1)) in
        fp32: below 0 gives 0, above 1 gives 255, NaN 0 --; then per triangle ``uchar 3`` and three ``int`` indices (13 bytes).
        ``triangles=None`` packs a point cloud.  No read-back."""
        v32 = self._rows3_arg(vertices, "ply_pack", "[V, 3] vertices")
        V = int(v32.shape[0])
        t32 = None if triangles is None else self._tri_arg(triangles, "ply_pack")
        T = 0 if t32 is None else int(t32.shape[0])
        rows = {}
        for name, a in (("normals", normals), ("colors", colors)):
            rows[name] = None
            if a is not None:
                rows[name] = self._rows3_arg(a, "ply_pack", f"[V, 3] {name}")
                if rows[name].shape[0] != V:
                    raise _lib.EndoSurfHipError(f"ply_pack: {name} has {rows[name].shape[0]} rows for {V} vertices")
        out = self.empty(self._scratch_bytes("es_ply_body_bytes", V, T, int(normals is not None), int(colors is not None)), dtype=torch.uint8)
        check(self.lib.es_ply_pack(ptr(v32), ptr(rows["normals"]), ptr(rows["colors"]), ptr(t32), V, T, ptr(out), self.st()), "es_ply_pack")
        return out

    # ---- mesh rasteriser (csrc/raster.hip) ------------------------------------------------------------------------------
    def project_vertices(self, vertices: torch.Tensor, intrinsics, pose):
        """Stage A of the rasteriser (``meshing.project_vertices`` is the numpy twin and the specification): world vertices [V, 3]
        through the pinhole camera ``intrinsics`` ([3,3] or [4,4]) at the camera-to-world ``pose`` [4,4] of ``data.get_rays``, in fp64:
        (xy [V, 2] int32 in 1/256-pixel fixed point, zc [V] fp32 camera depth, NaN for a non-finite vertex), on the device."""
        from .meshing import camera_params
        v32 = self._rows3_arg(vertices, "project_vertices", "[V, 3] vertices")
        cam = (C.c_double * 17)(*camera_params(intrinsics, pose).tolist())
        V = int(v32.shape[0])
        xy, zc = self.empty(V, 2, dtype=torch.int32), self.empty(V)
        check(self.lib.es_rast_project(ptr(v32), V, cam, ptr(xy), ptr(zc), self.st()), "es_rast_project")
        return xy, zc

    def rasterize_projected(self, xy: torch.Tensor, zc: torch.Tensor, triangles: torch.Tensor, height: int, width: int, attributes=None,
                            near: float = 1e-6, cull: str = "none"):
        """Stage B of the rasteriser on the output of ``project_vertices`` (``meshing.rasterize_projected`` is the numpy twin and the
        specification): the dict of ``rasterize``.  The host reads the number of work items back between counting and filling, and
        the counts of ``stats`` at the end."""
        from .meshing import RAST_CULL, RAST_MAX_ATTRS, RAST_MAX_SIZE, RAST_REASONS
        H, W = int(height), int(width)
        if not (1 <= H <= RAST_MAX_SIZE and 1 <= W <= RAST_MAX_SIZE):
            raise _lib.EndoSurfHipError(f"rasterize: height and width must be in 1..{RAST_MAX_SIZE} (got {height!r}, {width!r})")
        if cull not in RAST_CULL:
            raise _lib.EndoSurfHipError(f"rasterize: cull must be one of {sorted(RAST_CULL)} (got {cull!r})")
        if xy.dim() != 2 or xy.shape[1] != 2 or xy.dtype != torch.int32 or zc.dim() != 1 or zc.shape[0] != xy.shape[0] \
                or xy.device != self.device or zc.device != self.device:
            raise _lib.EndoSurfHipError(f"rasterize takes xy [V, 2] int32 and zc [V] on {self.device}")
        t32 = self._tri_arg(triangles, "rasterize")
        V, T = int(zc.shape[0]), int(t32.shape[0])
        att, Cn = None, 0
        if attributes is not None:
            if attributes.dim() != 2 or attributes.shape[0] != V or not 1 <= attributes.shape[1] <= RAST_MAX_ATTRS or attributes.device != self.device:
                raise _lib.EndoSurfHipError(f"rasterize takes [V, 1..{RAST_MAX_ATTRS}] attributes on {self.device} (got {tuple(attributes.shape)})")
            att, Cn = f32(attributes), int(attributes.shape[1])
        out = {"depth": None, "triangle": None, "bary": None, "attributes": None,
               "stats": dict({name: 0 for name in RAST_REASONS}, triangles=T, work_items=0, covered_pixels=0)}
        if V == 0 or T == 0:          # nothing to draw: no launch
            out.update(depth=torch.full((H, W), float("inf"), device=self.device), triangle=torch.full((H, W), -1, dtype=torch.int32, device=self.device),
                       bary=torch.zeros(H, W, 3, device=self.device), attributes=torch.zeros(H, W, Cn, device=self.device))
            out["stats"]["invalid"] = T
            return out
        xy32, zc32 = xy.contiguous(), f32(zc)
        scratch, totals, st = self._scratch("es_rast_scratch_bytes", V, T, H, W), self.empty(8, dtype=torch.int64), self.st()
        view = (H, W, float(near), RAST_CULL[cull], ptr(scratch))
        check(self.lib.es_rast_count(ptr(t32), V, T, ptr(xy32), ptr(zc32), *view, ptr(totals), st), "es_rast_count")
        n_work = int(totals[0].item())
        check(self.lib.es_rast_fill(ptr(t32), V, T, ptr(xy32), ptr(zc32), *view, n_work, st), "es_rast_fill")
        depth, tri, bary = self.empty(H, W), self.empty(H, W, dtype=torch.int32), self.empty(H, W, 3)
        attr = self.empty(H, W, Cn)
        check(self.lib.es_rast_resolve(ptr(t32), V, T, ptr(xy32), ptr(zc32), ptr(att), Cn, *view[:4], ptr(scratch), ptr(depth), ptr(tri), ptr(bary),
                                       ptr(attr) if Cn else None, ptr(totals), st), "es_rast_resolve")
        tt = totals.tolist()
        out["stats"].update({name: int(tt[1 + i]) for i, name in enumerate(RAST_REASONS)}, work_items=int(tt[0]), covered_pixels=int(tt[6]))
        out.update(depth=depth, triangle=tri, bary=bary, attributes=attr)
        return out

    def rasterize(self, vertices: torch.Tensor, triangles: torch.Tensor, intrinsics, pose, height: int, width: int, attributes=None,
                  near: float = 1e-6, cull: str = "none"):
        """A device mesh as images of a pinhole camera, without a display: ``depth`` [H, W] fp32 (camera z, the convention of
        ``data.depth_points``; +inf where nothing is hit), ``triangle`` [H, W] int32 (-1), ``bary`` [H, W, 3] (perspective-correct
        weights of the triangle's corners; 0), ``attributes`` [H, W, C] (the per-vertex ``attributes`` [V, C <= 8] interpolated with
        them; 0) and ``stats`` (triangles, rejected ones by reason -- invalid, near_rejected, zero_area, culled, offscreen --,
        work_items, covered_pixels).  Pixel (row i, column j) is sampled where ``data.get_rays`` casts its ray; one sample per pixel.
        A triangle with a corner not farther than ``near`` along the camera axis is dropped whole (no clipping); ``cull`` = "none",
        "back" or "front" (the front is the side the normal (v1 - v0) x (v2 - v0) points to: the outside of ``iso_surface``'s meshes).
        ``meshing.rasterize`` is the numpy twin; the rules of coverage and depth are in ``meshing.rasterize_projected``.  Equal depths
        go to the smaller triangle index, so the images are bit-identical from call to call."""
        xy, zc = self.project_vertices(vertices, intrinsics, pose)
        return self.rasterize_projected(xy, zc, triangles, height, width, attributes, near, cull)

    # ---- frame evaluation (csrc/metrics.hip) ---------------------------------------------------------------------------
    def _eval_stack(self, name, t, channels=None, like=None):
        """``t`` as the evaluation kernels read it: an fp32 [n,H,W,C] stack on this device, contiguous (a strided view is copied, never
        read through its strides).  Raises for another dtype, device or shape; launches nothing."""
        if not torch.is_tensor(t) or t.device != self.device or t.dtype != torch.float32:
            raise _lib.EndoSurfHipError(f"{name} must be an fp32 tensor on {self.device} (got "
                                        f"{(t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__})")
        if t.dim() == 3 and channels in (None, 1):
            t = t.unsqueeze(-1)
        if t.dim() != 4 or (channels is not None and t.shape[-1] != channels) or (like is not None and t.shape != like.shape):
            want = tuple(like.shape) if like is not None else f"[n, H, W, {channels or 'C'}]"
            raise _lib.EndoSurfHipError(f"{name} must be {want} (got {tuple(t.shape)})")
        return t.detach().contiguous()

    def _eval_mask(self, mask, like):
        """A per-pixel mask [n,H,W] or [n,H,W,1] of the stack ``like`` as a contiguous fp32 [n,H,W]; None stays None (= ones)."""
        if mask is None:
            return None
        if not torch.is_tensor(mask) or mask.device != self.device or mask.dtype != torch.float32:
            raise _lib.EndoSurfHipError(f"mask must be an fp32 tensor on {self.device} or None")
        if mask.dim() == 4 and mask.shape[-1] == 1:
            mask = mask[..., 0]
        if mask.shape != like.shape[:3]:
            raise _lib.EndoSurfHipError(f"mask must be [n, H, W] or [n, H, W, 1] of the images (got {tuple(mask.shape)} for {tuple(like.shape)})")
        return mask.detach().contiguous()

    def _eval_out(self, out, numel):
        if out is None:
            return self.empty(numel, dtype=torch.float64)
        if out.dtype != torch.float64 or out.device != self.device or out.dim() != 1 or out.numel() != numel or not out.is_contiguous():
            raise _lib.EndoSurfHipError(f"out must be a contiguous fp64 [{numel}] on {self.device}")
        return out

    def _eval_scratch(self, scratch, fn_name, *dims):
        nbytes = self._scratch_bytes(fn_name, *dims)
        if scratch is None:
            return self.empty(max(nbytes, 8), dtype=torch.uint8)
        if scratch.device != self.device or not scratch.is_contiguous() or scratch.numel() * scratch.element_size() < nbytes:
            raise _lib.EndoSurfHipError(f"scratch must be a contiguous buffer of at least {nbytes} bytes on {self.device}")
        return scratch

    def ssim(self, a, b, mask=None, data_range: float = 1.0, full: bool = False, out=None, scratch=None):
        """The reference's ``cal_ssim`` of two fp32 stacks [n,H,W,C] (C <= 4) on this device (``imaging.ssim`` is the numpy twin and the
        specification): both times the per-pixel ``mask``, "valid" 11 x 11 window from the reference's 121-entry fp32 table, moments
        and map in fp64, ``data_range`` = L.  Returns dict(``mean`` [] fp64, ``per_frame`` [n] fp64, and with ``full`` ``map``
        [n,H-10,W-10,C] fp64), all on the device (no read-back); ``mean`` and ``per_frame`` are views of ``out`` [n+1] when one is given.
        Bit-identical from call to call, whatever ``scratch`` holds."""
        from .imaging import SSIM_MAX_CHANNELS, SSIM_WINDOW, ssim_window
        a = self._eval_stack("a", a)
        b = self._eval_stack("b", b, like=a)
        m = self._eval_mask(mask, a)
        n, H, W, Cn = (int(v) for v in a.shape)
        if H < SSIM_WINDOW or W < SSIM_WINDOW or not 1 <= Cn <= SSIM_MAX_CHANNELS:
            raise _lib.EndoSurfHipError(f"ssim needs images of at least {SSIM_WINDOW} x {SSIM_WINDOW} pixels and 1..{SSIM_MAX_CHANNELS} channels "
                                        f"(got {H} x {W} x {Cn})")
        if not (float(data_range) > 0.0 and float(data_range) < float("inf")):
            raise _lib.EndoSurfHipError(f"ssim: data_range must be finite and positive (got {data_range!r})")
        if getattr(self, "_ssim_window", None) is None:
            self._ssim_window = torch.from_numpy(ssim_window()).to(self.device).contiguous()
        out = self._eval_out(out, n + 1)
        scratch = self._eval_scratch(scratch, "es_ssim_scratch_bytes", n, H, W)
        smap = self.empty(n, H - SSIM_WINDOW + 1, W - SSIM_WINDOW + 1, Cn, dtype=torch.float64) if full else None
        check(self.lib.es_ssim(ptr(a), ptr(b), ptr(m), ptr(self._ssim_window), n, H, W, Cn, float(data_range), ptr(scratch), ptr(out), ptr(smap),
                               self.st()), "es_ssim")
        if n == 0:
            out.fill_(float("nan"))
        res = {"mean": out[n], "per_frame": out[:n]}
        if full:
            res["map"] = smap
        return res

    def masked_sq_sums(self, a, b, mask=None, out=None, scratch=None):
        """Per frame of two fp32 stacks [n,H,W,C] on this device, in fp64: S = sum (a - b)^2 m, M = sum m (the per-pixel ``mask`` once
        per pixel) -- everything ``cal_psnr`` / ``cal_rmse`` need (``imaging.masked_sq_sums`` is the twin).  Returns dict(``S`` [n],
        ``M`` [n], ``S_total`` [], ``M_total`` []) of device fp64, views of ``out`` [2n+2] when one is given.  No read-back."""
        a = self._eval_stack("a", a)
        b = self._eval_stack("b", b, like=a)
        m = self._eval_mask(mask, a)
        n, H, W, Cn = (int(v) for v in a.shape)
        if H < 1 or W < 1 or not 1 <= Cn <= 16:
            raise _lib.EndoSurfHipError(f"masked_sq_sums needs non-empty images of 1..16 channels (got {H} x {W} x {Cn})")
        out = self._eval_out(out, 2 * n + 2)
        scratch = self._eval_scratch(scratch, "es_sq_sums_scratch_bytes", n, H, W)
        check(self.lib.es_masked_sq_sums(ptr(a), ptr(b), ptr(m), n, H, W, Cn, ptr(scratch), ptr(out), self.st()), "es_masked_sq_sums")
        if n == 0:
            out.zero_()
        return {"S": out[:n], "M": out[n:2 * n], "S_total": out[2 * n], "M_total": out[2 * n + 1]}

    def _panel_target(self, x, out, col):
        """(picture, pitch in bytes, column) a panel of the stack ``x`` [n,H,W,*] is written to: a fresh [n,H,W,3] or the caller's
        contiguous uint8 picture [n,H,W_total,3] from column ``col`` on."""
        n, H, W = (int(v) for v in x.shape[:3])
        if out is None:
            return self.empty(n, H, W, 3, dtype=torch.uint8), 3 * W, 0
        if out.dtype != torch.uint8 or out.device != self.device or out.dim() != 4 or not out.is_contiguous() or out.shape[0] != n \
                or out.shape[1] != H or out.shape[3] != 3 or int(col) < 0 or int(col) + W > out.shape[2]:
            raise _lib.EndoSurfHipError(f"a panel of {n} x {H} x {W} at column {col} needs a contiguous uint8 [{n}, {H}, >= {int(col) + W}, 3] "
                                        f"picture on {self.device}")
        return out, 3 * int(out.shape[2]), int(col)

    def panel_rgb(self, x, out=None, col: int = 0):
        """``gen_rgb``'s picture of an fp32 stack [n,H,W,3] (or grey [n,H,W] / [n,H,W,1]): uint8(clip(256 x, 0, 255)), as a new
        [n,H,W,3] or into the columns ``col``.. of the picture ``out`` [n,H,W_total,3] (returned).  Twin: ``imaging.panel_rgb``."""
        x = self._eval_stack("an rgb panel's image", x)
        if x.shape[-1] not in (1, 3):
            raise _lib.EndoSurfHipError(f"an rgb panel takes 1 or 3 channels (got {x.shape[-1]})")
        pic, pitch, col = self._panel_target(x, out, col)
        n, H, W, Cn = (int(v) for v in x.shape)
        check(self.lib.es_eval_panel_rgb(ptr(x), n, H, W, Cn, ptr(pic), pitch, col, self.st()), "es_eval_panel_rgb")
        return pic

    def panel_depth(self, d, depth_max=None, out=None, col: int = 0):
        """``gen_depth``'s picture of an fp32 depth stack [n,H,W,1] (or [n,H,W]): uint8(255 - clip(d / depth_max, 0, 1) 255) on three
        channels; ``depth_max=None``: the largest value of the stack (one reduction and read-back).  Twin: ``imaging.panel_depth``."""
        d = self._eval_stack("a depth panel's image", d, channels=1)
        if depth_max is None:
            depth_max = float(d.max()) if d.numel() else 1.0
        if not (float(depth_max) > 0.0 and float(depth_max) < float("inf")):
            raise _lib.EndoSurfHipError(f"panel_depth: depth_max must be finite and positive (got {depth_max!r})")
        pic, pitch, col = self._panel_target(d, out, col)
        n, H, W, _ = (int(v) for v in d.shape)
        check(self.lib.es_eval_panel_depth(ptr(d), n, H, W, float(depth_max), ptr(pic), pitch, col, self.st()), "es_eval_panel_depth")
        return pic

    def panel_normal(self, normals, poses, revert: bool = False, out=None, col: int = 0):
        """``gen_normal`` of an fp32 stack of world normals [n,H,W,3] and the camera-to-world ``poses`` [n,4,4] of its frames:
        n / (|n| + 1e-10) turned into each camera's frame by inv(pose[:3,:3]) (inverted in fp32 on the host: 9 floats per frame go to
        the kernel), negated with ``revert``.  Returns (the float picture [n,H,W,3] fp32, uint8(clip(128 n + 128, 0, 255)) as in
        ``panel_rgb``).  Twin: ``imaging.panel_normal``."""
        from .imaging import normal_rotations
        x = self._eval_stack("a normal panel's image", normals, channels=3)
        n, H, W, _ = (int(v) for v in x.shape)
        p = poses.detach().cpu().numpy() if torch.is_tensor(poses) else poses
        rot = normal_rotations(p)
        if rot.shape != (n, 3, 3):
            raise _lib.EndoSurfHipError(f"panel_normal needs one [4,4] pose per frame (got {rot.shape[0]} for {n} frames)")
        rot_d = torch.from_numpy(rot.reshape(n, 9).copy()).to(self.device)
        pic, pitch, col = self._panel_target(x, out, col)
        out_f = self.empty(n, H, W, 3)
        check(self.lib.es_eval_panel_normal(ptr(x), ptr(rot_d), n, H, W, int(bool(revert)), ptr(out_f), ptr(pic), pitch, col, self.st()),
              "es_eval_panel_normal")
        return out_f, pic

    def eval_panels(self, color_gt, color, depth_gt, depth, normal, poses, depth_max=None, revert: bool = False):
        """The five panels of the reference's eval picture (``imaging.PANELS``: rgb_gt, rgb_pred, depth_gt, depth_pred, normal_pred),
        each written by its kernel straight into its columns of one ``sheet`` [n,H,5W,3] uint8 (no concatenation).  Returns
        dict(``sheet``, ``panels`` = {name: the [n,H,W,3] view of its columns}, ``normal`` = the float camera-frame normals)."""
        from .imaging import PANELS
        color = self._eval_stack("color", color, channels=3)
        n, H, W, _ = (int(v) for v in color.shape)
        sheet = self.empty(n, H, len(PANELS) * W, 3, dtype=torch.uint8)
        stacks = {"rgb_gt": self._eval_stack("color_gt", color_gt, like=color), "rgb_pred": color,
                  "depth_gt": self._eval_stack("depth_gt", depth_gt, channels=1), "depth_pred": self._eval_stack("depth", depth, channels=1),
                  "normal_pred": self._eval_stack("normal", normal, like=color)}
        for k in ("depth_gt", "depth_pred"):
            if stacks[k].shape[:3] != color.shape[:3]:
                raise _lib.EndoSurfHipError(f"{k} must be [{n}, {H}, {W}, 1] (got {tuple(stacks[k].shape)})")
        normal_f = None
        for i, name in enumerate(PANELS):
            if name.startswith("rgb"):
                self.panel_rgb(stacks[name], out=sheet, col=i * W)
            elif name.startswith("depth"):
                self.panel_depth(stacks[name], depth_max, out=sheet, col=i * W)
            else:
                normal_f, _ = self.panel_normal(stacks[name], poses, revert, out=sheet, col=i * W)
        return {"sheet": sheet, "panels": {name: sheet[:, :, i * W:(i + 1) * W] for i, name in enumerate(PANELS)}, "normal": normal_f}

    # ---- per-kernel timers (csrc/timing.hip) ---------------------------------------------------------
    def timing_enable(self, on: bool):
        self._timing_on = bool(on)          # (events cannot be recorded inside a captured graph: the renderer's captured forward stands down)
        check(self.lib.es_timing_enable(int(on)), "es_timing_enable")

    def timing_drain(self):
        """[(kernel name, rows, ms)] of every launch recorded since the last drain."""
        cap = 65536
        kid = (C.c_int * cap)()
        rows = (C.c_longlong * cap)()
        ms = (C.c_float * cap)()
        n = C.c_int()
        check(self.lib.es_timing_drain(cap, kid, rows, ms, C.byref(n)), "es_timing_drain")
        return [(self.lib.es_kernel_name(kid[i]).decode(), int(rows[i]), float(ms[i])) for i in range(n.value)]


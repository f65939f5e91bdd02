"""The tail of a live render: room behind a grad-enabled render's samples in which the colour-less point evaluations of the calls that
follow it (``errorondepth``, ``surface_neighbour_error``) ride, so that ONE backward chain serves all three calls.

``_Tail`` owns the rows and every change of their state: the renderer and ``functions._RenderFn`` only ask (``peek`` / ``claim`` /
``open`` / ``evaluate`` / ``finish`` / ``close``).  WHEN a render hosts a tail, how large it is and who may use it is the renderer's policy
(``EndoSurfRenderer._new_tail``, ``_aux_demand``, ``_live_tail``).  ``_TailEvalFn`` and ``_LazyEodFn`` are the autograd nodes of the
evaluations placed here, ``_PendingEod`` / ``_Lazy`` the deferred form of ``errorondepth``'s.

Writing points in place: a caller may ``peek`` a slot, have its points kernel write straight into ``slot.x`` / ``slot.t`` and hand those
views on to ``EndoSurfRenderer._point_eval``, which peeks the same slot again, recognises the views by their address and skips the copy.
Nothing is reserved by a peek: the rows belong to whoever ``claim``s them next.
"""
from __future__ import annotations

import collections
import weakref
from typing import Optional

import torch

from .engine import Engine, f32


# where the next ``m`` points of a tail go: the row offset behind the render's samples and the views [m,3] / [m] to write them to
_Slot = collections.namedtuple("_Slot", "off x t")


class _Tail:
    """Room behind a grad-enabled render's samples for the colour-less points of the calls that FOLLOW it in the reference trainer's step
    (``renderer(rays)`` -> ``errorondepth`` -> ``surface_neighbour_error``, trainer_endosurf.py:130, :140, :155).  The render lays its point
    workspace out for P + cap rows and evaluates the first P; each later grad-enabled point evaluation writes its points into the next free
    rows of (aux_x, aux_t), evaluates exactly those rows (es_point_forward_rows) and deposits its adjoints in (g_sdf, g_go) when autograd
    reaches it; the render's backward -- which autograd runs after them, see ``_TailEvalFn`` -- then back-propagates the whole workspace in
    ONE chain of launches with the tail's stages mixed into the main ones, exactly as the fused training step does.  The three separate
    backward chains this replaces cost 2.1 ms of a 19.6 ms step (two of them run 16 - 32 workgroups at a tile's full latency per launch).

    ``cap`` is learnt: the rows the previous step asked for (EndoSurfRenderer._aux_demand); rows nobody claimed are evaluated (at whatever
    finite points the buffer holds, with zero adjoints) before the backward, so every row of the workspace is defined."""

    def __init__(self, eng: Engine, P_: int, cap: int):
        self.P, self.cap, self.used = int(P_), int(cap), 0
        buf = eng.zeros(8 * cap)                      # one allocation, one fill: points (x | t) and adjoints (g_sdf | g_go)
        self.aux_x, self.aux_t = buf[:3 * cap].view(cap, 3), buf[3 * cap:4 * cap]
        self.g_sdf, self.g_go = buf[4 * cap:5 * cap].view(cap, 1), buf[5 * cap:].view(cap, 3)
        self.gbuf = buf[4 * cap:]                     # both adjoint buffers: cleared again behind every backward that consumed them
        self.pctx, self.weff, self.flags = None, None, 0
        self.pending = None                           # a deferred errorondepth evaluation placed in these rows (_PendingEod)

    @staticmethod
    def rows64(m: int) -> int:
        """Rows ``m`` points take: evaluations come in tiles of 64 rows."""
        return (int(m) + 63) // 64 * 64

    def peek(self, m: int, weff, flags: int) -> Optional[_Slot]:
        """The slot the next ``m`` points would get, or None: no open workspace, other weights or flags than the render's, no room."""
        if self.pctx is None or self.weff is not weff or self.flags != flags or self.used + self.rows64(m) > self.cap:
            return None
        off = self.used
        return _Slot(off, self.aux_x[off:off + m], self.aux_t[off:off + m])

    def claim(self, m: int) -> int:
        """Take the next ``rows64(m)`` rows; -> their offset (what ``peek`` announced)."""
        off = self.used
        self.used = off + self.rows64(m)
        return off

    def open(self, pctx, weff, flags: int):
        """The render has evaluated its own rows of ``pctx``, a workspace laid out for P + cap rows: the tail's rows can be claimed."""
        self.pctx, self.weff, self.flags = pctx, weff, flags

    def defer(self, pending: "_PendingEod"):
        """``pending``'s rows are claimed but not evaluated: the next ``evaluate`` folds them into its launch, anything else forces them."""
        self.pending = pending

    def issued(self, pending: "_PendingEod"):
        if self.pending is pending:
            self.pending = None

    def force_pending(self):
        if self.pending is not None:
            self.pending.force()

    def evaluate(self, eng: Engine, off: int, m: int, weff, packed):
        """Evaluate the claimed rows [off, off + rows64(m)) (es_point_forward_rows)."""
        m64 = self.rows64(m)
        pend = self.pending
        if pend is not None and not pend.done and not pend.rows_done and pend.off + pend.m64 == off and pend.stream == torch.cuda.current_stream(eng.device):
            # errorondepth's deferred rows sit right in front of these: ONE launch chain evaluates both pieces
            eng.point_forward_rows(self.pctx, weff, packed, self.P + pend.off, pend.m64 + m64)
            pend.rows_done = True
            pend.force()
        else:
            self.force_pending()
            eng.point_forward_rows(self.pctx, weff, packed, self.P + off, m64)

    def finish(self, eng: Engine, weff, packed):
        """Before the render's backward: every row of the workspace defined.  The later calls' nodes have run (they depend on the render's
        through the token) and left their adjoints in (g_sdf, g_go); rows nobody claimed are evaluated now, with zero adjoints."""
        self.force_pending()          # (a deferred errorondepth nobody has read: its rows must be defined before the backward)
        if self.pctx is not None and self.used < self.cap:
            eng.point_forward_rows(self.pctx, weff, packed, self.P + self.used, self.cap - self.used)
            self.used = self.cap

    def close(self, eng: Engine):
        """Behind the render's backward: the workspace is consumed."""
        self.pctx = None
        # (a later pass through this graph -- retain_graph -- must not find this pass's adjoints where a node deposits none)
        eng.zero(self.gbuf)


class _TailEvalFn(torch.autograd.Function):
    """(sdf [m,1], g_o [m,3]) of ``m`` colour-less points evaluated into rows [off, off + m) of a live render's tail (``_Tail``).

    The only differentiable input is the render's ``token`` output: it makes the render node a dependency of this one, so autograd runs
    this backward -- which merely deposits the adjoints -- BEFORE the render's (even when nothing else of the render is used in the
    loss), and the render's backward carries them to the weights."""

    @staticmethod
    def forward(ctx, token, tail: _Tail, eng: Engine, off: int, m: int):
        pctx = tail.pctx
        r0 = tail.P + off
        sdf, go = eng.empty(m, 1), eng.empty(m, 3)          # own storage: outputs must not alias the workspace
        eng.copy2(sdf, pctx.view("sdf")[r0:], m, go, pctx.view("go")[r0:], 3 * m)
        ctx.tail, ctx.eng, ctx.off, ctx.m = tail, eng, off, m
        ctx.set_materialize_grads(False)
        return sdf, go

    @staticmethod
    def backward(ctx, d_sdf, d_go):
        tail, eng, off, m = ctx.tail, ctx.eng, ctx.off, ctx.m
        f = lambda g: None if g is None else f32(g)
        d_sdf, d_go = f(d_sdf), f(d_go)
        if d_sdf is not None or d_go is not None:
            eng.copy2(tail.g_sdf[off:], d_sdf, m if d_sdf is not None else 0, tail.g_go[off:], d_go, 3 * m if d_go is not None else 0)
        return None, None, None, None, None


class _Lazy(torch.Tensor):
    """A result whose producing launches have not been ISSUED yet: every torch function that touches it first issues them (on the calling
    thread, in program order: whatever reads the value is enqueued behind them), then runs on the plain tensor.  Attribute getters
    (``.shape``, ``.dtype``, ``.requires_grad``, ``.grad_fn`` ...) do not trigger.  Used by ``errorondepth``: see ``_PendingEod``."""

    # what may be asked of the tensor without its value (everything else -- including the ``.data`` / ``.T`` getters, which hand out
    # aliases of the storage -- issues the launches first)
    _META = frozenset(("shape", "dtype", "device", "requires_grad", "grad_fn", "is_cuda", "is_leaf", "ndim", "layout", "names", "is_sparse",
                       "is_quantized", "is_meta", "output_nr", "_version", "grad", "is_cpu", "itemsize", "nbytes"))
    _META_FN = frozenset(("dim", "size", "numel", "ndimension", "nelement", "is_contiguous", "is_floating_point", "is_complex", "stride",
                          "element_size", "get_device"))

    @staticmethod
    def wrap(t: torch.Tensor, pending):
        r = t.as_subclass(_Lazy)
        r._es_pending = pending
        return r

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        meta = (name == "__get__" and getattr(getattr(func, "__self__", None), "__name__", "") in cls._META) or name in cls._META_FN

        def plain(a):
            if isinstance(a, _Lazy):
                p = a.__dict__.get("_es_pending")
                if p is not None and not meta:
                    p.force()
                return a.as_subclass(torch.Tensor)
            if isinstance(a, (list, tuple)):
                return type(a)(plain(b) for b in a)
            return a

        with torch._C.DisableTorchFunctionSubclass():
            return func(*[plain(a) for a in args], **{k: plain(v) for k, v in kwargs.items()})


class _PendingEod:
    """``errorondepth``'s network evaluation + reductions, not issued yet.  The reference trainer reads ``sdf_loss`` / ``angle_loss`` only
    after it has called ``surface_neighbour_error`` (trainer_endosurf.py:139-162), whose own colour-less points take the rows right
    behind these in the render workspace's tail: the two evaluations then go out as ONE launch chain (deformation on 16-point tiles, SDF +
    VJP on 32-row tiles: 96 workgroups at one tile's latency instead of 32, then 64, at one tile's latency EACH: 0.37 ms per step).
    ``force()`` issues whatever is still missing; it is called by the next evaluation into the same tail (which folds these rows into
    its launch first), by the first torch function that touches a result (``_Lazy``), by this node's backward and by the render's
    backward -- whichever comes first; so nothing depends on the caller's order of calls, only the saving does."""

    def __init__(self, eng: Engine, tail, off, n, rays, mask, weff, packed):
        # (weak references: the tail is kept alive by the render's autograd node, which every reader of the results reaches through this
        # evaluation's own node; a strong one would close a cycle with ``tail.pending`` around the 6.7 GB workspace)
        self._tail, self.off, self.n, self.m64 = weakref.ref(tail), int(off), int(n), _Tail.rows64(n)
        self.rays, self.mask, self.weff, self.packed, self.eng = rays, mask, weff, packed, eng
        self.out, self.inside = eng.empty(3), eng.empty(n, 1)
        self.sdf, self.go = eng.empty(n, 1), eng.empty(n, 3)
        self.rows_done, self.done = False, False
        self.stream = torch.cuda.current_stream(eng.device)

    @property
    def tail(self):
        t = self._tail()
        if t is None:
            raise RuntimeError("errorondepth's deferred evaluation outlived the render it was placed in")
        return t

    def force(self):
        if self.done:
            return
        eng, tail = self.eng, self.tail
        self.done = True
        tail.issued(self)
        cur = torch.cuda.current_stream(eng.device)
        with torch.no_grad(), torch.cuda.stream(self.stream):          # (on the stream the call was made on, whoever triggers it)
            if tail.pctx is None:
                raise RuntimeError("errorondepth's deferred evaluation outlived the render workspace it was placed in")
            if not self.rows_done:
                eng.point_forward_rows(tail.pctx, self.weff, self.packed, tail.P + self.off, self.m64)
                self.rows_done = True
            r0, n = tail.P + self.off, self.n
            eng.copy2(self.sdf, tail.pctx.view("sdf")[r0:], n, self.go, tail.pctx.view("go")[r0:], 3 * n)
            eng.eod_loss(self.rays, tail.aux_x[self.off:], self.mask, self.sdf, self.go, n, self.out, self.inside)
        if cur != self.stream:
            cur.wait_stream(self.stream)


class _LazyEodFn(torch.autograd.Function):
    """(sdf_error, angle_error) of a ``_PendingEod``: the autograd node exists from the call on, its values from ``force()`` on.  Like
    ``_TailEvalFn`` it hangs on the render's token and deposits the points' adjoints in the tail for the render's backward."""

    @staticmethod
    def forward(ctx, token, pending: _PendingEod):
        ctx.pending = pending
        ctx.set_materialize_grads(False)
        return pending.out[0], pending.out[1]

    @staticmethod
    def backward(ctx, g_sdf_err, g_ang_err):
        p = ctx.pending
        if g_sdf_err is None and g_ang_err is None:
            return None, None
        p.force()
        eng, tail, n = p.eng, p.tail, p.n
        f = lambda g: None if g is None else g.detach().to(torch.float32).reshape(1)
        ga, gb = f(g_sdf_err), f(g_ang_err)
        eng.eod_loss_backward(p.rays, p.inside, p.sdf, p.go, p.out, ga, gb, n, tail.g_sdf[p.off:], tail.g_go[p.off:])
        return None, None

"""Autograd functions of the shared per-position MLP stack, built on the C-ABI kernels.

Activations are channels-last matrices [P, C] (P = B*S*K grouped samples or B*N points).  A
"shared MLP" is the reference's (Conv1x1 -> train-mode BatchNorm -> ReLU) x L chain, optionally
followed by the max over the K samples of each group (models/pointnet_util.py:195-199,
:252-256, :310-313).  Here each layer is ONE MFMA GEMM whose prologue applies the previous
layer's BatchNorm+ReLU while loading ("normalise on load") and whose epilogue emits the partial
sums for its own BatchNorm, so no normalised activation is ever written to HBM.
"""
import collections
import ctypes
import os
from typing import NamedTuple, Optional

import torch

from . import profiler
from . import arena as zero_pool
from ._lib import call, cur_stream, dll, ptr, query

NT, NN, TN = 0, 1, 2
EPI_NONE, EPI_CHORD, EPI_MSKERNEL, EPI_MSBWD = 0, 1, 2, 3
_LL = ctypes.c_longlong
_F = ctypes.c_float
_D = ctypes.c_double


def _rows_per_slab():
    return query("prifit_reduce_rows_per_slab")


_STREAM = os.environ.get("PRIFIT_GEMM_STREAM", "1") != "0"   # 0: every product takes the tiled kernel (A/B runs)
_FUSE_RED = os.environ.get("PRIFIT_FUSE_BN_REDUCE", "1") != "0"  # 0: separate bn_relu_bwd_reduce launches (A/B runs)
_FUSE_POOL_FWD = os.environ.get("PRIFIT_FUSE_POOL_FWD", "1") != "0"  # 0: pool_fwd re-reads the last layer's Y (A/B runs)
_FUSE_BN_APPLY = os.environ.get("PRIFIT_FUSE_BN_APPLY", "1") != "0"  # 0: bn_relu_bwd_apply writes a middle layer's dY (A/B runs)
_FUSE_POOL = os.environ.get("PRIFIT_FUSE_POOL_BWD", "1") != "0"  # 0: pool_bwd_apply writes the pooled layer's dY (A/B runs)
# dA and dW of a streaming-shape layer from ONE pass over its rows (csrc/gemm_stream_bwd.hip) instead of the separate
# streaming dA (NN) and dW (TN) kernels, which each read G, Y and the previous layer's pre-activation.  "auto" (default):
# where it measured faster -- the unpooled middle layers (_FUSE_BWD_AUTO below; round 3 had only the 96 -> 64 one);
# "1": every supported shape (slower on the others: the kernel's dW role is latency-bound); "0": never.
_FUSE_BWD = os.environ.get("PRIFIT_FUSE_DA_DW", "auto")

# (round 4, tools/fam_table.py on one box: one-pass kernel against the separate dA + dW pair)
#   [1.57 M x 96 x 64] 546 / 712 us, [786 K x 64 x 64] 171 / 282, [197 K x 128 x 128] 152 / 176, [49 K x 128 x 128] 54 / 72;
#   pooled layers stay on the pairs: [1.57 M x 128 x 96] 887 / 874, [786 K x 128 x 64] 337 / 304
_FUSE_BWD_AUTO = {(96, 64), (64, 64), (128, 128)}


def _fuse_bwd_on(Cout, Kin, pooled):
    if _FUSE_BWD == "auto":
        return (Cout, Kin) in _FUSE_BWD_AUTO and not pooled
    return _FUSE_BWD not in ("0", "")


def _bn_tile(N):
    """Column tile of the tiled kernel's instantiation for N output columns (the span names carry it)."""
    return 32 if N <= 32 else (64 if N <= 64 else (96 if N <= 96 else 128))


def _stream_ok(layout, M, N, K, batch=1, splitk=1, epi=EPI_NONE, b_affine=None, a_rowsum=None, accumulate=False,
               aux=None, row_add=None, bias_stride=0):
    """The tall-and-skinny products of the shared MLPs (forward NT, dA NN) take the weights-stationary streaming
    kernel (csrc/gemm_stream.hip); everything else the tiled kernel (csrc/gemm.hip)."""
    return (_STREAM and batch == 1 and splitk == 1 and epi == EPI_NONE and b_affine is None and a_rowsum is None and
            not accumulate and aux is None and row_add is None and
            bool(query("prifit_gemm_stream_supported", layout, M, N, K)))


def slab_sum(part):
    """part [nslab, ...] -> its sum over the slabs in a fixed order (prifit_slab_sum; torch's reduction: 10-13 us + a memset)."""
    part = part.contiguous()
    out = torch.empty(part.shape[1:], dtype=torch.float32, device=part.device)
    call("prifit_slab_sum", ptr(part), part.shape[0], _LL(out.numel()), ptr(out), cur_stream())
    return out


def gemm_stats_slabs(M, N, K, aligned=True):
    """Number of column-statistics slabs a forward (NT) product of this shape writes (aligned=False: gemm() keeps an operand
    that is not 16-byte aligned off the streaming kernel)."""
    if aligned and _stream_ok(NT, M, N, K):
        return query("prifit_gemm_stream_slabs", M, K)
    t = query("prifit_gemm_stats_tile_m", M, N)
    return (M + t - 1) // t


def gemm(layout, M, N, K, A, lda, B, ldb, C, ldc, batch=1, sA=0, sB=0, sC=0, splitk=1, a_affine=None,
         b_affine=None, bias=None, bias_stride=0, stats=None, epi=EPI_NONE, epi_scalar=None, aux=None, ld_aux=0, s_aux=0,
         row_add=None, a_rowsum=None, accumulate=None, tiled_stats=False):
    """tiled_stats=True: the caller reads `stats` as one slab per 128 rows of C (per-sample statistics, src/dgcnn.py);
    otherwise the slab count is gemm_stats_slabs(M, N, K)."""
    if accumulate is None:
        accumulate = splitk > 1
    if (not (tiled_stats and stats is not None) and _stream_ok(layout, M, N, K, batch, splitk, epi, b_affine, a_rowsum, accumulate, aux, row_add) and lda % 4 == 0 and
            A.data_ptr() % 16 == 0 and (layout == NN or (ldb % 4 == 0 and B.data_ptr() % 16 == 0))):
        # HBM-bound: the span's work is the algorithmic bytes (A read once, C written once, B once)
        with profiler.span(profiler.tag("gemm_stream_%s" % ("nt", "nn")[layout], M, N, K), 4.0 * (M * K + M * N + N * K)):
            call("prifit_gemm_stream_f32", layout, M, N, K, ptr(A), _LL(lda), ptr(B), _LL(ldb), ptr(C), _LL(ldc),
                 ptr(a_affine[0]) if a_affine else None, ptr(a_affine[1]) if a_affine else None, ptr(bias), ptr(stats),
                 cur_stream())
        return
    # span name = the kernel instantiation (layout, BN tile) so that it lines up with rocprofv3's per-kernel rows
    with profiler.span(profiler.tag("gemm_%s_bn%d" % (("nt", "nn", "tn")[layout], _bn_tile(N)), M, N, K, batch, splitk),
                       2.0 * M * N * K * batch):
        call("prifit_gemm_f32", layout, M, N, K, ptr(A), _LL(lda), _LL(sA), ptr(B), _LL(ldb), _LL(sB), ptr(C),
             _LL(ldc), _LL(sC), batch, splitk,
             ptr(a_affine[0]) if a_affine else None, ptr(a_affine[1]) if a_affine else None,
             ptr(b_affine[0]) if b_affine else None, ptr(b_affine[1]) if b_affine else None,
             ptr(bias), _LL(bias_stride), ptr(stats), epi, ptr(epi_scalar), ptr(aux), _LL(ld_aux), _LL(s_aux), ptr(row_add),
             ptr(a_rowsum), int(accumulate), cur_stream())


# split-K of the tiled dW products: one round of resident workgroups (512: two 8-wave workgroups per CU) measured best
# ([256 x 196 x 393 K]: 549 / 455 / 466 / 494 us at 256 / 512 / 1024 / 2048 workgroups)
_SPLITK_WGS = 512


def _splitk_for(P, tiles):
    """Workgroups along the reduction for dW = dY^T A: aim at _SPLITK_WGS workgroups, >= 8 k-tiles each."""
    ktiles = (P + 31) // 32
    want = max(1, _SPLITK_WGS // max(1, tiles))
    return int(max(1, min(want, ktiles // 8 if ktiles >= 8 else 1, 4096)))


def _weight_grad(dY, P, Cout, Ain, Kin, a_affine, out=None):
    """dW [Cout, Kin] = dY[P, Cout]^T . A[P, Kin] (A optionally normalised on load).  `out`: a zero-filled
    [Cout, Kin] destination (several layers share one zeroed arena: one fill instead of one per layer)."""
    if _STREAM and query("prifit_gemm_stream_tn_supported", Cout, Kin, P):
        # tall reduction, small output: the LDS-free streaming kernel (csrc/gemm_stream.hip), HBM-bound
        dW = out if out is not None else zero_pool.zeros(Cout, Kin, device=dY.device)
        ws = torch.empty(query("prifit_gemm_stream_tn_workspace", Cout, Kin, P), dtype=torch.float32, device=dY.device)
        with profiler.span(profiler.tag("gemm_stream_tn", Cout, Kin, P), 4.0 * P * (Cout + Kin)):
            call("prifit_gemm_stream_tn_f32", Cout, Kin, _LL(P), ptr(dY), _LL(dY.stride(0)), ptr(Ain), _LL(Ain.stride(0)),
                 ptr(dW), _LL(Kin), ptr(a_affine[0]) if a_affine else None, ptr(a_affine[1]) if a_affine else None,
                 ptr(ws), cur_stream())
        return dW
    tiles = ((Cout + 127) // 128) * ((Kin + 127) // 128)
    sk = _splitk_for(P, tiles)
    if out is not None:
        dW = out
    elif sk == 1:
        dW = torch.empty(Cout, Kin, dtype=torch.float32, device=dY.device)
    else:
        dW = zero_pool.zeros(Cout, Kin, device=dY.device)
    gemm(TN, Cout, Kin, P, dY, dY.stride(0), Ain, Ain.stride(0), dW, Kin, splitk=sk, b_affine=a_affine)
    return dW


class _FwdRoute(NamedTuple):
    """How one layer of SharedMLPFn.forward comes about (DESIGN.md 3.1 has the entry points in order): the arm (a key of
    _FWD_ARMS), where the layer's column-statistics slab comes from ("front": the launch that computed layer 0; "launch": the
    arm's own product; None: eval mode, running statistics) and whether the arm leaves pool candidates.
      preact         layer 0 computed elsewhere (cfg["front"])
      norows_gather  layer 1 over first-layer rows that were never stored: the streaming product gathers them from U
      eval           the general product with bias, no statistics
      stream_pool / tiled_pool   a max-pooled last layer whose epilogue also emits (max, argmax, min, argmin) per 32 rows and
                     column, so that the pool reads those candidates (1/8 of Y) instead of Y -- on the streaming kernel, or on
                     the tiled (persistent) one (SA2's 256-wide last layers)
      gemm           the general product with a statistics slab: everything else"""
    arm: str
    slab: Optional[str]
    cand: bool


def _forward_route(l, L, P, Cout, Kin, pool_K, training, mode, aligned, has_affine):
    """The route of layer l of an L-layer stack over P rows (Cout x Kin weights); launches nothing, allocates nothing, reads the
    module switches and query(...) only, at every call (tests flip the switches between two calls).  mode: as in
    _backward_route; aligned: the layer's input rows and weights are 16-byte aligned with a row stride % 4 == 0; has_affine:
    the layer below hands its (scale, shift) on (every layer but the first of a "plain" stack)."""
    if l == 0 and mode != "plain":
        return _FwdRoute("preact", "front", False)
    if l == 1 and mode == "norows":
        assert training and L >= 3, "norows: a training-mode stack of >= 3 layers (pointnet_util._norows_scales)"
        return _FwdRoute("norows_gather", "launch", False)
    if not training:
        return _FwdRoute("eval", None, False)
    if l == L - 1 and pool_K and pool_K % 32 == 0 and _FUSE_POOL_FWD and aligned and has_affine:
        if _stream_ok(NT, P, Cout, Kin):
            return _FwdRoute("stream_pool", "launch", True)
        if query("prifit_gemm_pool_supported", P, Cout, Kin):
            return _FwdRoute("tiled_pool", "launch", True)
    return _FwdRoute("gemm", "launch", False)


class _FwdLayer(NamedTuple):
    """What a forward arm reads: the stack's rows P and device, the layer's widths, its input rows `prev` (None: never stored,
    the norows arm re-forms them from front.U / Vc) with the (scale, shift) `aff` of the layer below applied on load (None: raw
    input), its contiguous weight W and bias, the stack's FrontEnd (or None), and `aligned` as _forward_route takes it."""
    P: int
    Cout: int
    Kin: int
    dev: torch.device
    prev: Optional[torch.Tensor]
    aff: Optional[tuple]
    W: Optional[torch.Tensor]
    bias: Optional[torch.Tensor]
    front: Optional[tuple]
    aligned: bool


# The forward arms: f(ly) -> (Y [P, Cout], the slab of its column statistics or None, the pool candidates or None).

def _fwd_preact(ly):
    return ly.prev, ly.front.slab, None


def _fwd_eval(ly):
    Y = torch.empty(ly.P, ly.Cout, dtype=torch.float32, device=ly.dev)
    gemm(NT, ly.P, ly.Cout, ly.Kin, ly.prev, ly.prev.stride(0), ly.W, ly.Kin, Y, ly.Cout, a_affine=ly.aff, bias=ly.bias)
    return Y, None, None


def _fwd_norows_gather(ly):
    P, Cout, Kin, nr = ly.P, ly.Cout, ly.Kin, ly.front
    assert ly.prev is None
    Y = torch.empty(P, Cout, dtype=torch.float32, device=ly.dev)
    slab = torch.empty(query("prifit_gemm_stream_slabs", P, Kin), 2, Cout, dtype=torch.float32, device=ly.dev)
    with profiler.span(profiler.tag("gemm_stream_nt", P, Cout, Kin, "gather"), 4.0 * (P * Cout + P + Cout * Kin)):
        call("prifit_gemm_stream_gather_f32", P, Cout, ptr(nr.idx), ptr(nr.U), ptr(nr.Vc), nr.N, nr.S,
             nr.K, ptr(ly.W), _LL(Kin), ptr(Y), _LL(Cout), ptr(ly.aff[0]), ptr(ly.aff[1]), ptr(ly.bias), ptr(slab),
             cur_stream())
    return Y, slab, None


def _fwd_stream_pool(ly):
    P, Cout, Kin, prev, dev = ly.P, ly.Cout, ly.Kin, ly.prev, ly.dev
    Y = torch.empty(P, Cout, dtype=torch.float32, device=dev)
    slab = torch.empty(query("prifit_gemm_stream_slabs", P, Kin), 2, Cout, dtype=torch.float32, device=dev)
    cand = torch.empty(P // 32, 4, Cout, dtype=torch.float32, device=dev)
    with profiler.span(profiler.tag("gemm_stream_nt", P, Cout, Kin, 1), 4.0 * (P * Kin + P * Cout + Cout * Kin)):
        call("prifit_gemm_stream_pool_f32", P, Cout, Kin, ptr(prev), _LL(prev.stride(0)), ptr(ly.W), _LL(Kin),
             ptr(Y), _LL(Cout), ptr(ly.aff[0]), ptr(ly.aff[1]), ptr(ly.bias), ptr(slab), ptr(cand), cur_stream())
    return Y, slab, cand


def _fwd_tiled_pool(ly):
    P, Cout, Kin, prev, dev = ly.P, ly.Cout, ly.Kin, ly.prev, ly.dev
    Y = torch.empty(P, Cout, dtype=torch.float32, device=dev)
    slab = torch.empty(gemm_stats_slabs(P, Cout, Kin), 2, Cout, dtype=torch.float32, device=dev)   # (not a streaming shape)
    cand = torch.empty(P // 32, 4, Cout, dtype=torch.float32, device=dev)
    with profiler.span(profiler.tag("gemm_nt_bn128", P, Cout, Kin, "pool"), 2.0 * P * Cout * Kin):
        call("prifit_gemm_pool_f32", P, Cout, Kin, ptr(prev), _LL(prev.stride(0)), ptr(ly.W), _LL(Kin), ptr(Y),
             _LL(Cout), ptr(ly.aff[0]), ptr(ly.aff[1]), ptr(ly.bias), ptr(slab), ptr(cand), cur_stream())
    return Y, slab, cand


def _fwd_gemm(ly):
    P, Cout, Kin = ly.P, ly.Cout, ly.Kin
    Y = torch.empty(P, Cout, dtype=torch.float32, device=ly.dev)
    slab = torch.empty(gemm_stats_slabs(P, Cout, Kin, ly.aligned), 2, Cout, dtype=torch.float32, device=ly.dev)
    gemm(NT, P, Cout, Kin, ly.prev, ly.prev.stride(0), ly.W, Kin, Y, Cout, a_affine=ly.aff, bias=ly.bias, stats=slab)
    return Y, slab, None


_FWD_ARMS = {"preact": _fwd_preact, "eval": _fwd_eval, "norows_gather": _fwd_norows_gather, "stream_pool": _fwd_stream_pool,
             "tiled_pool": _fwd_tiled_pool, "gemm": _fwd_gemm}


def _forward_output(cfg, Y, aff, cand, P, dev):
    """The stack's output from its last layer's rows Y and coefficients -> (out, arg): the max over each group of
    cfg["pool_K"] rows of relu(scale Y + shift) with its int32 winners (from `cand`, where the last layer's arm left pool
    candidates, else from Y), or relu(scale Y + shift) itself and None."""
    CL, pool_K = Y.shape[1], cfg["pool_K"]
    if not pool_K:
        out = torch.empty(P, CL, dtype=torch.float32, device=dev)
        call("prifit_affine_relu", ptr(Y), _LL(CL), ptr(aff[0]), ptr(aff[1]), P, CL, 0, _F(0.0), ptr(out), _LL(CL), cur_stream())
        return out, None
    G = P // pool_K
    # pool_out: a [G, CL] column window of the level's concatenated output (the scales of a multi-scale level write
    # side by side: no torch.cat); the pool kernels take a leading dimension
    out = cfg.get("pool_out")
    if out is None:
        out = torch.empty(G, CL, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (G, CL) or out.stride(1) != 1 or out.dtype != torch.float32 or out.device != dev:
        raise ValueError("pool_out must be a [G, C] fp32 column window on the input's device")
    arg = torch.empty(G, CL, dtype=torch.int32, device=dev)
    if cand is not None:
        call("prifit_pool_from_candidates", ptr(cand), ptr(aff[0]), ptr(aff[1]), G, pool_K, CL, 0, _F(0.0),
             ptr(out), _LL(out.stride(0)), ptr(arg), None, cur_stream())
    else:
        call("prifit_pool_fwd", ptr(Y), _LL(CL), ptr(aff[0]), ptr(aff[1]), G, pool_K, CL, 0, _F(0.0),
             ptr(out), _LL(out.stride(0)), ptr(arg), cur_stream())
    return out, arg


# How one layer of SharedMLPFn.backward gets from (G, its coefficients) to the gradient of the layer below.
#   name    kernel                      what runs (DESIGN.md 3.1 has the entry points in order)
#   pool    one_pass | pair             pooled last layer, dY = T*[k == arg] + b*Y + d formed inside its consumers from Y itself
#   bn      one_pass | pair             middle layer, dY = a*(relu mask)*G + b*Y + d formed inside its consumers from G and Y
#   norows  one_pass                    layer 2 over first-layer rows that were never stored
#   direct0 rows | gather               first conv of a direct-mode set-abstraction scale: its weight gradient, dY formed on load
#   gather0 csr | atomic                first layer by linearity: dU / dVc, dY formed on load
#   preact0 None                        layer 0 is a pre-activation computed elsewhere: its dY is the gradient handed back
#   plain   stream | tiled | gemm | None   dY written by an apply pass, then dW, then dA by the named kernel (None: not needed)
# red: the route leaves the BatchNorm-backward (m1, m2) sums of the layer below, which then skips its own reduce pass.
_Route = collections.namedtuple("_Route", "name kernel red")


def _backward_route(l, L, P, Cout, Kin, pool_K, training, mode, need_dW, need_dx, g_dense, g_contig, below_ld4, N0=0):
    """The route of layer l of an L-layer stack over P rows (Cout x Kin weights); launches nothing, reads the module switches
    and query(...) only, at every call (tests flip the switches between two calls).
    mode: how layer 0 comes about -- "plain" (a product like the others), "preact" (x is its pre-activation), "direct" /
    "gather" (fused set-abstraction front end whose input gradients this function owns), "norows" (direct, rows not stored).
    need_dW / need_dx: the layer's weight slot / the stack's input wants a gradient.  g_dense: G has row stride Cout and is
    16-byte aligned; g_contig: G is contiguous; below_ld4: the row stride of the layer below is a multiple of 4; N0: points
    per cloud (gather mode)."""
    pooled = l == L - 1 and bool(pool_K)

    def streams():   # both consumers of the layer's dY are streaming shapes
        return _stream_ok(NN, P, Kin, Cout) and bool(query("prifit_gemm_stream_tn_supported", Cout, Kin, P))

    # (groups of 64 rows: what the *_pool_f32 kernels take, against 32 in the forward epilogue; no 96-wide layer: kept as found)
    if pooled and _FUSE_POOL and training and l > 0 and pool_K % 64 == 0 and Cout != 96 and need_dW and streams():
        if (_fuse_bwd_on(Cout, Kin, True) and _FUSE_RED and query("prifit_gemm_stream_bwd_supported", P, Cout, Kin, pool_K) and
                below_ld4):
            return _Route("pool", "one_pass", True)
        return _Route("pool", "pair", bool(_FUSE_RED))
    if l == 0 and mode in ("direct", "norows"):
        return _Route("direct0", "gather" if mode == "norows" else "rows", False)
    if l == 0 and mode == "gather":
        csr = _GATHER_BWD_CSR and query("prifit_gather_linear_bwd_csr_supported", N0, Cout) and g_contig
        return _Route("gather0", "csr" if csr else "atomic", False)
    fuse_bn = bool(_FUSE_BN_APPLY and _FUSE_RED and not pooled and training and l > 0 and need_dW and g_dense and streams())
    if l == 1 and mode == "norows":
        assert fuse_bn, "norows: the streaming backward of layer 2 is required (pointnet_util._norows_scales)"
        return _Route("norows", "one_pass", True)
    if fuse_bn:
        if _fuse_bwd_on(Cout, Kin, False) and query("prifit_gemm_stream_bwd_supported", P, Cout, Kin, 0) and below_ld4:
            return _Route("bn", "one_pass", True)
        return _Route("bn", "pair", True)
    if l == 0:
        if mode == "preact":
            return _Route("preact0", None, False)
        return _Route("plain", "gemm" if need_dx else None, False)
    if not _FUSE_RED:
        return _Route("plain", "gemm", False)
    return _Route("plain", "stream" if _stream_ok(NN, P, Kin, Cout) else "tiled", True)


class _BwdLayer(NamedTuple):
    """What a route reads, built by SharedMLPFn.backward once per layer.  Every route: P, Cout, dev, G (the gradient w.r.t. the
    layer's ReLU or pooled output), Y, the layer's (scale, shift) and its backward coefficients ca, cb, cd (dY = ca Gm + cb Y +
    cd).  The routes with a layer below (pool, bn, norows, plain): Kin, W, Yp / aff_p / stats_p -- the rows, (scale, shift) and
    (mean, invstd) of the layer below (x, None, None at layer 0) -- and dW, the layer's zero-filled [Cout, Kin] window of the
    stack's arena (None if not wanted).  pool and plain: pooled, pool_K, arg (the pool's winners).  direct0, gather0, norows:
    front (the stack's FrontEnd); gather0: bias0.  need_dW: direct0, plain; want_db (eval mode, the bias wants sum(dY)): plain."""
    P: int
    Cout: int
    Kin: int
    dev: torch.device
    pooled: bool
    pool_K: int
    arg: Optional[torch.Tensor]
    G: torch.Tensor
    Y: Optional[torch.Tensor]
    W: Optional[torch.Tensor]
    scale: torch.Tensor
    shift: torch.Tensor
    ca: torch.Tensor
    cb: torch.Tensor
    cd: torch.Tensor
    Yp: Optional[torch.Tensor]
    aff_p: Optional[tuple]
    stats_p: Optional[tuple]
    front: Optional[tuple]
    bias0: Optional[torch.Tensor]
    dW: Optional[torch.Tensor]
    need_dW: bool
    want_db: bool


# The routes: f(ly, route) -> (G_prev, dW or None, the slab of sums left for the layer below or None, extra).
# extra: gather0's dVc; the plain route's dY.sum(0) where ly.want_db asks for it; None otherwise.

def _fused_bwd(ly, route, Ttab=None):
    """Gp, dW and the (m1, m2) sums of the layer below from one pass over the layer's rows: prifit_gemm_stream_bwd_f32 (Ttab:
    the pooled layer, dY formed from the pool's table), or, on the norows route (the rows of the layer below were never stored),
    prifit_gemm_stream_bwd_gather_f32, which re-forms them from U."""
    P, Cout, Kin, G, Y, dev = ly.P, ly.Cout, ly.Kin, ly.G, ly.Y, ly.dev
    rslab = torch.empty(query("prifit_gemm_stream_bwd_slabs", P, Cout, Kin), 2, Kin, dtype=torch.float32, device=dev)
    ws = torch.empty(query("prifit_gemm_stream_bwd_workspace", P, Cout, Kin), dtype=torch.float32, device=dev)
    Gp = torch.empty(P, Kin, dtype=torch.float32, device=dev)
    (sc1, sh1), (mu1, is1) = ly.aff_p, ly.stats_p
    pooled = Ttab is not None
    if route.name == "norows":
        nr = ly.front
        with profiler.span(profiler.tag("gemm_stream_bwd", P, Cout, Kin, "gather"), 4.0 * P * (2 * Cout + Kin)):
            call("prifit_gemm_stream_bwd_gather_f32", _LL(P), Cout, ptr(G), ptr(Y), ptr(ly.scale), ptr(ly.shift), ptr(ly.ca),
                 ptr(ly.cb), ptr(ly.cd), ptr(ly.W), _LL(Kin), ptr(nr.idx), ptr(nr.U), ptr(nr.Vc), nr.N, nr.S, nr.K,
                 ptr(sc1), ptr(sh1), ptr(mu1), ptr(is1), ptr(Gp), _LL(Kin), ptr(rslab), ptr(ly.dW), _LL(Kin), ptr(ws),
                 cur_stream())
        return Gp, ly.dW, rslab, None
    # HBM-bound on the narrow layers: every tensor once (G and Y or Y alone, Yp in, Gp out)
    with profiler.span(profiler.tag("gemm_stream_bwd", P, Cout, Kin, "pool" if pooled else "bn"),
                       4.0 * P * ((1 if pooled else 2) * Cout + 2 * Kin)):
        call("prifit_gemm_stream_bwd_f32", _LL(P), Cout, Kin, ptr(None if pooled else G), ptr(Y), ptr(None if pooled else ly.scale),
             ptr(None if pooled else ly.shift), ptr(None if pooled else ly.ca), ptr(ly.cb), ptr(ly.cd),
             ptr(ly.arg if pooled else None), ptr(Ttab), ly.pool_K if pooled else 0, ptr(ly.W), _LL(Kin), ptr(ly.Yp),
             _LL(ly.Yp.stride(0)), ptr(sc1), ptr(sh1), ptr(mu1), ptr(is1), ptr(Gp), _LL(Kin), ptr(rslab), ptr(ly.dW), _LL(Kin),
             ptr(ws), cur_stream())
    return Gp, ly.dW, rslab, None


def _route_pool(ly, route):
    P, Cout, Kin, K, G, Y, W, Yp, dev = ly.P, ly.Cout, ly.Kin, ly.pool_K, ly.G, ly.Y, ly.W, ly.Yp, ly.dev
    Ttab = torch.empty(P // K, Cout, dtype=torch.float32, device=dev)
    call("prifit_pool_bwd_table", ptr(G), _LL(G.stride(0)), ptr(Y), _LL(Cout), ptr(ly.arg), ptr(ly.scale),
         ptr(ly.shift), ptr(ly.ca), P // K, K, Cout, _F(0.0), ptr(Ttab), cur_stream())
    if route.kernel == "one_pass":
        return _fused_bwd(ly, route, Ttab)
    ws = torch.empty(query("prifit_gemm_stream_tn_workspace", Cout, Kin, P), dtype=torch.float32, device=dev)
    (sc1, sh1), (mu1, is1) = ly.aff_p, ly.stats_p
    with profiler.span(profiler.tag("gemm_stream_tn", Cout, Kin, P, 1), 4.0 * P * (Cout + Kin)):
        call("prifit_gemm_stream_tn_pool_f32", Cout, Kin, _LL(P), ptr(Y), _LL(Cout), ptr(Yp), _LL(Yp.stride(0)), ptr(ly.dW),
             _LL(Kin), ptr(sc1), ptr(sh1), ptr(ly.arg), ptr(Ttab), ptr(ly.cb), ptr(ly.cd), K, ptr(ws), cur_stream())
    G_prev = torch.empty(P, Kin, dtype=torch.float32, device=dev)
    bias_dw = torch.mv(W.t(), ly.cd)   # the constant d^T W of every row of dY . W
    rslab = None
    if route.red:
        rslab = torch.empty(query("prifit_gemm_stream_slabs", P, Cout), 2, Kin, dtype=torch.float32, device=dev)
    with profiler.span(profiler.tag("gemm_stream_nn", P, Kin, Cout, 1), 4.0 * (P * Cout + 2 * P * Kin + Kin * Cout)):
        call("prifit_gemm_stream_dgrad_pool_f32", P, Kin, Cout, ptr(Y), _LL(Cout), ptr(W), _LL(Kin), ptr(G_prev),
             _LL(Kin), ptr(bias_dw), ptr(ly.arg), ptr(Ttab), ptr(ly.cb), K, ptr(Yp), _LL(Yp.stride(0)),
             ptr(sc1), ptr(sh1), ptr(mu1), ptr(is1), ptr(rslab), cur_stream())
    return G_prev, ly.dW, rslab, None


def _route_bn(ly, route):
    if route.kernel == "one_pass":
        return _fused_bwd(ly, route)
    P, Cout, Kin, G, Y, W, Yp, dev = ly.P, ly.Cout, ly.Kin, ly.G, ly.Y, ly.W, ly.Yp, ly.dev
    ws = torch.empty(query("prifit_gemm_stream_tn_workspace", Cout, Kin, P), dtype=torch.float32, device=dev)
    (sc1, sh1), (mu1, is1) = ly.aff_p, ly.stats_p
    with profiler.span(profiler.tag("gemm_stream_tn", Cout, Kin, P, "bn"), 4.0 * P * (2 * Cout + Kin)):
        call("prifit_gemm_stream_tn_bn_f32", Cout, Kin, _LL(P), ptr(G), ptr(Y), _LL(Cout), ptr(Yp), _LL(Yp.stride(0)),
             ptr(ly.dW), _LL(Kin), ptr(sc1), ptr(sh1), ptr(ly.scale), ptr(ly.shift), ptr(ly.ca), ptr(ly.cb), ptr(ly.cd), ptr(ws),
             cur_stream())
    G_prev = torch.empty(P, Kin, dtype=torch.float32, device=dev)
    rslab = torch.empty(query("prifit_gemm_stream_slabs", P, Cout), 2, Kin, dtype=torch.float32, device=dev)
    with profiler.span(profiler.tag("gemm_stream_nn", P, Kin, Cout, "bn"), 4.0 * (2 * P * Cout + 2 * P * Kin + Kin * Cout)):
        call("prifit_gemm_stream_dgrad_bn_f32", P, Kin, Cout, ptr(G), ptr(Y), _LL(Cout), ptr(W), _LL(Kin), ptr(G_prev),
             _LL(Kin), ptr(ly.scale), ptr(ly.shift), ptr(ly.ca), ptr(ly.cb), ptr(ly.cd), ptr(Yp), _LL(Yp.stride(0)),
             ptr(sc1), ptr(sh1), ptr(mu1), ptr(is1), ptr(rslab), cur_stream())
    return G_prev, ly.dW, rslab, None


def _route_direct0(ly, route):
    """dW1 = dY^T [feat | rel] of a direct-mode set-abstraction scale's first conv, with dY formed on load."""
    if not ly.need_dW:
        return None, None, None, None
    P, Cout, G, fe, dev = ly.P, ly.Cout, ly.G, ly.front, ly.dev
    nblk = int(max(1, min(1024, (P + 1023) // 1024)))
    part = torch.empty(nblk, Cout, fe.D + 3, dtype=torch.float32, device=dev)
    if route.kernel == "gather":
        with profiler.span("sa_first_layer_dw", 4.0 * P * (Cout + 1)):
            call("prifit_sa_first_layer_dw_bn_gather", ptr(G), ptr(fe.U), ptr(fe.Vc), ptr(ly.scale), ptr(ly.shift),
                 ptr(ly.ca), ptr(ly.cb), ptr(ly.cd), ptr(fe.idx), ptr(fe.xyz), ptr(fe.new_xyz),
                 ptr(fe.feat), fe.B, fe.N, fe.S, fe.K, Cout, fe.D, int(fe.feat_first), nblk, ptr(part), cur_stream())
    else:
        with profiler.span("sa_first_layer_dw", 4.0 * P * (2 * Cout + 1)):
            call("prifit_sa_first_layer_dw_bn", ptr(G), ptr(ly.Y), ptr(ly.scale), ptr(ly.shift), ptr(ly.ca), ptr(ly.cb), ptr(ly.cd),
                 ptr(fe.idx), ptr(fe.xyz), ptr(fe.new_xyz), ptr(fe.feat), fe.B, fe.N, fe.S, fe.K, Cout,
                 fe.D, int(fe.feat_first), nblk, ptr(part), cur_stream())
    return None, slab_sum(part), None, None


def _route_gather0(ly, route):
    """dU / dVc of a first layer by linearity straight from (G, Y): BatchNorm + ReLU backward formed on load."""
    P, Cout, G, fe, dev = ly.P, ly.Cout, ly.G, ly.front, ly.dev
    Bq, Nq, Sq, Kq = fe.B, fe.N, fe.S, fe.K
    if route.kernel == "csr":
        # as a gather over the in-edge lists of the points: no atomics, no staging, y1 re-formed from U / Vc (the
        # layer's rows are not read); the CSR of the ball-query lists is built here, once per level and scale
        Uq, Vq = fe.U.detach().contiguous(), fe.Vc.detach().contiguous()
        E = Sq * Kq
        offs = torch.empty(Bq, Nq + 1, dtype=torch.int32, device=dev)
        lst, pos, own = (torch.empty(Bq, E, dtype=torch.int32, device=dev) for _ in range(3))
        wsd = torch.empty(query("prifit_gather_linear_bwd_csr_workspace", Bq, Sq, Kq, Cout), dtype=torch.float64, device=dev)
        dU = torch.empty(Bq, Nq, Cout, dtype=torch.float32, device=dev)
        dVc = torch.empty(Bq, Sq, Cout, dtype=torch.float32, device=dev)
        # bytes: G twice (once per pass), the lists, the tables
        with profiler.span("gather_linear_bwd", 4.0 * (2.0 * P * Cout + 4.0 * P + 2.0 * (Bq * Nq + Bq * Sq) * Cout)):
            call("prifit_list_csr", ptr(fe.idx), Bq, Nq, E, ptr(offs), ptr(lst), ptr(pos), ptr(own), cur_stream())
            call("prifit_gather_linear_bwd_csr", ptr(G), ptr(Uq), ptr(Vq), ptr(ly.bias0), ptr(ly.scale), ptr(ly.shift),
                 ptr(ly.ca), ptr(ly.cb), ptr(ly.cd), ptr(fe.idx), ptr(offs), ptr(lst), ptr(own), Bq, Nq, Sq, Kq, Cout, ptr(dU),
                 ptr(dVc), ptr(wsd), cur_stream())
    else:
        # the scatter staged in LDS, with atomics
        dU = zero_pool.zeros(Bq, Nq, Cout, device=dev)
        dVc = zero_pool.zeros(Bq, Sq, Cout, device=dev)
        with profiler.span("gather_linear_bwd", 4.0 * (2.0 * P * Cout + P + (Bq * Nq + Bq * Sq) * Cout)):
            call("prifit_gather_linear_bwd_bn", ptr(G), ptr(ly.Y), ptr(ly.scale), ptr(ly.shift), ptr(ly.ca), ptr(ly.cb), ptr(ly.cd),
                 ptr(fe.idx), Bq, Nq, Sq, Kq, Cout, ptr(dU), ptr(dVc), cur_stream())
    return None, dU, None, dVc


def _route_plain(ly, route):
    """dY written out by the layer's apply pass (preact0: that is all), then dW, then dA by route.kernel."""
    P, Cout, Kin, G, W, Yp, dev = ly.P, ly.Cout, ly.Kin, ly.G, ly.W, ly.Yp, ly.dev
    dY = torch.empty(P, Cout, dtype=torch.float32, device=dev)
    if ly.pooled:
        call("prifit_pool_bwd_apply", ptr(G), _LL(G.stride(0)), ptr(ly.Y), _LL(Cout), ptr(ly.arg), ptr(ly.scale), ptr(ly.shift),
             ptr(ly.ca), ptr(ly.cb), ptr(ly.cd), P // ly.pool_K, ly.pool_K, Cout, 0, _F(0.0), ptr(dY), _LL(Cout), cur_stream())
    else:
        call("prifit_bn_relu_bwd_apply", ptr(G), _LL(G.stride(0)), ptr(ly.Y), _LL(Cout), ptr(ly.scale), ptr(ly.shift),
             ptr(ly.ca), ptr(ly.cb), ptr(ly.cd), P, Cout, 0, _F(0.0), ptr(dY), _LL(Cout), cur_stream())
    if route.name == "preact0":
        return dY, None, None, None
    dW = _weight_grad(dY, P, Cout, Yp, Kin, ly.aff_p, out=ly.dW) if ly.need_dW else None
    db = dY.sum(dim=0) if ly.want_db else None
    G_prev = None if route.kernel is None else torch.empty(P, Kin, dtype=torch.float32, device=dev)
    rslab = None
    if route.red:   # the dA product leaves the BatchNorm-backward column sums of the layer below: streaming or tiled kernel
        (sc1, sh1), (mu1, is1) = ly.aff_p, ly.stats_p
    if route.kernel == "gemm":
        gemm(NN, P, Kin, Cout, dY, Cout, W, Kin, G_prev, Kin)
    elif route.kernel == "stream":
        rslab = torch.empty(query("prifit_gemm_stream_slabs", P, Cout), 2, Kin, dtype=torch.float32, device=dev)
        with profiler.span(profiler.tag("gemm_stream_nn", P, Kin, Cout, 0), 4.0 * (P * Cout + 2 * P * Kin + Kin * Cout)):
            call("prifit_gemm_stream_dgrad_f32", P, Kin, Cout, ptr(dY), _LL(Cout), ptr(W), _LL(Kin), ptr(G_prev),
                 _LL(Kin), ptr(Yp), _LL(Yp.stride(0)), ptr(sc1), ptr(sh1), ptr(mu1), ptr(is1), ptr(rslab), cur_stream())
    elif route.kernel == "tiled":
        t = query("prifit_gemm_stats_tile_m", P, Kin)
        rslab = torch.empty((P + t - 1) // t, 2, Kin, dtype=torch.float32, device=dev)
        with profiler.span(profiler.tag("gemm_nn_bn%d" % _bn_tile(Kin), P, Kin, Cout, "red"), 2.0 * P * Kin * Cout):
            call("prifit_gemm_dgrad_bnred_f32", P, Kin, Cout, ptr(dY), _LL(Cout), ptr(W), _LL(Kin), ptr(G_prev),
                 _LL(Kin), ptr(Yp), _LL(Yp.stride(0)), ptr(sc1), ptr(sh1), ptr(mu1), ptr(is1), ptr(rslab), cur_stream())
    return G_prev, dW, rslab, db


_ROUTES = {"pool": _route_pool, "bn": _route_bn, "norows": _fused_bwd, "direct0": _route_direct0,
           "gather0": _route_gather0, "preact0": _route_plain, "plain": _route_plain}


def _eval_coeffs(gamma, beta, rmean, rvar, eps):
    """(scale, shift, mean, invstd) of an eval-mode BatchNorm, from its running statistics."""
    invstd = torch.rsqrt(rvar + eps)
    mean = rmean.clone()
    scale = gamma * invstd
    return scale, beta - mean * scale, mean, invstd


# How layer 0 of a shared-MLP stack came about when something else computed it: the record a set-abstraction front end
# (models/pointnet_util._sa_level) hands to SharedMLPFn as cfg["front"].  No record: layer 0 is a product like the others
# (_backward_route's mode "plain").  Fields a mode does not use are None.
#   mode     "preact": x is layer 0's pre-activation and its gradient is handed back (GatherLinearFn, SAGroup*Fn autograd);
#            "direct" / "gather": fused front end, x is plain data and SharedMLPFn owns the gradients of its inputs;
#            "norows": direct, and the rows are not even stored (x is None): their consumers re-form them from (idx, U, Vc)
#   slab     [nslab, 2, C] column statistics of x, written by the launch that produced it (read in training only: True
#            does in eval mode)
#   idx      int32 [B, S, K] ball-query lists;  B, N, S, K, D: clouds, points per cloud, centres, samples, feature width
#   xyz, new_xyz, feat, feat_first    what the direct-mode weight gradient dW1 = dY^T [feat | rel] gathers from
#   U, Vc    per-point / per-centre tables of the first layer by linearity (gather: differentiable; norows: data)
FrontEnd = collections.namedtuple("FrontEnd", "mode slab idx B N S K D xyz new_xyz feat feat_first U Vc",
                                  defaults=(None,) * 12)


def _mlp_tensors(convs, bns, first_weight):
    ts = []
    for i, (conv, bn) in enumerate(zip(convs, bns)):
        w = first_weight if i == 0 else conv.weight.reshape(conv.weight.shape[0], -1)
        ts += [w, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
    return ts


def front_end_args(cfg, convs, bns, front):
    """(cfg, tensors) of SharedMLPFn.apply(x, cfg, *tensors) for a stack whose layer 0 is described by `front` (a FrontEnd);
    cfg: the stack's base dict (pool_K, training, eps, momentum), which gains "front".  Layer 0 has no product, so its two
    weight slots carry what backward returns gradients for -- the one statement of that convention:
      mode               tensors[0] (W slot)                     tensors[1] (bias slot)   behind the 6 L layer tensors
      "preact"           None                                    None                     -
      "direct", "norows" first conv's weight, upstream [C1, D+3] the conv's bias          -
      "gather"           front.U                                 the conv's bias          front.Vc
    (the bias of a fused front end gets the zero gradient of a bias in front of batch statistics; the gather mode's csr
    backward re-forms y1 = U - Vc + bias from it)."""
    cfg["front"] = front
    if front.mode == "gather":
        return cfg, _mlp_tensors(convs, bns, front.U) + [front.Vc]
    if front.mode in ("direct", "norows"):
        return cfg, _mlp_tensors(convs, bns, convs[0].weight.reshape(convs[0].weight.shape[0], -1))
    ts = _mlp_tensors(convs, bns, None)
    ts[1] = None
    return cfg, ts


class _SavedLayer(NamedTuple):
    """What SharedMLPFn.forward keeps of one layer: its pre-activation rows Y [P, Cout] (layer 0 of a front end: x, None in mode
    "norows"), its contiguous weight (None: layer 0 of a front end, which has no product) and the BatchNorm coefficients
    applied to Y -- relu(scale Y + shift) is the layer's output, (mean, invstd) the statistics behind them."""
    Y: Optional[torch.Tensor]
    W: Optional[torch.Tensor]
    scale: torch.Tensor
    shift: torch.Tensor
    mean: torch.Tensor
    invstd: torch.Tensor


class _SavedStack(NamedTuple):
    """What SharedMLPFn.forward hands to backward: one _SavedLayer per layer, the input x, the pool's int32 winners (None:
    not pooled), the rows P and device, how layer 0 came about (_backward_route's mode) with the front end's record (the
    fused modes read it in backward), layer 0's bias slot (gather mode's csr backward re-forms y1 from it) and cfg without
    "front" / "pool_out"."""
    layers: list
    x: Optional[torch.Tensor]
    arg: Optional[torch.Tensor]
    P: int
    dev: torch.device
    mode: str
    front: Optional[tuple]
    bias0: Optional[torch.Tensor]
    cfg: dict


def _layer_dims(W, Y, front):
    """(Cout, Kin) of a layer from its weight; a front end's layer 0 (no weight): the width of its rows Y (of front.U where
    they are not stored), 0."""
    if W is not None:
        return W.shape
    return (front.U.shape[-1] if Y is None else Y.shape[1]), 0


def _grad_arena(st, needs):
    """One zero-filled arena for every weight gradient of the stack (split-K adds into it) and, in training, its (exactly
    zero) bias gradients -> (arena or None, {layer: (weight offset, weight size, bias offset, bias size)})."""
    wslots, total = {}, 0
    for l, sv in enumerate(st.layers):
        if sv.W is None:
            continue
        n = sv.W.numel() if needs[2 + 6 * l] else 0
        nb = sv.W.shape[0] if (st.cfg["training"] and needs[2 + 6 * l + 1]) else 0
        wslots[l] = (total, n, total + n, nb)
        total += n + nb
    return (zero_pool.zeros(total, device=st.dev) if total else None), wslots


def _bwd_coefficients(st, sv, Cout, pooled, G, fused_red):
    """The layer's backward coefficients [5, C] = dgamma, dbeta, a, b, d (dY = a Gm + b Y + d): prifit_bn_bwd_finalize from the
    slab of (m1, m2) sums -- prifit_pool_bwd_reduce for a pooled layer, else `fused_red` where the route of the layer above
    has left it, else prifit_bn_relu_bwd_reduce."""
    P, pool_K, dev = st.P, st.cfg["pool_K"], st.dev
    coefs = torch.empty(5, Cout, dtype=torch.float32, device=dev).unbind(0)
    if pooled:
        prs = query("prifit_pool_reduce_groups_per_slab")
        slab = torch.empty((P // pool_K + prs - 1) // prs, 2, Cout, dtype=torch.float32, device=dev)
        call("prifit_pool_bwd_reduce", ptr(G), _LL(G.stride(0)), ptr(sv.Y), _LL(Cout), ptr(st.arg), ptr(sv.scale),
             ptr(sv.shift), ptr(sv.mean), ptr(sv.invstd), P // pool_K, pool_K, Cout, 0, _F(0.0), ptr(slab), cur_stream())
    elif fused_red is not None:
        slab = fused_red
    else:
        rps = _rows_per_slab()
        slab = torch.empty((P + rps - 1) // rps, 2, Cout, dtype=torch.float32, device=dev)
        call("prifit_bn_relu_bwd_reduce", ptr(G), _LL(G.stride(0)), ptr(sv.Y), _LL(Cout), ptr(sv.scale),
             ptr(sv.shift), ptr(sv.mean), ptr(sv.invstd), P, Cout, 0, _F(0.0), ptr(slab), cur_stream())
    dgamma, dbeta, ca, cb, cd = coefs
    call("prifit_bn_bwd_finalize", ptr(slab), slab.shape[0], Cout, _D(float(P)), int(st.cfg["training"]), ptr(sv.scale),
         ptr(sv.mean), ptr(sv.invstd), ptr(dgamma), ptr(dbeta), ptr(ca), ptr(cb), ptr(cd), cur_stream())
    return coefs


class SharedMLPFn(torch.autograd.Function):
    """(conv1x1 + BatchNorm + ReLU) x L [+ max over the K samples of each group].

    apply(x, cfg, *tensors) with, per layer, tensors = (W [Cout, Kin], bias, gamma, beta,
    running_mean, running_var); cfg = dict(pool_K, training, eps, momentum[list]) [+ pool_out, a column window the pooled
    output is written into].

    cfg["front"] (a FrontEnd, built with front_end_args) says that layer 0 was computed elsewhere: it then has no GEMM, x is
    its pre-activation (None in mode "norows") and front.slab its column statistics.  Mode "preact": the gradient returned
    for x is the one w.r.t. that pre-activation.  Modes "direct" / "norows" / "gather" (training, fused set-abstraction
    front end): x is plain data and this function returns the gradients of the front end's inputs from layer 0's slots (the
    table at front_end_args), with the BatchNorm + ReLU backward of layer 0 folded into their kernels (no dY of that layer
    is ever written)."""

    @staticmethod
    def forward(ctx, x, cfg, *tensors):
        L = len(tensors) // 6
        front = cfg.get("front")
        mode = "plain" if front is None else front.mode
        # norows: layer 0's pre-activation rows are not stored (x is None); they are re-formed from (idx, U, Vc) by the
        # three kernels that consume them
        if mode == "norows":
            P, dev = front.B * front.S * front.K, front.U.device
        else:
            P, dev = x.shape[0], x.device
        training = cfg["training"]
        layers, prev, aff, cand = [], x, None, None
        for l in range(L):
            W, b, gamma, beta, rmean, rvar = tensors[6 * l:6 * l + 6]
            W = None if (l == 0 and front is not None) else W.contiguous()   # (a front end's layer 0 has no product)
            Cout, Kin = _layer_dims(W, x, front)
            assert W is None or Kin == (front.U.shape[-1] if prev is None else prev.shape[1]), (Kin, l)
            aligned = (W is not None and prev is not None and prev.stride(0) % 4 == 0 and prev.data_ptr() % 16 == 0 and
                       W.data_ptr() % 16 == 0)
            route = _forward_route(l, L, P, Cout, Kin, cfg["pool_K"], training, mode, aligned, aff is not None)
            # slab: the column statistics of Y, written by the launch that produces the layer (training)
            Y, slab, cand = _FWD_ARMS[route.arm](_FwdLayer(P, Cout, Kin, dev, prev, aff, W, b, front, aligned))
            if training:
                # the layer's coefficients [4, C] = scale, shift, mean, invstd, written by prifit_bn_finalize from that slab
                scale, shift, mean, invstd = torch.empty(4, Cout, dtype=torch.float32, device=dev).unbind(0)
                call("prifit_bn_finalize", ptr(slab), slab.shape[0], Cout, _D(float(P)), ptr(gamma), ptr(beta),
                     _F(cfg["eps"]), _F(cfg["momentum"][l]), ptr(rmean), ptr(rvar), ptr(scale), ptr(shift),
                     ptr(mean), ptr(invstd), cur_stream())
            else:
                scale, shift, mean, invstd = _eval_coeffs(gamma, beta, rmean, rvar, cfg["eps"])
            layers.append(_SavedLayer(Y, W, scale, shift, mean, invstd))
            prev, aff = Y, (scale, shift)
        out, arg = _forward_output(cfg, prev, aff, cand, P, dev)
        # (an attribute, not save_for_backward: nothing saved here is an output of this function, so no reference cycle)
        ctx.stack = _SavedStack(layers, x, arg, P, dev, mode, front, tensors[1],
                                {k: v for k, v in cfg.items() if k not in ("front", "pool_out")})
        return out

    @staticmethod
    def backward(ctx, gout):
        st, needs = ctx.stack, ctx.needs_input_grad
        L, P, dev, front = len(st.layers), st.P, st.dev, st.front
        training, pool_K = st.cfg["training"], st.cfg["pool_K"]
        # a pooled stack takes its gradient with any row stride (a column slice of the concatenated multi-scale gradient:
        # every kernel that reads it has a leading dimension) -- no copy; the unpooled paths index rows densely
        if not (pool_K and L > 1 and gout.dim() == 2 and gout.stride(1) == 1 and gout.stride(0) % 4 == 0 and
                gout.data_ptr() % 16 == 0):
            gout = gout.contiguous()
        grads = [None] * (6 * L)
        arena, wslots = _grad_arena(st, needs)
        G_in = gout  # gradient w.r.t. the ReLU output of layer l (or pooled output for the last layer)
        fused_red = None   # the slab of (m1, m2) sums of layer l, where the route of the layer above has left it
        for l in range(L - 1, -1, -1):
            sv, below = st.layers[l], st.layers[l - 1] if l > 0 else None
            Cout, Kin = _layer_dims(sv.W, sv.Y, front)
            pooled = l == L - 1 and bool(pool_K)
            dgamma, dbeta, ca, cb, cd = _bwd_coefficients(st, sv, Cout, pooled, G_in, fused_red)
            route = _backward_route(
                l, L, P, Cout, Kin, pool_K, training, st.mode, needs[2 + 6 * l], needs[0],
                g_dense=G_in.stride(0) == Cout and G_in.data_ptr() % 16 == 0, g_contig=G_in.is_contiguous(),
                below_ld4=l > 0 and below.Y is not None and below.Y.stride(0) % 4 == 0,
                N0=front.N if st.mode == "gather" else 0)
            wo, wn, bo, nb = wslots.get(l, (0, 0, 0, 0))
            Yp, aff_p, stats_p = (below.Y, (below.scale, below.shift), (below.mean, below.invstd)) if l > 0 else (st.x, None, None)
            ly = _BwdLayer(
                P=P, Cout=Cout, Kin=Kin, dev=dev, pooled=pooled, pool_K=pool_K, arg=st.arg, G=G_in, Y=sv.Y, W=sv.W, scale=sv.scale,
                shift=sv.shift, ca=ca, cb=cb, cd=cd, Yp=Yp, aff_p=aff_p, stats_p=stats_p, front=front, bias0=st.bias0,
                dW=arena[wo:wo + wn].view(Cout, Kin) if wn else None, need_dW=needs[2 + 6 * l],
                want_db=needs[3 + 6 * l] and not training)
            G_in, grads[6 * l], fused_red, extra = _ROUTES[route.name](ly, route)
            if needs[3 + 6 * l]:
                # a bias in front of a batch-statistics BatchNorm has zero gradient (the arena's zeros; layer 0 of a fused front
                # end has no arena window); with running statistics it is sum(dY)
                grads[6 * l + 1] = (arena[bo:bo + nb] if training else extra) if l in wslots else zero_pool.zeros(Cout, device=dev)
            grads[6 * l + 2] = dgamma
            grads[6 * l + 3] = dbeta
        # (gather mode: layer 0 took the gather0 route, whose extra is the gradient of Vc, the tensor behind the 6 L layer tensors)
        return (G_in, None) + tuple(grads) + ((extra,) if st.mode == "gather" else ())


class GatherLinearFn(torch.autograd.Function):
    """First layer of a set-abstraction MLP by linearity (upstream models/pointnet_util.py:243-252):
    conv1([feat_j | xyz_j - c_g]) = U_j - Vc_g + bias with U = [feat | xyz] W1^T per point and
    Vc = c W1x^T per centre.  apply(U [B,N,C], Vc [B,S,C], bias, idx [B,S,K], training)
    -> (Y1 [B*S*K, C], column-statistics slab for the BatchNorm that follows)."""

    @staticmethod
    def forward(ctx, U, Vc, bias, idx, training):
        U, Vc, idx = U.contiguous(), Vc.contiguous(), idx.contiguous()
        B, N, C = U.shape
        _, S, K = idx.shape
        assert Vc.shape == (B, S, C) and idx.dtype == torch.int32, (Vc.shape, idx.dtype)
        P = B * S * K
        Y = torch.empty(P, C, dtype=torch.float32, device=U.device)
        rps = _rows_per_slab()
        slab = torch.empty((P + rps - 1) // rps, 2, C, dtype=torch.float32, device=U.device)
        # algorithmic bytes: read U and Vc once, read idx, write the C-wide grouped pre-activations
        with profiler.span("gather_linear", 4.0 * B * (N * C + S * C + S * K + S * K * C)):
            call("prifit_gather_linear_fwd", ptr(U), ptr(Vc), ptr(bias), ptr(idx), B, N, S, K, C, ptr(Y), ptr(slab),
                 cur_stream())
        ctx.save_for_backward(idx)
        ctx.meta = (B, N, S, K, C, training)
        ctx.mark_non_differentiable(slab)
        return Y, slab

    @staticmethod
    def backward(ctx, gY, _gslab):
        (idx,) = ctx.saved_tensors
        B, N, S, K, C, training = ctx.meta
        gY = gY.contiguous()
        dU = zero_pool.zeros(B, N, C, device=gY.device)
        dVc = torch.empty(B, S, C, dtype=torch.float32, device=gY.device)
        call("prifit_gather_linear_bwd", ptr(gY), ptr(idx), B, N, S, K, C, ptr(dU), ptr(dVc), cur_stream())
        db = None
        if ctx.needs_input_grad[2]:
            # a bias in front of a batch-statistics BatchNorm has zero gradient
            db = zero_pool.zeros(C, device=gY.device) if training else gY.sum(dim=0)
        return dU, dVc, db, None, None


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def sa_group_supported(N, nsamples, widths):
    """Limits of prifit_sa_group_linear_fwd (include/prifit_hip.h)."""
    return (N <= 2048 and 1 <= len(nsamples) <= 4 and sum(nsamples) <= 320 and
            all(16 <= c <= 128 and (c & (c - 1)) == 0 for c in widths))


def _sa_group_launch(mode, xyz, new_xyz, feat, feat_first, radii, nsamples, widths, Ws, Us, Vcs, biases,
                     feat_xyz=False, rows=None):
    """One launch: ball query for every radius + the first-layer pre-activations Y_r [B*S*K_r, C_r], their
    BatchNorm column-statistics slabs and the int32 index lists.  rows (gather mode): per radius False = do not store
    Y_r (None is returned for it): index lists and statistics only."""
    import numpy as np

    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    R = len(radii)
    dev = xyz.device
    q = query("prifit_sa_group_queries_per_slab", B, S)
    nslab = B * ((S + q - 1) // q)
    rows = [True] * R if rows is None else list(rows)
    assert mode == 1 or all(rows)
    Ys = [torch.empty(B * S * k, c, dtype=torch.float32, device=dev) if keep else None
          for k, c, keep in zip(nsamples, widths, rows)]
    slabs = [torch.empty(nslab, 2, c, dtype=torch.float32, device=dev) for c in widths]
    idxs = [torch.empty(B, S, k, dtype=torch.int32, device=dev) for k in nsamples]
    r2 = (ctypes.c_float * R)(*[float(np.float32(r ** 2)) for r in radii])  # fp32(radius^2), like ops.ball_query_multi
    ns = (ctypes.c_int * R)(*[int(k) for k in nsamples])
    wd = (ctypes.c_int * R)(*[int(c) for c in widths])
    D = 0 if feat is None else feat.shape[-1]
    # algorithmic bytes (SURVEY.md 8d with the grouped-out term = the C1-wide first-layer rows this launch writes):
    # clouds and centres once, index lists once, rows once, plus the per-point / per-centre projections (gather mode)
    # or the feature table (direct mode)
    work = B * (12.0 * (N + S) + sum(4.0 * S * k * (1 + (c if keep else 0)) for k, c, keep in zip(nsamples, widths, rows)) +
                (sum(4.0 * (N + S) * c for c in widths) if mode == 1 else 4.0 * N * D))
    with profiler.span("sa_group_linear", work):
        call("prifit_sa_group_linear_fwd", ptr(xyz), ptr(new_xyz), B, N, S, R, r2, ns, wd, mode, ptr(feat), D,
             int(feat_first), int(feat_xyz), _ptr_array(Ws) if Ws else None, _ptr_array(Us) if Us else None,
             _ptr_array(Vcs) if Vcs else None, _ptr_array(biases), _ptr_array(Ys), _ptr_array(slabs), _ptr_array(idxs),
             cur_stream())
    return Ys, slabs, idxs


def sa_point_tables(first_convs, feats, xyz, new_xyz, feat_first):
    """U_r [B,N,C_r] (bias folded in) and Vc_r [B,S,C_r] of every radius in one launch (prifit_sa_point_tables)."""
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    D = 0 if feats is None else feats.shape[-1]
    R = len(first_convs)
    Ws = [c.weight.detach().reshape(c.weight.shape[0], -1).contiguous() for c in first_convs]
    bs = [None if c.bias is None else c.bias.detach().contiguous() for c in first_convs]
    Us = [torch.empty(B, N, w.shape[0], dtype=torch.float32, device=xyz.device) for w in Ws]
    Vcs = [torch.empty(B, S, w.shape[0], dtype=torch.float32, device=xyz.device) for w in Ws]
    wd = (ctypes.c_int * R)(*[int(w.shape[0]) for w in Ws])
    call("prifit_sa_point_tables", ptr(xyz.contiguous()), ptr(new_xyz.contiguous()), ptr(None if feats is None else feats.contiguous()),
         B, N, S, D, int(feat_first), R, wd, _ptr_array(Ws), _ptr_array(bs), _ptr_array(Us), _ptr_array(Vcs), cur_stream())
    return Us, Vcs


class SAGroupDirectFn(torch.autograd.Function):
    """Ball query + grouping + first conv of every per-radius MLP in one launch, narrow inputs (upstream
    models/pointnet_util.py:87-107, :127-133 / :243-249, :195-197 / :250-252): y = W_r [feat_j | xyz_j - c] + b_r
    computed from the LDS copy of the cloud, no grouped tensor.  apply(xyz [B,N,3], new_xyz [B,S,3], feat [B,N,D] or
    None (D in 0/3/6, data: no gradient), meta = (radii, nsamples, feat_first, training), W_0, b_0, W_1, b_1, ...)
    with W_r [C_r, D+3] in upstream column order -> (Y_0, slab_0, Y_1, slab_1, ...)."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, feat, meta, *tensors):
        radii, nsamples, feat_first, training = meta
        Ws = [w.contiguous() for w in tensors[0::2]]
        bs = [None if b is None else b.contiguous() for b in tensors[1::2]]
        widths = [w.shape[0] for w in Ws]
        # upstream feeds the coordinates themselves as point features (models/pointnet2_part_seg_msg.py:69-75)
        feat_xyz = feat is not None and feat.shape[-1] == 3 and feat.data_ptr() == xyz.data_ptr()
        Ys, slabs, idxs = _sa_group_launch(0, xyz, new_xyz, feat, feat_first, radii, nsamples, widths, Ws, None, None, bs,
                                           feat_xyz=feat_xyz)
        ctx.save_for_backward(xyz, new_xyz, feat, *idxs)
        ctx.meta = (nsamples, widths, feat_first, training, [b is not None for b in bs])
        out = []
        for y, sl in zip(Ys, slabs):
            out += [y, sl]
        ctx.mark_non_differentiable(*slabs)
        return tuple(out)

    @staticmethod
    def backward(ctx, *gouts):
        xyz, new_xyz, feat = ctx.saved_tensors[:3]
        idxs = ctx.saved_tensors[3:]
        nsamples, widths, feat_first, training, has_bias = ctx.meta
        B, N, _ = xyz.shape
        S = new_xyz.shape[1]
        D = 0 if feat is None else feat.shape[-1]
        grads = []
        for r, (K, C) in enumerate(zip(nsamples, widths)):
            gY = gouts[2 * r]
            dW = db = None
            if gY is not None:
                gY = gY.contiguous()
                P = B * S * K
                nblk = int(max(1, min(1024, (P + 1023) // 1024)))
                part = torch.empty(nblk, C, D + 3, dtype=torch.float32, device=gY.device)
                with profiler.span("sa_first_layer_dw", 4.0 * P * (C + 1)):
                    call("prifit_sa_first_layer_dw", ptr(gY), ptr(idxs[r]), ptr(xyz), ptr(new_xyz), ptr(feat), B, N, S,
                         K, C, D, int(feat_first), nblk, ptr(part), cur_stream())
                dW = slab_sum(part)
                if has_bias[r]:
                    # a bias in front of a batch-statistics BatchNorm has zero gradient
                    db = zero_pool.zeros(C, device=gY.device) if training else gY.sum(dim=0)
            grads += [dW, db]
        return (None, None, None, None) + tuple(grads)


class SAGroupGatherFn(torch.autograd.Function):
    """Same launch for wide inputs, the first layer by linearity: y = U_r[b, j] - Vc_r[b, s] + b_r with
    U = [feat | xyz] W1^T per point and Vc = c W1x^T per centre (see GatherLinearFn).  apply(xyz, new_xyz,
    meta = (radii, nsamples, training), U_0, Vc_0, b_0, U_1, ...) -> (Y_0, slab_0, Y_1, slab_1, ...)."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, meta, *tensors):
        radii, nsamples, training = meta
        Us = [u.contiguous() for u in tensors[0::3]]
        Vcs = [v.contiguous() for v in tensors[1::3]]
        bs = [None if b is None else b.contiguous() for b in tensors[2::3]]
        widths = [u.shape[-1] for u in Us]
        Ys, slabs, idxs = _sa_group_launch(1, xyz, new_xyz, None, True, radii, nsamples, widths, None, Us, Vcs, bs)
        ctx.save_for_backward(*idxs)
        ctx.meta = (xyz.shape[0], xyz.shape[1], new_xyz.shape[1], nsamples, widths, training, [b is not None for b in bs])
        out = []
        for y, sl in zip(Ys, slabs):
            out += [y, sl]
        ctx.mark_non_differentiable(*slabs)
        return tuple(out)

    @staticmethod
    def backward(ctx, *gouts):
        idxs = ctx.saved_tensors
        B, N, S, nsamples, widths, training, has_bias = ctx.meta
        grads = []
        for r, (K, C) in enumerate(zip(nsamples, widths)):
            gY = gouts[2 * r]
            dU = dVc = db = None
            if gY is not None:
                gY = gY.contiguous()
                dU = zero_pool.zeros(B, N, C, device=gY.device)
                dVc = torch.empty(B, S, C, dtype=torch.float32, device=gY.device)
                call("prifit_gather_linear_bwd", ptr(gY), ptr(idxs[r]), B, N, S, K, C, ptr(dU), ptr(dVc), cur_stream())
                if has_bias[r]:
                    db = zero_pool.zeros(C, device=gY.device) if training else gY.sum(dim=0)
            grads += [dU, dVc, db]
        return (None, None, None) + tuple(grads)


def _few_rows_splitk(M, N, K):
    """Split of the reduction for a product with at most one row tile (M <= 128: the per-SAMPLE rows of the DGCNN decoder's
    offset, 24 x 512 x 1024) and a deep K: its N / 128 workgroups would each walk all of K serially (88 us for 25 MFLOP).
    Aim at ~256 workgroups, >= 2 k-tiles of 32 each."""
    if M > 128 or K < 256:
        return 1
    tiles = max(1, (N + 127) // 128)
    return int(max(1, min(256 // tiles, K // 64)))


class LinearFn(torch.autograd.Function):
    """Y = X W^T + b on [P, C] rows (a conv1x1 without BatchNorm: conv2 / extra_conv_emb,
    models/pointnet2_part_seg_msg.py:109,128)."""

    @staticmethod
    def forward(ctx, x, W, b):
        x = x.contiguous()
        W = W.contiguous()
        P, Kin = x.shape
        Cout = W.shape[0]
        sk = _few_rows_splitk(P, Cout, Kin)
        if sk > 1:   # a handful of rows against a deep reduction: a few workgroups would each walk the whole K serially
            Y = zero_pool.zeros(P, Cout, device=x.device)
            gemm(NT, P, Cout, Kin, x, Kin, W, Kin, Y, Cout, bias=b, splitk=sk)
        else:
            Y = torch.empty(P, Cout, dtype=torch.float32, device=x.device)
            gemm(NT, P, Cout, Kin, x, Kin, W, Kin, Y, Cout, bias=b)
        ctx.save_for_backward(x, W)
        return Y

    @staticmethod
    def backward(ctx, gy):
        x, W = ctx.saved_tensors
        gy = gy.contiguous()
        P, Kin = x.shape
        Cout = W.shape[0]
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            sk = _few_rows_splitk(P, Kin, Cout)
            if sk > 1:
                dx = zero_pool.zeros(P, Kin, device=x.device)
                gemm(NN, P, Kin, Cout, gy, Cout, W, Kin, dx, Kin, splitk=sk)
            else:
                dx = torch.empty(P, Kin, dtype=torch.float32, device=x.device)
                gemm(NN, P, Kin, Cout, gy, Cout, W, Kin, dx, Kin)
        if ctx.needs_input_grad[1]:
            dW = _weight_grad(gy, P, Cout, x, Kin, None)
        if ctx.needs_input_grad[2]:
            if Cout % 4 == 0 and gy.data_ptr() % 16 == 0:
                db = torch.empty(Cout, dtype=torch.float32, device=x.device)
                ws = torch.empty(query("prifit_col_sum_workspace", P, Cout), dtype=torch.float32, device=x.device)
                call("prifit_col_sum", ptr(gy), _LL(Cout), P, Cout, ptr(db), ptr(ws), cur_stream())
            else:
                db = gy.sum(dim=0)
        return dx, dW, db


class CrossEntropyFn(torch.autograd.Function):
    """F.cross_entropy(x, target) (mean over the rows; models/pointnet2_part_seg_msg.py:137-144) for x [P, C <= 64] on the GPU, with
    torch's default label semantics: -100 (ignore_index) rows are skipped and left out of the denominator, any other label outside
    [0, C) turns the loss into NaN (torch: a device-side assert):
    one pass forward (+ a one-workgroup mean), one pass backward (prifit_cross_entropy_fwd / _bwd).  torch's nll_loss reduces
    with a single workgroup: 73 + 47 us per step at 49152 x 50."""

    @staticmethod
    def forward(ctx, x, target):
        if x.stride(1) != 1:
            x = x.contiguous()
        target = target.contiguous()
        P, C = x.shape
        lse = torch.empty(P, dtype=torch.float32, device=x.device)
        ws = torch.empty(query("prifit_cross_entropy_workspace"), dtype=torch.float32, device=x.device)
        loss = torch.empty(2, dtype=torch.float32, device=x.device)     # (mean over the kept rows, number of kept rows)
        call("prifit_cross_entropy_fwd", ptr(x), _LL(x.stride(0)), ptr(target), _LL(P), C, ptr(lse), ptr(ws), ptr(loss), cur_stream())
        ctx.save_for_backward(x, target, lse, loss)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        x, target, lse, loss = ctx.saved_tensors
        P, C = x.shape
        dx = torch.empty(P, C, dtype=torch.float32, device=x.device)
        g = g.reshape(1).to(torch.float32).contiguous()
        call("prifit_cross_entropy_bwd", ptr(x), _LL(x.stride(0)), ptr(target), ptr(lse), ptr(g), ptr(loss[1:]), _LL(P), C, ptr(dx),
             _LL(C), cur_stream())
        return dx, None


# SA first layer by linearity, backward as a gather over the points' in-edge lists (0: the walk-and-stage kernel with atomics; A/B, tested)
_GATHER_BWD_CSR = os.environ.get("PRIFIT_GATHER_BWD_CSR", "1") != "0"
# the segmentation loss on the library's kernels (0: torch's F.cross_entropy; A/B arm)
_CE_KERNEL = os.environ.get("PRIFIT_CE_KERNEL", "1") != "0"


def cross_entropy(x, target):
    """F.cross_entropy with the default arguments; rows of up to 64 classes on the GPU go through CrossEntropyFn."""
    if _CE_KERNEL and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.shape[1] <= 64 and target.dim() == 1 and target.dtype == torch.int64:
        return CrossEntropyFn.apply(x, target)
    return torch.nn.functional.cross_entropy(x, target)


class GroupGatherFn(torch.autograd.Function):
    """Grouped rows [B*S*K, ld] = [feat[idx], xyz[idx] - centre, 0-pad] (order 0) or
    [xyz[idx] - centre, feat[idx], 0-pad] (order 1); gradient flows to `feat` only (xyz is data)."""

    @staticmethod
    def forward(ctx, feat, xyz, new_xyz, idx, order, ld_out):
        from . import ops

        out = ops.group_gather(feat, xyz, new_xyz, idx, order=order, ld_out=ld_out)
        ctx.save_for_backward(idx)
        ctx.meta = (feat.shape, order) if feat is not None else None
        return out

    @staticmethod
    def backward(ctx, gout):
        from . import ops

        if ctx.meta is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        (idx,) = ctx.saved_tensors
        (B, N, C), order = ctx.meta
        gout = gout.contiguous()
        dfeat = ops.group_scatter_add(gout, 0 if order == 0 else 3, idx, B, N, C)
        return dfeat, None, None, None, None, None


class ConcatWindowsFn(torch.autograd.Function):
    """The concatenation of column windows that were written IN PLACE into one buffer (SharedMLPFn cfg["pool_out"]): returns the
    buffer as a function of the windows -- no copy forward, column slices of the gradient backward.
    apply(wide [R, sum C_i], *windows) -> [R, sum C_i]."""

    @staticmethod
    def forward(ctx, wide, *windows):
        ctx.widths = [w.shape[1] for w in windows]
        return wide.view_as(wide)

    @staticmethod
    def backward(ctx, g):
        outs, c0 = [], 0
        for wd in ctx.widths:
            outs.append(g[:, c0:c0 + wd])
            c0 += wd
        return (None, *outs)


class FpRowsFn(torch.autograd.Function):
    """[interpolated | points1 | 0-pad] rows of a feature-propagation MLP, [B N, kp], in one launch (prifit_fp_rows).
    apply(points2 [B,S,D2], idx [B,N,3] or None (S == 1), weight, points1 [B,N,D1] or None, kp)."""

    @staticmethod
    def forward(ctx, points2, idx, weight, points1, kp):
        points2 = points2.contiguous()
        B, S, D2 = points2.shape
        N = idx.shape[1] if idx is not None else points1.shape[1]
        D1 = 0 if points1 is None else points1.shape[-1]
        p1 = None if points1 is None else points1.contiguous()
        out = torch.empty(B * N, kp, dtype=torch.float32, device=points2.device)
        call("prifit_fp_rows", ptr(points2), ptr(idx), ptr(weight), ptr(p1), B, N, S, D2, D1, kp, ptr(out), cur_stream())
        ctx.save_for_backward(idx, weight)
        ctx.dims = (B, N, S, D2, D1)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import ops
        idx, weight = ctx.saved_tensors
        B, N, S, D2, D1 = ctx.dims
        g = g.contiguous()
        if idx is None:      # S == 1: the gradient of the broadcast
            dp2 = g[:, :D2].reshape(B, N, D2).sum(dim=1, keepdim=True)
        else:
            dp2 = ops.three_interpolate_bwd(g, 0, idx, weight, B, S, D2)
        dp1 = g[:, D2:D2 + D1].reshape(B, N, D1) if D1 else None
        return dp2, None, None, dp1, None


class ThreeInterpolateFn(torch.autograd.Function):
    """interpolated[(b,n), :] = sum_j w[b,n,j] * points2[b, idx[b,n,j], :]"""

    @staticmethod
    def forward(ctx, points2, idx, weight):
        from . import ops

        points2 = points2.contiguous()
        ctx.save_for_backward(idx, weight)
        ctx.shape = points2.shape
        return ops.three_interpolate(points2, idx, weight)

    @staticmethod
    def backward(ctx, gout):
        from . import ops

        idx, weight = ctx.saved_tensors
        B, S, C = ctx.shape
        gout = gout.contiguous()
        return ops.three_interpolate_bwd(gout, 0, idx, weight, B, S, C), None, None

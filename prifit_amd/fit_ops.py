"""Autograd functions of the fitting path: batched mean-shift clustering, soft membership, weighted
ellipsoid fit and the analytic-chamfer loss terms, on the C-ABI kernels.

Everything is batched over the B shapes of a GPU with fixed-capacity cluster slots (KM per shape,
validity masks instead of the reference's python lists / -1 sentinels), so one forward+backward of
the loss is a fixed sequence of launches with a single host read-back (the cluster-count check of
src/ellipsoid_utils.py:19-27).  Reference sites are cited per function (paths relative to upstream).
"""
import contextlib
import ctypes
import os
import time
from typing import NamedTuple, Optional

import torch

from . import profiler
from . import arena as zero_pool
from ._lib import call, cur_stream, dll, ptr, query, require_cuda
from .nn_ops import EPI_CHORD, EPI_MSBWD, EPI_MSKERNEL, NN, NT, TN, gemm

_LL = ctypes.c_longlong
KM = 32          # cluster slots per shape on the loss path (>= max_num_clusters = 25, src/ellipsoid_utils.py:6); slots_for()
KM_MAX = 64      # ... and up to 64 when the caller raises --max_num_clusters (args_parser.py:48; the reference's own
                 # gaurd_mean_shift accepts 49, src/mean_shift.py:212-226): every kernel takes the slot count at run time
NMS_CAP = 64     # centre ids kept by nms before the cluster-count check
SAMPLE_CAP = 13312  # >= 10000 + KM * 100 surface samples per shape (src/ellipsoid_utils.py:105-106); sample_cap(K)

# The switches of the mean-shift clustering path (A/B arms; which route each one selects: DESIGN 3.8).  The route functions
# below read them at every call; a backward follows the route its forward stored.
# mean-shift backward engine: "hybrid" (default) | "gemm" | "fused", see _dense_bwd_route
BWD_MODE = os.environ.get("PRIFIT_MS_BWD", "hybrid")
# 1: dX from the stream-fed flash-style kernel (prifit_meanshift_dx_streams: no split-K atomics, so dX is bit-reproducible
# from run to run) instead of the dual-source GEMM; measured 456 vs ~440 us per call at B = 24, N = 2048 -> default off
DX_STREAMS = os.environ.get("PRIFIT_MS_DX_STREAMS", "0") != "0"
# stream-K schedule of the dense backward's dZ kernel (grid = resident slots, split query blocks combine through atomics):
# +7 % (488 -> 452 us at B = 24, N = 2048).  (The forward's time is linear in its block count: no such schedule there.)
MS_BALANCED = True
CHORD_SYM = os.environ.get("PRIFIT_CHORD_SYM", "1") != "0"   # symmetric kernel for chord_matrix(X, X)
FUSE_NMS_OWNER = True   # nms: the owner pass (column argmin) in the chord kernel's epilogue (False: a second read of the matrix)
# cluster(): the loss reads the shifted points through `center = new_X[indices]` only, so the mean-shift backward runs
# on those rows alone (MeanShiftRowsFn); 0 = the dense backward of MeanShiftFn + a gather (same numbers; the A/B arm
# and the path of callers that differentiate through the whole of new_X)
ROWS_BWD = os.environ.get("PRIFIT_MS_ROWS", "1") != "0"
# LABELLED EXPERIMENT, default off: the two products of the mean-shift FORWARD on the 16-bit matrix pipe with
# error-compensated operands (csrc/meanshift_split.hip): "bf16x3" | "bf16x6" | "fp16x3".  D = 128, N % 256 == 0, and only
# where the kernel matrix is not kept (the row-sparse backward, i.e. cluster()); anything else takes the fp32 kernels.
# A number measured with it on is not an fp32 number: bench.py labels it (`dtype`, `experiment`) and never reports it as
# the headline.
MS_SPLIT = os.environ.get("PRIFIT_MS_SPLIT", "0")
_SPLIT_MODES = {"bf16x3": 1, "bf16x6": 2, "fp16x3": 3}
split_launches = 0   # updates that took the experiment's kernel (tests assert on it; nothing reads it in the product)
# The first mean-shift update of a trajectory reads the chord matrix the bandwidth step has just written instead of forming
# S = X X^T again (csrc/meanshift_fused.hip, SLOAD: Z_0 = X, one of the 20 N x N x D products of ten updates gone).  0: every
# update takes the standard kernel (A/B arm, tested against this one).
MS_FIRST_CHORD = os.environ.get("PRIFIT_MS_FIRST_CHORD", "1") != "0"
# How the row-sparse backward runs its T iterations (csrc/meanshift_rows.hip, prifit_meanshift_rows_bwd `mode`):
#   2  one workgroup per live row runs all T iterations of that row (nothing crosses workgroups): 2 launches;
#   1  key-tiled iterations as ONE launch over a work queue: 3 launches;  0  one launch per iteration: T + 2 launches.
# "auto": 2 up to 32 cluster slots per shape (the loss path: ~8 live rows per shape, 148 us against 198 / 221 at B = 24), 1 above
# (many live rows: the key-tiled forms read the dictionary once for all rows).  profiles/r06_ms_rows.txt.
MS_ROWS_MODE = os.environ.get("PRIFIT_MS_ROWS_MODE", "auto")
# nms reads ONE BIT per element of its chord matrix once the owner pass is fused into the kernel that forms it: the matrix is
# then never written (csrc/gemm.hip chord_sym_kernel MODE 2: 12.6 MB of mask instead of 403 MB at B = 24, N = 2048).  0: the
# float matrix (A/B arm, tested equal).
NMS_MASK = os.environ.get("PRIFIT_NMS_MASK", "1") != "0"


def slots_for(max_num_clusters):
    """Cluster slots per shape for a cluster-count limit: 32 (the loss path's 25) or 64."""
    m = int(max_num_clusters)
    if m <= KM:
        return KM
    if m <= KM_MAX:
        return KM_MAX
    raise ValueError("max_num_clusters = %d: at most %d clusters per shape are supported (cluster slots, nms keeps %d centres)"
                     % (m, KM_MAX, NMS_CAP))


def sample_cap(K):
    """Surface-sample slots per shape for K cluster slots: 10000 + 100 K (src/ellipsoid_utils.py:105-106), in blocks of 256."""
    return SAMPLE_CAP if K <= KM else (10000 + 100 * K + 255) // 256 * 256


def split_mode(N, D, keep_kernel=False):
    """The mode id of MS_SPLIT for this shape, 0 = the fp32 kernels.  An unknown name raises."""
    if MS_SPLIT in ("0", "", None, False) or keep_kernel:
        return 0
    mode = _SPLIT_MODES[MS_SPLIT]
    return mode if query("prifit_meanshift_split_supported", N, D, mode) else 0


def rows_mode(R):
    return (2 if R <= 32 else 1) if MS_ROWS_MODE == "auto" else int(MS_ROWS_MODE)


def rows_supported(N, D, R):
    return bool(query("prifit_meanshift_rows_supported", N, D, R))


class ShiftIter(NamedTuple):
    """One update of a mean-shift trajectory: the iterate it read, the kernel matrix where it was kept (D = 128: K^T
    [key][query]; other widths: K), O = K X, rowsum(K), the iterate it wrote and the norms ||O / rowsum|| per row."""
    Z: torch.Tensor
    K: Optional[torch.Tensor]
    O: torch.Tensor
    rowsum: torch.Tensor
    Zn: torch.Tensor
    nrm: torch.Tensor


class ShiftRoute(NamedTuple):
    """The forward arm of the first update and of the others ("split" | "fused" | "gemm"; first may be "chord"), and whether
    every ShiftIter carries its kernel matrix (the dense backward reads it)."""
    first: str
    rest: str
    kernel_kept: bool


class DenseBwdRoute(NamedTuple):
    """MeanShiftFn.backward: the engine of one iteration ("hybrid" | "fused" | "gemm_kt" | "gemm"), how its two dX terms are
    formed ("streams" | "dual" | "two" launches; None: the fused engine's own second kernel) and the dZ kernel's schedule."""
    engine: str
    dx: Optional[str]
    balanced: bool


class Shifted(NamedTuple):
    """What _shift hands to nms and _centres: the shifted points (detached) and, on the row-sparse engine, the trajectory
    (no autograd graph yet) or, on the dense engine, the differentiable Z of MeanShiftFn.  The other field is None."""
    Z: torch.Tensor
    traj: Optional[list]
    Zgrad: Optional[torch.Tensor]


class Round(NamedTuple):
    """One bandwidth -> shift -> nms pass (_round) over the shapes `shapes` ([n] int64 indices into the batch, None: all of
    it): their X, what the three steps returned, and `accepted` ([n] bool, set by the retry loop's verdict)."""
    shapes: Optional[torch.Tensor]
    accepted: Optional[torch.Tensor]
    X: torch.Tensor
    bw: torch.Tensor
    shifted: Shifted
    ids: torch.Tensor
    count: torch.Tensor
    labels: torch.Tensor
    used: torch.Tensor


# The route functions launch nothing and allocate nothing: module switches and the library's queries, at every call.
def _chord_route(same, N, M, D, contiguous, aligned):
    """chord_matrix: "sym" (a set against itself in whole 128 x 128 tiles, 32-wide k-steps, dense 16-byte-aligned rows: the
    upper triangle of tiles only, same bits) or "gemm"."""
    return "sym" if CHORD_SYM and same and N == M and N % 128 == 0 and D % 32 == 0 and contiguous and aligned else "gemm"


def _nms_route(N, D, contiguous, aligned):
    """nms: "mask" (the owner pass in the chord kernel's epilogue, one bit per element, the matrix never written),
    "float_owner" (the same epilogue, the float matrix read once) or "float" (the matrix read twice)."""
    if not (FUSE_NMS_OWNER and _chord_route(True, N, N, D, contiguous, aligned) == "sym"):
        return "float"
    return "mask" if NMS_MASK else "float_owner"


def _forward_route(N, D, keep_kernel, has_chord):
    """mean_shift_trajectory: D = 128 takes the flash-style kernel (csrc/meanshift_fused.hip) or the MS_SPLIT experiment's,
    other widths the GEMM chain; the first update reads the caller's chord matrix where nothing else asks for S = X X^T."""
    rest = "gemm" if D != 128 else "split" if split_mode(N, D, keep_kernel) else "fused"
    chord = (rest == "fused" and has_chord and not keep_kernel and MS_FIRST_CHORD and
             query("prifit_meanshift_fused_first_supported", N, D))
    return ShiftRoute("chord" if chord else rest, rest, bool(keep_kernel))


def _dense_bwd_route(N, D):
    """MeanShiftFn.backward, 4 N^2 D products per iteration in every case but "fused":
      "hybrid" (default): flash-style dZ kernel (gS = (gO X^T + g_rowsum) * K / b^2 in registers, dZ = gS X, gS^T
                streamed out once) + ONE dual-source MFMA GEMM for dX += gS^T Z + K^T gO (N % 32 == 0);
      "gemm_kt" (PRIFIT_MS_BWD=gemm, and every N the kernels above do not take): MFMA GEMM chain on the saved K^T (gS^T by a
                GEMM epilogue, dZ by a TN GEMM, the same dual-source GEMM or two products): +0.6 ms / step;
      "fused":  flash-style kernels that re-form gS in registers for dX too (5 products, no gS in HBM; N % 4 == 0): +4.5 ms;
      "gemm":   the GEMM chain on K, widths other than 128."""
    if D != 128:
        return DenseBwdRoute("gemm", "two", False)
    if BWD_MODE == "fused" and N % 4 == 0:
        return DenseBwdRoute("fused", None, False)
    if BWD_MODE == "hybrid" and N % 32 == 0:
        return DenseBwdRoute("hybrid", "streams" if DX_STREAMS and N % 64 == 0 else "dual", bool(MS_BALANCED))
    return DenseBwdRoute("gemm_kt", "dual" if N % 32 == 0 else "two", False)


def _shift_engine(N, D, slots):
    """Who differentiates the shift: "rows" (trajectory now, MeanShiftRowsFn on the kept rows later) or "dense" (MeanShiftFn)."""
    return "rows" if ROWS_BWD and rows_supported(N, D, slots) else "dense"


def _bgemm(layout, M, N, K, A, lda, B_, ldb, C, ldc, batch, sA, sB, sC, **kw):
    gemm(layout, M, N, K, A, lda, B_, ldb, C, ldc, batch=batch, sA=sA, sB=sB, sC=sC, **kw)


def _skinny_splitk(M, N, K, batch):
    """Split of the reduction for [M, N] = [M, K] [K, N] products with few, deep output tiles (mean-shift
    backward: 16 x 1 x 24 tiles of 64 k-tiles on 256 CUs): aim at >= 6 workgroups per CU so that the two resident
    ones per CU stay busy to the end.  At B=24, N=2048, D=128 (384 tiles) with the tile loads truly in flight: NN 278 (sk 1),
    232 (sk 2), 243 (sk 4), 270 us (sk 8); TN 286 / 237 / 249 / 278 -> aim at ~768 workgroups (sk = 2)."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128) * batch
    sk = 1
    while tiles * sk < 768 and (K // 32) // (2 * sk) >= 8:
        sk *= 2
    return sk


def chord_matrix(A, B_, owner_key=None):
    """2 - 2 A B^T for unit rows (src/mean_shift.py:154,168,185).  A [B,N,D], B_ [B,M,D] -> [B,N,M].
    owner_key: a one-element list; when the symmetric kernel runs it receives the [B,N] int64 keys of nms's owner pass
    (argmin over each column in the low word), computed in the kernel's epilogue."""
    Bt, N, D = A.shape
    M = B_.shape[1]
    out = torch.empty(Bt, N, M, dtype=torch.float32, device=A.device)
    if _chord_route(A.data_ptr() == B_.data_ptr(), N, M, D, A.is_contiguous(), A.data_ptr() % 16 == 0) == "sym":
        keys = None
        if owner_key is not None:
            keys = torch.full((Bt, N), -1, dtype=torch.int64, device=A.device)   # all bits set: the atomic-min identity
            owner_key.append(keys)
        # work = the products the kernel really does: the T (T + 1) / 2 tiles (128 x 128) on and above the diagonal
        nt = N // 128
        with profiler.span(profiler.tag("chord_sym", N, D, Bt), 2.0 * Bt * (nt * (nt + 1) // 2) * 128 * 128 * D):
            call("prifit_chord_sym_f32", ptr(A), _LL(D), _LL(N * D), ptr(out), _LL(N), _LL(N * N), N, D, Bt, ptr(keys), cur_stream())
        return out
    _bgemm(NT, N, M, D, A, D, B_, D, out, M, Bt, N * D, M * D, N * M, epi=EPI_CHORD)
    return out


def compute_bandwidth(X, quantile, num_samples=None, rows=None, keep_chord=None):
    """src/mean_shift.py:138-160, batched: X [B,N,D] (unit rows) -> bw [B].

    num_samples < N (upstream :148-151: a random row subset, the default of `clustering(X)`, num_samples=1000): the
    statistic is taken over `rows` [B, num_samples] (int64 row indices; hidden randomness made an explicit input like
    the other ones) or, when omitted, over a fresh random subset per shape, as upstream.  num_samples > N: upstream's
    slice keeps all N rows and K = int(quantile * num_samples) (:155) all the same -- and so here (topk raises when
    K exceeds the row length; so does this).
    keep_chord: a list; when the statistic is taken over ALL rows, the chord matrix [B,N,N] = 2 - 2 X X^T is appended to it
    (mean_shift_trajectory(chord=...) reads it in the first update)."""
    Bt, N, D = X.shape
    ns = N if num_samples is None else int(num_samples)
    full = ns >= N
    if ns < N:
        if rows is None:
            rows = torch.stack([torch.randperm(N, device=X.device)[:ns] for _ in range(Bt)])
        rows = rows.to(X.device).long()
        if rows.shape != (Bt, ns):
            raise ValueError("bandwidth rows must be [B, num_samples]")
        X = torch.gather(X, 1, rows.unsqueeze(-1).expand(-1, -1, D)).contiguous()
        N = ns
    dist = chord_matrix(X, X)
    if keep_chord is not None and full:
        keep_chord.append(dist)
    k = int(quantile * ns)
    if k < 1:
        raise ValueError("quantile * num_samples < 1: torch.topk(k=0) upstream")
    if k > N:
        raise ValueError("k = int(quantile * num_samples) = %d exceeds the %d rows (torch.topk raises upstream)" % (k, N))
    kth = torch.empty(Bt * N, dtype=torch.float32, device=X.device)
    with profiler.span("kth_smallest", 4.0 * Bt * N * N):
        call("prifit_kth_smallest_rows", ptr(dist), _LL(Bt * N), N, k, ptr(kth), cur_stream())
    bw = torch.empty(Bt, dtype=torch.float32, device=X.device)
    call("prifit_bandwidth_from_kth", ptr(kth), Bt, N, ptr(bw), cur_stream())     # mean(sqrt(clamp(kth, 1e-6))) per shape
    return bw


class Normalize2Fn(torch.autograd.Function):
    """F.normalize(F.normalize(x, dim=-1), dim=-1) on [..., D <= 256] rows in one kernel (convex_loss.py:41,57)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        D = x.shape[-1]
        y = torch.empty_like(x)
        call("prifit_row_normalize2_fwd", ptr(x), D, _LL(x.numel() // D), ctypes.c_float(1e-12), ptr(y), cur_stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        D = x.shape[-1]
        gx = torch.empty_like(x)
        call("prifit_row_normalize2_bwd", ptr(x), ptr(g.contiguous()), D, _LL(x.numel() // D), ctypes.c_float(1e-12), ptr(gx),
             cur_stream())
        return gx


def _update_split(X, bw, it, Kmat, cut):
    """The MS_SPLIT experiment's two products, then the fp32 normalisation.  cut: (the dictionary's planes, the mode id)."""
    global split_launches
    Bt, N, D = X.shape
    split_launches += 1
    with profiler.span("ms_split_fwd[%s]" % MS_SPLIT, 4.0 * Bt * N * N * D):
        call("prifit_meanshift_split_fwd", ptr(it.Z), ptr(cut[0]), ptr(bw), Bt, N, D, cut[1], ptr(it.O), ptr(it.rowsum), cur_stream())
    call("prifit_meanshift_update_fwd", ptr(it.O), ptr(it.rowsum), ptr(it.Z), D, _LL(Bt * N), ptr(it.Zn), ptr(it.nrm),
         cur_stream())


def _update_first_chord(X, bw, it, Kmat, chord):
    """Z_0 = X: S = X X^T = 1 - chord / 2 is in HBM already; ONE matrix product (O = K X) + a read of the chord matrix."""
    Bt, N, D = X.shape
    with profiler.span("ms_first_fwd", 2.0 * Bt * N * N * D):
        call("prifit_meanshift_fused_first_fwd", ptr(X), ptr(chord), _LL(N), _LL(N * N), ptr(bw), Bt, N, D, ptr(it.Zn), ptr(it.O),
             ptr(it.rowsum), ptr(it.nrm), cur_stream())


def _update_fused(X, bw, it, Kmat, _):
    Bt, N, D = X.shape
    with profiler.span("ms_fused_fwd", 4.0 * Bt * N * N * D):
        call("prifit_meanshift_fused_fwd", ptr(it.Z), ptr(X), ptr(bw), Bt, N, D, ptr(Kmat), _LL(N),
             _LL(N * N), ptr(it.Zn), ptr(it.O), ptr(it.rowsum), ptr(it.nrm), cur_stream())


def _update_gemm(X, bw, it, Kmat, _):
    Bt, N, D = X.shape
    _bgemm(NT, N, N, D, it.Z, D, X, D, Kmat, N, Bt, N * D, N * D, N * N, epi=EPI_MSKERNEL, epi_scalar=bw)
    _bgemm(NN, N, D, N, Kmat, N, X, D, it.O, D, Bt, N * N, N * D, N * D, a_rowsum=it.rowsum)  # K X, rowsum(K)
    call("prifit_meanshift_update_fwd", ptr(it.O), ptr(it.rowsum), ptr(it.Z), D, _LL(Bt * N), ptr(it.Zn), ptr(it.nrm),
         cur_stream())


_UPDATES = {"split": _update_split, "chord": _update_first_chord, "fused": _update_fused, "gemm": _update_gemm}


def mean_shift_trajectory(X, bw, iterations, keep_kernel, chord=None):
    """`iterations` updates of src/mean_shift.py:61-82 (gaussian kernel, delta = 1) for all shapes at once, no autograd.
    X [B,N,D] unit rows (contiguous), bw [B].  Returns (Z_final, one ShiftIter per iteration);
    keep_kernel=False: the N x N kernel matrix is not kept (D = 128: never written -- prifit_meanshift_fused_fwd with
    KT = NULL; other widths: one scratch matrix for the GEMM chain).
    chord: the chord matrix 2 - 2 X X^T [B,N,N] of THIS X when the caller has it (compute_bandwidth(keep_chord=...)): the
    first update then reads it instead of forming X X^T again (prifit_meanshift_fused_first_fwd; D = 128, N % 64 == 0)."""
    Bt, N, D = X.shape
    dev = X.device
    route = _forward_route(N, D, keep_kernel, chord is not None)
    # Z_0 = X.clone() (:60): no kernel writes its input iterate, so the first one IS X (a 25 MB copy saved; with no iteration
    # the caller gets its own tensor)
    Z = X if iterations > 0 else X.clone()
    saved = []
    scratch = None
    aux = {"chord": chord}
    if route.rest == "split":   # the dictionary is the same in every iteration (:65): cut once
        split = _SPLIT_MODES[MS_SPLIT]
        cut = torch.empty(query("prifit_meanshift_split_workspace", Bt, N, D, split), dtype=torch.uint8, device=dev)
        call("prifit_meanshift_split_prep", ptr(X), Bt, N, D, split, ptr(cut), cur_stream())
        aux["split"] = (cut, split)
    for _ in range(iterations):
        Kmat = None
        if route.kernel_kept:
            Kmat = torch.empty(Bt, N, N, dtype=torch.float32, device=dev)  # fused: K^T [key][query]; else K
        elif route.rest == "gemm":
            scratch = Kmat = scratch if scratch is not None else torch.empty(Bt, N, N, dtype=torch.float32, device=dev)
        it = ShiftIter(Z, Kmat if route.kernel_kept else None, torch.empty(Bt, N, D, dtype=torch.float32, device=dev),
                       torch.empty(Bt, N, dtype=torch.float32, device=dev), torch.empty_like(Z),
                       torch.empty(Bt, N, dtype=torch.float32, device=dev))
        arm = route.rest if saved else route.first
        _UPDATES[arm](X, bw, it, Kmat, aux.get(arm))
        saved.append(it)
        Z = it.Zn
    return Z, saved


class MeanShiftRowsFn(torch.autograd.Function):
    """centres = new_X[ids] of src/mean_shift.py:44-46 as a function of the embedding X, given the trajectory
    `mean_shift_trajectory(X, bw, T, keep_kernel=False)` already computed (nms needed its end point to choose ids).

    Row i of an iterate depends on row i of the previous one alone (the dictionary is the fixed X, :65), so the gradient
    that enters through the gathered rows stays on those rows in every iteration: the backward is R x N x D products per
    iteration (prifit_meanshift_rows_bwd) instead of the dense N x N x D ones -- the same numbers, the dense form's other
    rows multiply exact zeros.  apply(X, bw, ids [B,R] int64, nrows [B] int32 or None, traj) -> [B,R,D]."""

    @staticmethod
    def forward(ctx, X, bw, ids, nrows, traj):
        X = X.contiguous()
        Bt, N, D = X.shape
        R = ids.shape[1]
        if not rows_supported(N, D, R):
            raise ValueError("row-sparse mean-shift backward: D in {32, 64, 128}, R <= 32 (got D=%d, R=%d)" % (D, R))
        ids = ids.to(device=X.device, dtype=torch.int64).clamp(0, N - 1).contiguous()
        Zf = traj[-1].Zn if traj else X
        out = torch.gather(Zf, 1, ids.unsqueeze(-1).expand(-1, -1, D))
        # (attributes, not save_for_backward: nothing saved here is an output of this function, so no reference cycle)
        ctx.traj, ctx.X, ctx.bw, ctx.ids, ctx.mode = traj, X, bw, ids, rows_mode(R)
        ctx.nrows = None if nrows is None else nrows.to(device=X.device, dtype=torch.int32).contiguous()
        return out

    @staticmethod
    def backward(ctx, g):
        X, bw, ids, nrows, traj = ctx.X, ctx.bw, ctx.ids, ctx.nrows, ctx.traj
        if traj is None:
            raise RuntimeError("MeanShiftRowsFn: backward a second time -- the saved mean-shift trajectory is released by the "
                               "first backward (retain_graph is not supported here)")
        ctx.traj = None
        Bt, N, D = X.shape
        R = ids.shape[1]
        g = g.contiguous()
        gX = zero_pool.zeros(Bt, N, D, device=X.device)
        T = len(traj)
        ws = torch.empty(query("prifit_meanshift_rows_bwd_workspace", Bt, N, D, R, T), dtype=torch.float32, device=X.device)
        arr = lambda field: (ctypes.c_void_p * max(T, 1))(*[getattr(it, field).data_ptr() for it in traj])
        # HBM-bound: per iteration the dictionary is read once (4 B per element); dX read-modified-written once in all (8 B)
        with profiler.span("ms_rows_bwd", 4.0 * Bt * N * D * (T + 2)):
            call("prifit_meanshift_rows_bwd", ptr(X), ptr(bw), Bt, N, D, T, arr("Z"), arr("Zn"), arr("O"), arr("rowsum"), arr("nrm"),
                 ptr(ids), ptr(nrows), R, ptr(g), ptr(ws), ptr(gX), ctx.mode, cur_stream())
        return gX, None, None, None, None


class MeanShiftFn(torch.autograd.Function):
    """src/mean_shift.py:50-84 (gaussian kernel, delta = 1), all shapes at once.

    forward: Z_0 = X; per iteration K = exp(clamp((Z X^T - 1)/b^2)) (MFMA GEMM with the kernel transform in
    its epilogue), O = K X (second GEMM, which also emits the row sums of K while staging it),
    Z <- normalize(O/rowsum).
    backward: four GEMMs per iteration (dK through the saved K in the epilogue, dZ, and two dX terms)."""

    @staticmethod
    def forward(ctx, X, bw, iterations):
        X = X.contiguous()
        Z, saved = mean_shift_trajectory(X, bw, iterations, keep_kernel=True)
        # save_for_backward (not a python attribute): the last Zn IS the output, and an attribute would close a
        # reference cycle output -> grad_fn -> ctx -> output that only the cyclic GC frees (4 GB of K per step)
        ctx.save_for_backward(X, bw, *[t for it in saved for t in it])
        ctx.route = _dense_bwd_route(X.shape[1], X.shape[2])
        return Z

    @staticmethod
    def backward(ctx, g):
        X, bw = ctx.saved_tensors[:2]
        flat = ctx.saved_tensors[2:]
        n = len(ShiftIter._fields)
        saved = [ShiftIter(*flat[i:i + n]) for i in range(0, len(flat), n)]
        route = ctx.route
        Bt, N, D = X.shape
        dev = X.device
        g = g.contiguous()
        gX = zero_pool.zeros(Bt, N, D, device=dev)
        gS = None if route.engine == "fused" else torch.empty(Bt, N, N, dtype=torch.float32, device=dev)
        gO = torch.empty(Bt, N, D, dtype=torch.float32, device=dev)
        grs = torch.empty(Bt, N, dtype=torch.float32, device=dev)
        sk = _skinny_splitk(N, D, N, Bt)
        for it in reversed(saved):
            call("prifit_meanshift_update_bwd", ptr(g), ptr(it.Zn), ptr(it.nrm), ptr(it.O), ptr(it.rowsum), D, Bt, N, ptr(gO),
                 _LL(N * D), ptr(grs), cur_stream())
            if route.balanced:
                gZ = zero_pool.zeros(Bt, N, D, device=dev)   # stream-K schedule: split query blocks add their halves
            else:
                chain = sk > 1 and route.engine in ("gemm_kt", "gemm")    # split-K products accumulate
                gZ = (torch.zeros if chain else torch.empty)(Bt, N, D, dtype=torch.float32, device=dev)
            _DENSE_BWD[route.engine](route, X, bw, it, gO, grs, gS, gZ, gX, sk)
            g = gZ
        gX += g  # Z_0 = X.clone()
        return gX, None, None


def _dx_dual(span, X, it, gO, gS, gX):
    """dX += gS^T Z + K^T gO as one product over 2N (one epilogue of float atomics instead of two)."""
    Bt, N, D = X.shape
    with profiler.span(span, 4.0 * Bt * N * D * N):
        call("prifit_gemm_dual_nn_f32", N, D, N, N, ptr(gS), ptr(it.K), _LL(N), _LL(N * N), ptr(it.Z), ptr(gO),
             _LL(D), _LL(N * D), ptr(gX), _LL(D), _LL(N * D), Bt, _skinny_splitk(N, D, 2 * N, Bt), 1, cur_stream())


def _bwd_hybrid(route, X, bw, it, gO, grs, gS, gZ, gX, sk):
    """Flash-style dZ kernel (products 1 + 2, streams gS^T out) + both dX terms from the two streams."""
    Bt, N, D = X.shape
    with profiler.span("ms_fused_bwd", 4.0 * Bt * N * N * D):
        call("prifit_meanshift_fused_bwd_dz", ptr(gO), _LL(N * D), ptr(X), ptr(bw), ptr(grs), ptr(it.K),
             _LL(N), _LL(N * N), ptr(gS), Bt, N, D, ptr(gZ), int(route.balanced), cur_stream())
    if route.dx == "streams":
        with profiler.span("ms_fused_dx", 4.0 * Bt * N * D * N):
            call("prifit_meanshift_dx_streams", ptr(gO), ptr(it.Z), ptr(gS), ptr(it.K), _LL(N), _LL(N * N), Bt, N, D,
                 ptr(gX), cur_stream())
    else:
        _dx_dual("gemm_dual_nn", X, it, gO, gS, gX)


def _bwd_fused(route, X, bw, it, gO, grs, gS, gZ, gX, sk):
    Bt, N, D = X.shape
    with profiler.span("ms_fused_bwd", 10.0 * Bt * N * N * D):
        call("prifit_meanshift_fused_bwd_dz", ptr(gO), _LL(N * D), ptr(X), ptr(bw), ptr(grs), ptr(it.K),
             _LL(N), _LL(N * N), None, Bt, N, D, ptr(gZ), 0, cur_stream())           # dZ  = gS X
        call("prifit_meanshift_fused_bwd_dx", ptr(gO), ptr(it.Z), ptr(X), ptr(bw), ptr(grs), ptr(it.K),
             _LL(N), _LL(N * N), Bt, N, D, ptr(gX), cur_stream())                    # dX += gS^T Z + K^T gO


def _bwd_gemm_kt(route, X, bw, it, gO, grs, gS, gZ, gX, sk):
    """The transposed (key-major) orientation of the saved K^T: gS^T = (X gO^T + 1 g_rowsum^T) * K^T / b^2 where the clamp is
    inactive."""
    Bt, N, D = X.shape
    sM, sV = N * N, N * D
    _bgemm(NT, N, N, D, X, D, gO, D, gS, N, Bt, sV, sV, sM, epi=EPI_MSBWD, epi_scalar=bw, aux=it.K,
           ld_aux=N, s_aux=sM, bias=grs, bias_stride=N)
    _bgemm(TN, N, D, N, gS, N, X, D, gZ, D, Bt, sM, sV, sV, splitk=sk)                       # dZ  = gS X
    if route.dx == "dual":
        _dx_dual("gemm_nn_bn128", X, it, gO, gS, gX)
    else:
        _bgemm(NN, N, D, N, gS, N, it.Z, D, gX, D, Bt, sM, sV, sV, accumulate=True, splitk=sk)      # dX += gS^T Z
        _bgemm(NN, N, D, N, it.K, N, gO, D, gX, D, Bt, sM, sV, sV, accumulate=True, splitk=sk)      # dX += K^T gO


def _bwd_gemm(route, X, bw, it, gO, grs, gS, gZ, gX, sk):
    """dL/dS = (gO X^T + g_rowsum 1^T) * K / b^2 where the clamp is inactive."""
    Bt, N, D = X.shape
    sM, sV = N * N, N * D
    _bgemm(NT, N, N, D, gO, D, X, D, gS, N, Bt, sV, sV, sM, epi=EPI_MSBWD, epi_scalar=bw, aux=it.K,
           ld_aux=N, s_aux=sM, row_add=grs)
    _bgemm(NN, N, D, N, gS, N, X, D, gZ, D, Bt, sM, sV, sV, splitk=sk)                       # dZ = dS X
    _bgemm(TN, N, D, N, gS, N, it.Z, D, gX, D, Bt, sM, sV, sV, accumulate=True, splitk=sk)      # dX += dS^T Z
    _bgemm(TN, N, D, N, it.K, N, gO, D, gX, D, Bt, sM, sV, sV, accumulate=True, splitk=sk)      # dX += K^T dO


_DENSE_BWD = {"hybrid": _bwd_hybrid, "fused": _bwd_fused, "gemm_kt": _bwd_gemm_kt, "gemm": _bwd_gemm}


def nms(Z, bw):
    """src/mean_shift.py:162-202 as called at :44 (centers = X = shifted points), batched.
    Returns ids [B,NMS_CAP] (ascending kept centre ids), count [B], labels [B,N], used [B,NMS_CAP]."""
    Bt, N, D = Z.shape
    dev = Z.device
    i32 = dict(dtype=torch.int32, device=dev)
    owner = torch.empty(Bt, N, **i32)
    # (counts | flags | used in ONE allocation: prifit_nms zeroes them with one memset when they are adjacent)
    zeroed = torch.empty(2 * Bt * N + Bt * NMS_CAP, **i32)
    counts, flags = zeroed[:Bt * N].view(Bt, N), zeroed[Bt * N:2 * Bt * N].view(Bt, N)
    used = zeroed[2 * Bt * N:].view(Bt, NMS_CAP)
    ids = torch.empty(Bt, NMS_CAP, **i32)
    count = torch.empty(Bt, **i32)
    labels = torch.empty(Bt, N, **i32)
    route = _nms_route(N, D, Z.is_contiguous(), Z.data_ptr() % 16 == 0)
    if route == "mask":
        okey = torch.full((Bt, N), -1, dtype=torch.int64, device=dev)             # all bits set: the atomic-min identity
        mask = torch.empty(Bt, N, N // 32, **i32)
        nt = N // 128
        with profiler.span(profiler.tag("chord_sym_mask", N, D, Bt), 2.0 * Bt * (nt * (nt + 1) // 2) * 128 * 128 * D):
            call("prifit_chord_sym_mask", ptr(Z), _LL(D), _LL(N * D), ptr(bw), ptr(mask), N, D, Bt, ptr(okey), cur_stream())
        with profiler.span("nms", Bt * N * N / 8.0):
            call("prifit_nms_mask", ptr(mask), ptr(Z), Bt, N, D, NMS_CAP, ptr(okey), ptr(owner), ptr(counts), ptr(flags), ptr(ids),
                 ptr(count), ptr(labels), ptr(used), cur_stream())
        return ids, count, labels, used
    keys = [] if route == "float_owner" else None
    dist = chord_matrix(Z, Z, keys)      # (float_owner: the symmetric kernel, which leaves the owner keys)
    okey = keys[0] if keys else None
    # the chord matrix is read once (neighbour pick) when the owner pass ran in the chord kernel's epilogue, else twice
    with profiler.span("nms", (4.0 if okey is not None else 8.0) * Bt * N * N):
        call("prifit_nms", ptr(dist), ptr(Z), ptr(bw), Bt, N, D, NMS_CAP, ptr(okey), ptr(owner), ptr(counts), ptr(flags), ptr(ids),
             ptr(count), ptr(labels), ptr(used), cur_stream())
    return ids, count, labels, used


def nms_pair(C, X, bw):
    """src/mean_shift.py:162-202 with centres that are not the points: C [B,N,D], X [B,N,D] (the same row count -- upstream's
    broadcast at :191 needs it).  Same outputs as nms()."""
    Bt, N, D = X.shape
    assert C.shape == X.shape, "nms(centers, X, b): upstream needs centers.shape[0] == X.shape[0] (src/mean_shift.py:191)"
    dev = X.device
    C, X = C.contiguous(), X.contiguous()
    dist_xc = chord_matrix(X, C)      # row j: point j against every centre
    dist_cc = chord_matrix(C, C)
    i32 = dict(dtype=torch.int32, device=dev)
    owner, counts, flags, labels = (torch.empty(Bt, N, **i32) for _ in range(4))
    ids, used = (torch.empty(Bt, NMS_CAP, **i32) for _ in range(2))
    count = torch.empty(Bt, **i32)
    with profiler.span("nms", 8.0 * Bt * N * N):
        call("prifit_nms_pair", ptr(dist_xc), ptr(dist_cc), ptr(C), ptr(X), ptr(bw), Bt, N, D, NMS_CAP, ptr(owner), ptr(counts),
             ptr(flags), ptr(ids), ptr(count), ptr(labels), ptr(used), cur_stream())
    return ids, count, labels, used


class MembershipFn(torch.autograd.Function):
    """src/mean_shift.py:230-247, batched: centres [B,KM,D], X [B,N,D] -> W [B,N,KM] (0 for k >= count)."""

    @staticmethod
    def forward(ctx, centres, X, bw, count):
        centres, X = centres.contiguous(), X.contiguous()
        Bt, N, D = X.shape
        K = centres.shape[1]
        dev = X.device
        dots = torch.empty(Bt, N, K, dtype=torch.float32, device=dev)
        _bgemm(NT, N, K, D, X, D, centres, D, dots, K, Bt, N * D, K * D, N * K)
        gmax = torch.empty(Bt, dtype=torch.float32, device=dev)    # global max over the live (point, cluster) pairs, detached (:242)
        if K % 4 == 0:
            ws = torch.empty(query("prifit_membership_gmax_workspace", Bt), dtype=torch.float32, device=dev)
            call("prifit_membership_gmax", ptr(dots), ptr(bw), ptr(count), Bt, N, K, ptr(gmax), ptr(ws), cur_stream())
        else:   # (a slot count that is not a multiple of 4: never on the loss path, KM = 32)
            live = torch.arange(K, device=dev).view(1, 1, K) < count.view(Bt, 1, 1)
            gmax = dots.masked_fill(~live, float("-inf")).amax(dim=(1, 2)) / (bw * bw)
        W = torch.empty_like(dots)
        with profiler.span("membership", 8.0 * Bt * N * K):
            call("prifit_membership_fwd", ptr(dots), ptr(bw), ptr(gmax), ptr(count), Bt, N, K, ptr(W), cur_stream())
        ctx.save_for_backward(centres, X, bw, count, dots, gmax, W)
        return W

    @staticmethod
    def backward(ctx, gW):
        centres, X, bw, count, dots, gmax, W = ctx.saved_tensors
        Bt, N, D = X.shape
        K = centres.shape[1]
        gW = gW.contiguous()
        gd = torch.empty_like(dots)
        with profiler.span("membership", 16.0 * Bt * N * K):
            call("prifit_membership_bwd", ptr(gW), ptr(W), ptr(dots), ptr(bw), ptr(gmax), ptr(count), Bt, N, K, ptr(gd),
                 cur_stream())
        # dcentres = gd^T X: one 32 x 128 output tile per shape over N = 2048 rows -- split the reduction so that
        # more than 24 workgroups run (242 us -> tens of us at B = 24)
        sk = _skinny_splitk(K, D, N, Bt)
        gc = (zero_pool.zeros_like if sk > 1 else torch.empty_like)(centres)
        _bgemm(TN, K, D, N, gd, K, X, D, gc, D, Bt, N * K, N * D, K * D, splitk=sk)
        gX = torch.empty_like(X)
        _bgemm(NN, N, D, K, gd, K, centres, D, gX, D, Bt, N * K, K * D, N * D)  # dX = gd centres
        return gc, gX, None, None


class EllipsoidFitFn(torch.autograd.Function):
    """src/ellipsoid_fitting.py:19-69,104-141, one workgroup per (shape, cluster).
    points [B,N,3], W [B,N,KM], count [B], rnd [3,3] | [B,KM,3,3] -> r [B,KM,3], V [B,KM,3,3], c [B,KM,3], valid."""

    @staticmethod
    def forward(ctx, points, W, count, rnd, canonical):
        points, W, rnd = points.contiguous(), W.contiguous(), rnd.contiguous()
        Bt, N, _ = points.shape
        K = W.shape[2]
        dev = points.device
        sb, sk = (0, 0) if rnd.dim() == 2 else (K * 9, 9)
        r = torch.empty(Bt, K, 3, dtype=torch.float32, device=dev)
        V = torch.empty(Bt, K, 3, 3, dtype=torch.float32, device=dev)
        c = torch.empty(Bt, K, 3, dtype=torch.float32, device=dev)
        valid = torch.empty(Bt, K, dtype=torch.int32, device=dev)
        state = zero_pool.zeros(Bt, K, dll().prifit_fit_state_floats(), device=dev)
        with profiler.span("ellipsoid_fit", 3.0 * 16.0 * Bt * N * K):   # (12 + 4) N bytes, three passes, per cluster slot
            call("prifit_ellipsoid_fit_fwd", ptr(points), ptr(W), ptr(count), ptr(rnd), _LL(sb), _LL(sk), int(canonical),
                 Bt, N, K, ptr(r), ptr(V), ptr(c), ptr(valid), ptr(state), cur_stream())
        ctx.save_for_backward(points, W, count, rnd, state, valid)
        ctx.strides = (sb, sk)
        ctx.mark_non_differentiable(valid)
        return r, V, c, valid

    @staticmethod
    def backward(ctx, g_r, g_V, g_c, _gvalid):
        points, W, count, rnd, state, valid = ctx.saved_tensors
        Bt, N, _ = points.shape
        K = W.shape[2]
        sb, sk = ctx.strides
        gW = torch.empty_like(W)
        with profiler.span("ellipsoid_fit", 20.0 * Bt * N * K):
            call("prifit_ellipsoid_fit_bwd", ptr(points), ptr(W), ptr(count), ptr(valid), ptr(rnd), _LL(sb), _LL(sk),
                 ptr(state), ptr(g_r.contiguous()), ptr(g_V.contiguous()), ptr(g_c.contiguous()), Bt, N, K, ptr(gW),
                 cur_stream())
        return None, gW, None, None, None


class SdfLossFn(torch.autograd.Function):
    """sum over target points of (min_k |sdf_k|)^2 per shape (convex_loss.py:313-328, src/utils.py:410-411)."""

    @staticmethod
    def forward(ctx, targets, r, V, c, valid, cuboid=False):
        targets, r, V, c = targets.contiguous(), r.contiguous(), V.contiguous(), c.contiguous()
        Bt, M, _ = targets.shape
        K = r.shape[1]
        dev = targets.device
        arg = torch.empty(Bt, M, dtype=torch.int32, device=dev)
        fval = torch.empty(Bt, M, dtype=torch.float32, device=dev)
        s = torch.empty(Bt, dtype=torch.float32, device=dev)
        ctx.prim = "cuboid" if cuboid else "ellipsoid"   # convex_loss.py:473-502 vs :313-328
        with profiler.span("sdf", 20.0 * Bt * M):
            call("prifit_%s_sdf_fwd" % ctx.prim, ptr(targets), Bt, M, ptr(r), ptr(V), ptr(c), ptr(valid), K, ptr(arg),
                 ptr(fval), ptr(s), cur_stream())
        ctx.save_for_backward(targets, r, V, c, arg)
        return s

    @staticmethod
    def backward(ctx, gs):
        targets, r, V, c, arg = ctx.saved_tensors
        Bt, M, _ = targets.shape
        K = r.shape[1]
        g_r, g_V, g_c = zero_pool.zeros_like(r), zero_pool.zeros_like(V), zero_pool.zeros_like(c)
        with profiler.span("sdf", 16.0 * Bt * M):
            call("prifit_%s_sdf_bwd" % ctx.prim, ptr(targets), Bt, M, ptr(r), ptr(V), ptr(c), ptr(arg), ptr(gs.contiguous()),
                 K, ptr(g_r), ptr(g_V), ptr(g_c), cur_stream())
        return None, g_r, g_V, g_c, None, None


class SampleNNLossFn(torch.autograd.Function):
    """Surface samples (area-proportional budget, Fibonacci (U,V) table) -> exact nearest target -> sum of
    squared distances per shape (src/ellipsoid_utils.py:76-130, src/sample_ellipsoid.py:45-63,
    src/utils.py:413-416).  Returns (sum_d2 [B], total [B] number of samples)."""

    @staticmethod
    def forward(ctx, r, V, c, valid, targets, cuboid=False):
        targets, r, V, c = targets.contiguous(), r.contiguous(), V.contiguous(), c.contiguous()
        Bt, M, _ = targets.shape
        K = r.shape[1]
        dev = targets.device
        n = torch.empty(Bt, K, dtype=torch.int32, device=dev)
        off = torch.empty(Bt, K + 1, dtype=torch.int32, device=dev)
        # cuboid: src/ellipsoid_utils.py:162-214 + src/sample_ellipsoid.py:65-96 on the build's box-surface table
        ctx.pre = "prifit_cuboid_sample" if cuboid else "prifit_sample"
        cap = ctx.cap = sample_cap(K)
        call(ctx.pre + "_budget", ptr(r), ptr(valid), Bt, K, cap, ptr(n), ptr(off), cur_stream())
        nn_idx = torch.empty(Bt, cap, dtype=torch.int32, device=dev)
        s = torch.empty(Bt, dtype=torch.float32, device=dev)
        ws = torch.empty(query("prifit_sample_nn_workspace_floats", Bt, cap), dtype=torch.float32, device=dev)
        # VALU-bound exact search: every surface sample (budget ~10^4 per shape, src/ellipsoid_utils.py:105) against every
        # target, 8 flop per pair (3 sub, 3 fma-equivalents, compare + select)
        with profiler.span("sample_nn", 8.0 * Bt * 10000.0 * M):
            call(ctx.pre + "_nn_fwd", ptr(r), ptr(V), ptr(c), ptr(n), ptr(off), Bt, K, ptr(targets), M,
                 cap, ptr(nn_idx), ptr(s), ptr(ws), cur_stream())
        total = off[:, K].clone()
        ctx.save_for_backward(r, V, c, n, off, targets, nn_idx)
        ctx.mark_non_differentiable(total)
        return s, total

    @staticmethod
    def backward(ctx, gs, _gt):
        r, V, c, n, off, targets, nn_idx = ctx.saved_tensors
        Bt, M, _ = targets.shape
        K = r.shape[1]
        g_r, g_V, g_c = zero_pool.zeros_like(r), zero_pool.zeros_like(V), zero_pool.zeros_like(c)
        # HBM: per sample its (U, V) entry, its nearest target (gathered) and index; parameters from LDS
        with profiler.span("sample_nn_bwd", Bt * 10000.0 * (8.0 + 12.0 + 4.0)):
            call(ctx.pre + "_nn_bwd", ptr(r), ptr(V), ptr(c), ptr(n), ptr(off), Bt, K, ptr(targets), M, ctx.cap,
                 ptr(nn_idx), ptr(gs.contiguous()), ptr(g_r), ptr(g_V), ptr(g_c), cur_stream())
        return g_r, g_V, g_c, None, None, None


class ChamferNNFn(torch.autograd.Function):
    """Exact nearest neighbour between two batched point sets: a [B,NA,3] queries, b [B,NB,3] targets, na / nb [B] int32
    counts of live rows (None = all) -> (d2 [B,NA] squared distance to the nearest live target, idx [B,NA] int32 its index,
    the lowest on ties; -1 and d2 = 0 on dead rows).  What the [N,M] matrix + min of src/utils.py:284-292, :311-319, :338-353
    and the KD-tree query + gather of :368-374, :413-416 compute, without the matrix.  Gradients flow to a and b."""

    @staticmethod
    def forward(ctx, a, b, na=None, nb=None):
        require_cuda(a, b, na, nb)
        a, b = a.contiguous(), b.contiguous()
        if a.dtype != torch.float32 or b.dtype != torch.float32:
            raise TypeError("ChamferNNFn: float32 point sets expected, got %s / %s" % (a.dtype, b.dtype))
        if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3 or a.shape[0] != b.shape[0]:
            raise ValueError("ChamferNNFn: a [B,NA,3] and b [B,NB,3] expected, got %s / %s" % (tuple(a.shape), tuple(b.shape)))
        Bt, NA, NB = a.shape[0], a.shape[1], b.shape[1]
        dev = a.device
        na = None if na is None else na.to(torch.int32).contiguous()
        nb = None if nb is None else nb.to(torch.int32).contiguous()
        d2 = torch.empty(Bt, NA, dtype=torch.float32, device=dev)
        idx = torch.empty(Bt, NA, dtype=torch.int32, device=dev)
        nws = query("prifit_chamfer_nn_workspace_floats", Bt, NA, NB)
        ws = torch.empty(nws, dtype=torch.float32, device=dev) if nws else None
        # VALU-bound exact search, 11 operations per pair (3 sub, 3 mul, 2 add, compare + 2 selects)
        with profiler.span("chamfer_nn", 11.0 * Bt * NA * NB):
            call("prifit_chamfer_nn_fwd", ptr(a), ptr(b), ptr(na), ptr(nb), Bt, NA, NB, ptr(d2), ptr(idx), ptr(ws),
                 cur_stream())
        ctx.save_for_backward(a, b, idx, *[t for t in (na, nb) if t is not None])
        ctx.has = (na is not None, nb is not None)
        ctx.mark_non_differentiable(idx)
        return d2, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _gidx):
        a, b, idx = ctx.saved_tensors[:3]
        rest = list(ctx.saved_tensors[3:])
        na = rest.pop(0) if ctx.has[0] else None
        nb = rest.pop(0) if ctx.has[1] else None
        Bt, NA, NB = a.shape[0], a.shape[1], b.shape[1]
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        # HBM: per query its index, gradient, row and gathered target in, its row out; the target side re-reads idx + ga per wave
        with profiler.span("chamfer_nn_bwd", Bt * (NA * (4.0 + 4.0 + 12.0 + 12.0 + 12.0) + NB * 12.0)):
            call("prifit_chamfer_nn_bwd", ptr(a), ptr(b), ptr(na), ptr(nb), Bt, NA, NB, ptr(idx), ptr(g.contiguous()), ptr(ga),
                 ptr(gb), 0, cur_stream())
        return ga, gb, None, None


class ChamferCombineFn(torch.autograd.Function):
    """The last step of analytic_chamfer_distance (src/utils.py:417-426): per shape (d2_sum / max(total, 1) + sdf_sum / M) / 2,
    mean over the shapes with at least one valid primitive -> (loss [], dist_st [B], sdf_ts [B]); one launch each way
    instead of ~25 elementwise / reduce launches over B numbers."""

    @staticmethod
    def forward(ctx, d2_sum, total, sdf_sum, valid, M):
        Bt, K = valid.shape
        dev = d2_sum.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        part = torch.empty(2, Bt, dtype=torch.float32, device=dev)
        coef = torch.empty(2 * Bt + 1, dtype=torch.float32, device=dev)
        call("prifit_chamfer_combine_fwd", ptr(d2_sum.contiguous()), ptr(total.contiguous()), ptr(sdf_sum.contiguous()),
             ptr(valid.contiguous()), Bt, K, int(M), ptr(loss), ptr(part), ptr(coef), cur_stream())
        ctx.save_for_backward(coef)
        ctx.Bt = Bt
        ctx.mark_non_differentiable(part)
        return loss.view(()), part

    @staticmethod
    def backward(ctx, g, _gpart):
        (coef,) = ctx.saved_tensors
        g_d2 = torch.empty(ctx.Bt, dtype=torch.float32, device=coef.device)
        g_sdf = torch.empty_like(g_d2)
        call("prifit_chamfer_combine_bwd", ptr(g.contiguous()), ptr(coef), ctx.Bt, ptr(g_d2), ptr(g_sdf), cur_stream())
        return g_d2, None, g_sdf, None, None


# ------------------------------------------------------------------------------------------------
# Speculative clustering.  guard_mean_shift (src/mean_shift.py) reads the number of clusters on the host to
# decide whether to retry with a doubled quantile; that read-back drains the GPU queue in the middle of a step.
# Inside `with speculative() as spec:` cluster() assumes the first round is accepted (it is, except on
# degenerate embeddings), copies the verdict to pinned host memory asynchronously and carries on; the caller
# checks `spec.ok()` once everything is enqueued and, if the assumption was wrong, discards the step and re-runs
# it outside the context (train_step.SpeculativeRunner does exactly that) - results are the reference's either way.
# ------------------------------------------------------------------------------------------------
spec_wait_s = 0.0    # host seconds spent blocked in _Speculation.ok() since import (bench.py: enqueue time without the wait)


class _Speculation:
    def __init__(self):
        self.checks = []

    def ok(self):
        global spec_wait_s
        good = True
        t0 = time.perf_counter()
        for ev, flag in self.checks:
            ev.synchronize()
            good = good and int(flag[0]) == 0
        spec_wait_s += time.perf_counter() - t0
        self.checks.clear()
        return good


_spec = None
_flag_pool, _flag_next = [], 0


def _pinned_flag():
    global _flag_next
    if len(_flag_pool) < 16:
        _flag_pool.append(torch.zeros(1, dtype=torch.int32).pin_memory())
        return _flag_pool[-1]
    _flag_next = (_flag_next + 1) % len(_flag_pool)
    return _flag_pool[_flag_next]


@contextlib.contextmanager
def speculative():
    global _spec
    prev, _spec = _spec, _Speculation()
    try:
        yield _spec
    finally:
        _spec = prev


def _shift(X, bw, iterations, km=KM, chord=None):
    """The shifted points for nms + what the centre gather needs afterwards (Shifted)."""
    Bt, N, D = X.shape
    if _shift_engine(N, D, km) == "rows":
        with torch.no_grad():
            Xc = X.detach().contiguous()
            Z, traj = mean_shift_trajectory(Xc, bw, iterations, keep_kernel=False, chord=chord)
        return Shifted(Z, traj, None)
    Z = MeanShiftFn.apply(X, bw, iterations)
    return Shifted(Z.detach(), None, Z)


def _centres(X, bw, shifted, ids, count):
    """center = new_X[indices] (src/mean_shift.py:46), [B,KM,D], differentiable w.r.t. X."""
    if shifted.traj is not None:
        return MeanShiftRowsFn.apply(X, bw, ids, count, shifted.traj)      # (the kernels clamp the live count to the KM slots)
    return torch.gather(shifted.Zgrad, 1, ids.unsqueeze(-1).expand(-1, -1, X.shape[2]))


def _round(X, q, iterations, km, num_samples, rows, shapes):
    """compute_bandwidth (which keeps its chord matrix for the first update) -> _shift -> nms on X, the shapes `shapes`
    of the batch, at quantile q -> Round (not yet judged: `accepted` is None)."""
    keep = []
    with torch.no_grad():
        bw = compute_bandwidth(X, q, num_samples, rows, keep_chord=keep)
    shifted = _shift(X, bw, iterations, km, chord=keep[0] if keep else None)
    del keep
    with torch.no_grad():
        ids, count, labels, used = nms(shifted.Z, bw)
    return Round(shapes, None, X, bw, shifted, ids, count, labels, used)


def _cluster_speculative(X, quantile, iterations, max_num_clusters, num_samples=None, bandwidth_rows=None):
    Bt, N, D = X.shape
    km = slots_for(max_num_clusters)
    rnd = _round(X, quantile, iterations, km, num_samples, bandwidth_rows, None)
    with torch.no_grad():
        bad = torch.empty(1, dtype=torch.int32, device=X.device)
        call("prifit_cluster_verdict", ptr(rnd.count), ptr(rnd.used), Bt, NMS_CAP, int(max_num_clusters), km, None, ptr(bad),
             cur_stream())
        flag = _pinned_flag()
        flag.copy_(bad, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        _spec.checks.append((ev, flag))
    return {"bw": rnd.bw, "ids": rnd.ids[:, :km].long(), "count": rnd.count, "labels": rnd.labels.long(),
            "quantile": [quantile] * Bt, "Z": rnd.shifted.Z, "_shifted": rnd.shifted}


def _pin_representatives(res, center_ids):
    """Harness hook: use the given point of every mode as its representative.  Which member of a collapsed
    mode nms keeps is last-bit noise in the reference itself, but `center = new_X[indices]` (src/mean_shift.py:46) is a
    differentiable gather, so the gradient of everything downstream enters the mean-shift trajectory of exactly that
    point (d loss / d X moves by ~10 % with the pick, oracle/make_golden.py:golden_selfsup_step).  A gradient
    comparison against the reference therefore passes the reference's picks: [B,KM] int64, -1 padded, in the
    reference's (ascending id) order.  The partition must be the one nms found (checked, on the host)."""
    Z = res["Z"].detach()
    Bt, N, D = Z.shape
    km = res["ids"].shape[1]
    ids = torch.as_tensor(center_ids).to(Z.device).long()
    if ids.shape[1] < km:
        ids = torch.cat([ids, ids.new_full((Bt, km - ids.shape[1]), -1)], 1)
    ids = ids[:, :km]
    k = (ids >= 0).sum(1)
    if not torch.equal(k.cpu(), res["count"].long().cpu()):
        raise RuntimeError("center_ids: %s representatives for %s clusters" % (k.tolist(), res["count"].tolist()))
    ids = ids.clamp(min=0)
    cen = torch.gather(Z, 1, ids.unsqueeze(-1).expand(-1, -1, D))
    dots = torch.bmm(cen, Z.transpose(1, 2))                                    # labels = argmax_k centres_k . x (ms:199-201)
    dots.masked_fill_(torch.arange(km, device=Z.device).view(1, km, 1) >= k.view(Bt, 1, 1), float("-inf"))
    labels = dots.argmax(dim=1)
    for b in range(Bt):
        pairs = torch.unique(torch.stack([res["labels"][b], labels[b]], 1), dim=0)
        if pairs.shape[0] != int(k[b]):
            raise RuntimeError("center_ids describe another partition than nms found (shape %d)" % b)
    res["ids"], res["labels"] = ids, labels


def cluster(X, quantile, iterations, max_num_clusters, center_ids=None, num_samples=None, bandwidth_rows=None):
    """src/ellipsoid_utils.py:9-73 batched: mean-shift + nms with the quantile-doubling retry
    (one host read-back per round).  X [B,N,D] unit rows.
    Returns dict(Z, bw, ids [B,KM], count [B], labels [B,N] int64, centres [B,KM,D], W [B,N,KM], quantile list)."""
    Bt, N, D = X.shape
    dev = X.device
    if _spec is not None:
        res = _cluster_speculative(X, quantile, iterations, max_num_clusters, num_samples, bandwidth_rows)
        if center_ids is not None:
            _pin_representatives(res, center_ids)
        res["centres"] = _centres(X, res["bw"], res.pop("_shifted"), res["ids"], res["count"])
        res["W"] = MembershipFn.apply(res["centres"], X, res["bw"], res["count"])
        return res
    km = slots_for(max_num_clusters)
    res = {"bw": torch.empty(Bt, device=dev), "ids": torch.zeros(Bt, km, dtype=torch.int64, device=dev),
           "count": torch.zeros(Bt, dtype=torch.int32, device=dev),
           "labels": torch.zeros(Bt, N, dtype=torch.int64, device=dev), "quantile": [quantile] * Bt}
    pending = torch.arange(Bt, device=dev)
    q = quantile
    rounds = []   # the Rounds that accepted at least one shape
    while pending.numel():
        Xp = X if pending.numel() == Bt else X.index_select(0, pending)
        rows_p = bandwidth_rows
        if rows_p is not None and pending.numel() != Bt:
            with torch.no_grad():
                rows_p = rows_p.to(dev).index_select(0, pending)
        rnd = _round(Xp, q, iterations, km, num_samples, rows_p, pending)
        with torch.no_grad():
            nb = rnd.count.shape[0]
            both = torch.empty(2, nb, dtype=torch.int32, device=dev)
            both[0].copy_(rnd.count)
            scratch = torch.empty(1, dtype=torch.int32, device=dev)
            call("prifit_cluster_verdict", ptr(rnd.count), ptr(rnd.used), nb, NMS_CAP, int(max_num_clusters), km, ptr(both[1]),
                 ptr(scratch), cur_stream())
            host = both.cpu()  # the one host sync of the round (guard_mean_shift's check)
        ok = host[1] <= max_num_clusters
        if bool((ok & (host[0] > km)).any()):
            raise RuntimeError("more than %d kept centres with <= %d distinct labels: unsupported corner" % (km, max_num_clusters))
        okd = ok.to(dev)
        sel = pending[okd]
        if sel.numel():
            res["bw"][sel] = rnd.bw[okd]
            res["ids"][sel] = rnd.ids[okd][:, :km].long()
            res["count"][sel] = rnd.count[okd]
            res["labels"][sel] = rnd.labels[okd].long()
            rounds.append(rnd._replace(accepted=okd))
            for i in sel.tolist():
                res["quantile"][i] = q
        pending = pending[~okd]
        q *= 2
    whole = len(rounds) == 1 and bool(rounds[0].accepted.all())    # one round accepted every shape: its tensors ARE the batch's
    if whole:
        res["Z"] = rounds[0].shifted.Z
    else:
        res["Z"] = torch.zeros(Bt, N, D, device=dev).index_copy(0, torch.cat([r.shapes[r.accepted] for r in rounds]),
                                                                torch.cat([r.shifted.Z[r.accepted] for r in rounds]))
    if center_ids is not None:
        _pin_representatives(res, center_ids)
    # center = new_X[indices] (:46), per round: a shape's centres come from the trajectory of the round that accepted it
    if whole:
        centres = _centres(rounds[0].X, rounds[0].bw, rounds[0].shifted, res["ids"], res["count"])
    else:
        centres = torch.zeros(Bt, km, D, device=dev)
        for r in rounds:
            live = torch.where(r.accepted, res["count"].index_select(0, r.shapes),
                               torch.zeros_like(res["count"].index_select(0, r.shapes)))
            cen = _centres(r.X, r.bw, r.shifted, res["ids"].index_select(0, r.shapes), live)
            centres = centres.index_copy(0, r.shapes[r.accepted], cen[r.accepted])
    res["centres"] = centres
    res["W"] = MembershipFn.apply(centres, X, res["bw"], res["count"])
    return res

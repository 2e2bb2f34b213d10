"""Thin functional wrappers over the C ABI: index / grouping ops of the PointNet++ stack.

Every function takes and returns CUDA(HIP) tensors in channels-last layout and launches on the
current PyTorch stream.  Reference sites are cited per function (paths relative to upstream).
"""
import ctypes

import numpy as np
import torch

from . import _lib, profiler
from . import arena as zero_pool
from ._lib import call, cf, cur_stream, ptr, require_cuda


class SampledAhead:
    """Farthest-point samples of one set-abstraction level computed ahead of the step that uses them (`sample_ahead`):
    pass it where a module takes `fps_start`.  `farthest_point_sample` then only makes the consuming stream wait for the
    event and hands the stored (indices, coordinates) out -- the same numbers the in-line launch would produce."""
    __slots__ = ("idx", "new_xyz", "event", "npoint", "keep", "consumed", "stream")

    def __init__(self, idx, new_xyz, event, keep=(), stream=None):
        self.idx, self.new_xyz, self.event, self.npoint = idx, new_xyz, event, idx.shape[1]
        self.keep = keep   # the side stream's inputs: not back to the allocator before the consumer has waited for the event
        self.consumed = False   # set by farthest_point_sample once the consuming stream waits for the event
        # the stream whose allocator pool idx / new_xyz came from (the current stream when sample_ahead ran): a finaliser
        # can run anywhere -- inside `with torch.cuda.stream(side)`, on another thread -- so "current stream" at that
        # moment is not the pool's stream
        self.stream = stream

    def __del__(self):
        # dropped WITHOUT having been consumed: the side stream may still be writing idx / new_xyz, whose memory goes back to
        # the consuming stream's allocator pool right now -- make that stream wait for the chain (a device-side wait: no
        # host sync in a finaliser).  Once consumed, the consumer's wait_event already orders every later reuse.
        if self.consumed:
            return
        try:
            if not self.event.query():
                (self.stream or torch.cuda.current_stream(self.idx.device)).wait_event(self.event)
        except Exception:   # interpreter shutdown
            pass


_ahead_streams = {}


def sample_ahead(xyz, npoints, starts=None):
    """The farthest-point-sampling CHAIN of a batch (level l samples npoints[l] of level l - 1's samples; it depends on
    the coordinates alone) on a side stream, for the NEXT step's batch while the current step runs: the search is a
    serial loop of `npoint` rounds on one workgroup per shape (24 of 256 CUs busy for 0.32 ms of a 24 ms step), so on
    the step's own stream the rest of the chip waits for it.  xyz [B,N,3] channels-last; returns one SampledAhead per
    level.  The side stream first waits for everything already enqueued on the current stream (the batch's producers)."""
    require_cuda(xyz)
    dev = xyz.device
    side = _ahead_streams.get(dev)
    if side is None:
        side = _ahead_streams[dev] = torch.cuda.Stream(dev)
    xyz = cf(xyz)
    B = xyz.shape[0]
    starts = list(starts) if starts is not None else [None] * len(npoints)
    n_in = [xyz.shape[1]] + [int(n) for n in npoints[:-1]]
    starts = [torch.randint(0, n, (B,), dtype=torch.long, device=dev) if s is None
              else s.to(device=dev, dtype=torch.int64).contiguous() for s, n in zip(starts, n_in)]
    # outputs are allocated on the CONSUMING stream's pool: they are freed there, after the wait for the event
    outs = [(torch.empty(B, int(n), dtype=torch.int64, device=dev), torch.empty(B, int(n), 3, dtype=torch.float32, device=dev))
            for n in npoints]
    consumer = torch.cuda.current_stream(dev)
    side.wait_stream(consumer)
    with torch.cuda.stream(side):
        cur = xyz
        for (idx, nx), st, n in zip(outs, starts, npoints):
            call("prifit_fps", ptr(cur), B, cur.shape[1], int(n), ptr(st), ptr(idx), ptr(nx), cur_stream())
            cur = nx
        ev = torch.cuda.Event()
        ev.record(side)
    return [SampledAhead(idx, nx, ev, keep=(xyz, starts), stream=consumer) for idx, nx in outs]


def farthest_point_sample(xyz, npoint, start_idx=None, return_xyz=False):
    """models/pointnet_util.py:63-84.  xyz [B,N,3] -> int64 [B,npoint] (bit-exact for a given
    start_idx; when None a random start is drawn like the reference's torch.randint at :75).
    `start_idx` may be a SampledAhead (the samples of this level, launched earlier by `sample_ahead`)."""
    require_cuda(xyz)
    if isinstance(start_idx, SampledAhead):
        if start_idx.npoint != npoint or start_idx.idx.shape[0] != xyz.shape[0]:
            raise ValueError("SampledAhead holds %s samples, the module asks for [%d, %d]"
                             % (tuple(start_idx.idx.shape), xyz.shape[0], npoint))
        torch.cuda.current_stream(xyz.device).wait_event(start_idx.event)
        start_idx.consumed = True
        return (start_idx.idx, start_idx.new_xyz) if return_xyz else start_idx.idx
    xyz = cf(xyz)
    B, N, _ = xyz.shape
    if start_idx is None:
        start_idx = torch.randint(0, N, (B,), dtype=torch.long, device=xyz.device)
    start_idx = start_idx.to(device=xyz.device, dtype=torch.int64).contiguous()
    out = torch.empty(B, npoint, dtype=torch.int64, device=xyz.device)
    new_xyz = torch.empty(B, npoint, 3, dtype=torch.float32, device=xyz.device) if return_xyz else None
    call("prifit_fps", ptr(xyz), B, N, npoint, ptr(start_idx), ptr(out), ptr(new_xyz), cur_stream())
    return (out, new_xyz) if return_xyz else out


def ball_query_multi(radius_list, nsample_list, xyz, new_xyz, idx64=False):
    """models/pointnet_util.py:87-107 for several radii in one pass.  Returns a list of
    [B,S,nsample] index tensors (int32 internally, int64 for the reference-surface API)."""
    require_cuda(xyz, new_xyz)
    xyz, new_xyz = cf(xyz), cf(new_xyz)
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    outs = []
    for lo in range(0, len(radius_list), 4):
        rs = radius_list[lo:lo + 4]
        ks = nsample_list[lo:lo + 4]
        R = len(rs)
        o = [torch.empty(B, S, k, dtype=torch.int64 if idx64 else torch.int32, device=xyz.device) for k in ks]
        # the reference compares fp32 distances with the python double radius**2, i.e. fp32(radius**2)
        r2 = (ctypes.c_float * R)(*[float(np.float32(r ** 2)) for r in rs])
        ns = (ctypes.c_int * R)(*[int(k) for k in ks])
        op = (ctypes.c_void_p * R)(*[t.data_ptr() for t in o])
        # algorithmic bytes: clouds read once, indices written once
        with profiler.span("ball_query", B * (12.0 * (N + S) + sum(4.0 * S * k for k in ks))):
            call("prifit_ball_query", ptr(xyz), ptr(new_xyz), B, N, S, R, r2, ns, op, int(idx64), cur_stream())
        outs += o
    return outs


def three_nn(xyz1, xyz2, want_dist=False):
    """models/pointnet_util.py:291-297: 3 nearest of xyz2 for every xyz1 point + normalised
    inverse-distance weights.  Returns (idx int32 [B,N,3], weight [B,N,3][, dist [B,N,3]])."""
    require_cuda(xyz1, xyz2)
    xyz1, xyz2 = cf(xyz1), cf(xyz2)
    B, N, _ = xyz1.shape
    S = xyz2.shape[1]
    idx = torch.empty(B, N, 3, dtype=torch.int32, device=xyz1.device)
    w = torch.empty(B, N, 3, dtype=torch.float32, device=xyz1.device)
    d = torch.empty(B, N, 3, dtype=torch.float32, device=xyz1.device) if want_dist else None
    call("prifit_three_nn", ptr(xyz1), ptr(xyz2), B, N, S, ptr(idx), ptr(d), ptr(w), cur_stream())
    return (idx, w, d) if want_dist else (idx, w)


def square_distance(src, dst):
    """models/pointnet_util.py:19-40 (expanded form, bitwise)."""
    require_cuda(src, dst)
    src, dst = cf(src), cf(dst)
    B, S, _ = src.shape
    N = dst.shape[1]
    out = torch.empty(B, S, N, dtype=torch.float32, device=src.device)
    call("prifit_square_distance", ptr(src), ptr(dst), B, S, N, ptr(out), cur_stream())
    return out


def group_gather(feat, xyz, new_xyz, idx, order=0, ld_out=None):
    """models/pointnet_util.py:243-249 / :127-133.  Returns [B*S*K, ld_out] rows
    [feat, rel_xyz, 0..] (order 0, MSG) or [rel_xyz, feat, 0..] (order 1, SSG)."""
    require_cuda(xyz, new_xyz, idx)
    xyz, new_xyz = cf(xyz), cf(new_xyz)
    feat = None if feat is None else cf(feat)
    idx = idx.contiguous()
    assert idx.dtype == torch.int32
    B, N, _ = xyz.shape
    _, S, K = idx.shape
    C = 0 if feat is None else feat.shape[-1]
    if ld_out is None:
        ld_out = (C + 3 + 3) // 4 * 4
    out = torch.empty(B * S * K, ld_out, dtype=torch.float32, device=xyz.device)
    # algorithmic bytes: feature table read once + grouped rows [S*K, C+3] written once
    with profiler.span("group_gather", B * (4.0 * N * C + 4.0 * S * K * (C + 3))):
        call("prifit_group_gather", ptr(feat), ptr(xyz), ptr(new_xyz), ptr(idx), B, N, S, K, C, order, ld_out,
             ptr(out), cur_stream())
    return out


def group_scatter_add(gout, col0, idx, B, N, C, dfeat=None):
    """Backward of the feature columns of group_gather: returns dfeat [B,N,C]."""
    _, S, K = idx.shape
    if dfeat is None:
        dfeat = zero_pool.zeros(B, N, C, device=gout.device)
    call("prifit_group_scatter_add", ptr(gout), gout.stride(0), col0, ptr(idx), B, N, S, K, C, ptr(dfeat),
         cur_stream())
    return dfeat


def three_interpolate(points2, idx, weight, out=None, col0=0):
    """models/pointnet_util.py:298.  points2 [B,S,C] -> out[(b,n), col0:col0+C]."""
    B, S, C = points2.shape
    N = idx.shape[1]
    if out is None:
        out = torch.empty(B * N, C, dtype=torch.float32, device=points2.device)
    call("prifit_three_interpolate", ptr(points2), ptr(idx), ptr(weight), B, N, S, C, out.stride(0), col0,
         ptr(out), cur_stream())
    return out


def three_interpolate_bwd(gout, col0, idx, weight, B, S, C):
    N = idx.shape[1]
    dp2 = zero_pool.zeros(B, S, C, device=gout.device)
    call("prifit_three_interpolate_bwd", ptr(gout), gout.stride(0), col0, ptr(idx), ptr(weight), B, N, S, C,
         ptr(dp2), cur_stream())
    return dp2


def affine_points(src, affine, subset=None, want_cl=False, want_cf=False, out_cl=None):
    """One per-shape affine map of the first three channels, the channels-first copy and the subset gather in ONE launch
    (csrc/augment.hip; pretrain_partseg_shapenet.py:321-351: the provider.py augmentations, `.transpose(2, 1)`, and
    `chamfer_points[:, :, choice]`).  src [B,M,C] float32 channels-last, 3 <= C <= 8; affine [B,12] float32 (A row-major, then t;
    out = p . A + t) on the host or on the device; subset: indices into [0, M) -- numpy / a host tensor is checked here and
    uploaded TOGETHER with a host `affine` in one copy, a device tensor is taken as it is (the caller's contract).
    -> (cl [B,M,C] | None, cf [B,C,M] | None, sub [B,C,len(subset)] | None); out_cl: the tensor to write cl into (may be `src`:
    in place; implies want_cl)."""
    require_cuda(src)
    if src.dtype != torch.float32 or src.dim() != 3 or not src.is_contiguous():
        raise ValueError("affine_points: src must be a contiguous float32 [B,M,C] tensor")
    B, M, C = src.shape
    dev = src.device
    if out_cl is not None:
        want_cl = True
        if out_cl.shape != src.shape or out_cl.dtype != torch.float32 or not out_cl.is_cuda or not out_cl.is_contiguous():
            raise ValueError("affine_points: out_cl must be a contiguous float32 device tensor of src's shape")
    if not (want_cl or want_cf or subset is not None):
        raise ValueError("affine_points: no output requested")
    n_sub, sub_dev = 0, None
    if subset is not None and not (torch.is_tensor(subset) and subset.is_cuda):
        subset = np.ascontiguousarray(subset.numpy() if torch.is_tensor(subset) else subset)
        if subset.ndim != 1 or subset.size == 0 or subset.dtype.kind not in "iu":
            raise ValueError("affine_points: subset must be a non-empty 1-d integer array")
        if int(subset.min()) < 0 or int(subset.max()) >= M:
            raise IndexError("affine_points: subset index outside [0, %d)" % M)
        n_sub = subset.size
    elif subset is not None:
        if subset.dim() != 1 or subset.numel() == 0:
            raise ValueError("affine_points: subset must be a non-empty 1-d integer tensor")
        n_sub = subset.numel()
        sub_dev = subset.to(torch.int32).contiguous()
    if torch.is_tensor(affine) and affine.is_cuda:
        aff_dev = cf(affine)
        if n_sub and sub_dev is None:
            sub_dev = torch.from_numpy(subset.astype(np.int32)).to(dev)
    else:
        aff = np.ascontiguousarray(affine.numpy() if torch.is_tensor(affine) else affine, dtype=np.float32)
        if n_sub and sub_dev is None:
            # matrices and indices in one buffer of 32-bit words: one host-to-device copy
            words = np.empty(B * 12 + n_sub, dtype=np.float32)
            words[:B * 12] = aff.reshape(-1)
            words[B * 12:].view(np.int32)[:] = subset
            up = torch.from_numpy(words).to(dev)
            aff_dev, sub_dev = up[:B * 12], up[B * 12:].view(torch.int32)
        else:
            aff_dev = torch.from_numpy(aff).to(dev)
    if aff_dev.numel() != B * 12:
        raise ValueError("affine_points: affine must hold [B,12] floats")
    cl = (out_cl if out_cl is not None else torch.empty_like(src)) if want_cl else None
    cfirst = torch.empty(B, C, M, dtype=torch.float32, device=dev) if want_cf else None
    sub = torch.empty(B, C, n_sub, dtype=torch.float32, device=dev) if n_sub else None
    with profiler.span("affine_points", 4.0 * B * C * (M * (1 + bool(want_cl) + bool(want_cf)) + 2 * n_sub)):
        call("prifit_affine_points", ptr(src), B, M, C, ptr(aff_dev), ptr(sub_dev), n_sub, ptr(cl), ptr(cfirst), ptr(sub),
             cur_stream())
    return cl, cfirst, sub


def perturb_points(src, affine=None, *, rotate_normals=False, sigma=0.0, clip=0.0, drop_ratio=None, seed=0, want_cf=False, out=None):
    """The per-point augmentations of provider.py in ONE launch (csrc/perturb.hip; contract: prifit_perturb_points in the header):
    the per-shape map of `affine_points` on xyz, with `rotate_normals` its 3x3 part on channels 3..5 too, then clipped Gaussian
    jitter (sigma > 0: xyz += clamp(sigma * z, -clip, clip)), then point dropout (point p of shape b takes point 0's output iff
    its uniform draw is <= drop_ratio[b]).  src [B,M,C] contiguous float32, C 3 or 6; affine [B,12] float32 or None (xyz copied);
    drop_ratio [B] or None; both on the host (uploaded TOGETHER in one copy) or on the device.  seed: a 64-bit integer, the key
    of the counter-based generator -- the same seed gives the same bits.
    -> (cl [B,M,C] | None, cf [B,C,M] | None).  cl is written into `out` when given (may be `src`: in place), else into a new
    tensor; with want_cf and no `out`, only the channels-first copy is made and cl is None."""
    if not torch.is_tensor(src) or src.dtype != torch.float32 or src.dim() != 3 or src.shape[2] not in (3, 6) or not src.is_contiguous():
        raise ValueError("perturb_points: src must be a contiguous float32 [B,M,3] or [B,M,6] tensor")
    B, M, C = src.shape
    if B < 1 or M < 1:
        raise ValueError("perturb_points: empty batch %s" % (tuple(src.shape),))
    if rotate_normals and (C != 6 or affine is None):
        raise ValueError("perturb_points: rotate_normals needs a [B,M,6] batch and an affine map")
    sigma, clip = float(sigma), float(clip)
    if not sigma >= 0.0 or (sigma > 0.0 and not clip > 0.0):
        raise ValueError("perturb_points: sigma must be >= 0, and clip > 0 where sigma > 0 (got sigma %r, clip %r)" % (sigma, clip))
    if out is not None and (not torch.is_tensor(out) or out.shape != src.shape or out.dtype != torch.float32
                            or out.device != src.device or not out.is_contiguous()):
        raise ValueError("perturb_points: out must be a contiguous float32 tensor of src's shape on src's device")
    host = {}
    for name, v, n in (("affine", affine, B * 12), ("drop_ratio", drop_ratio, B)):
        if v is None:
            continue
        if torch.is_tensor(v) and v.is_cuda:
            if v.dtype != torch.float32 or v.numel() != n or not v.is_contiguous():
                raise ValueError("perturb_points: a device %s must hold %d contiguous float32" % (name, n))
        else:
            v = np.ascontiguousarray(v.numpy() if torch.is_tensor(v) else v, dtype=np.float32)
            if v.size != n:
                raise ValueError("perturb_points: %s must hold %d floats, got shape %s" % (name, n, v.shape))
            host[name] = v.reshape(-1)
        if name == "affine":
            affine = v
        else:
            drop_ratio = v
    require_cuda(src)
    if host:                                     # what lives on the host travels in one copy
        up = torch.from_numpy(np.concatenate(list(host.values()))).to(src.device)
        at = 0
        for name, v in host.items():
            part, at = up[at:at + v.size], at + v.size
            if name == "affine":
                affine = part
            else:
                drop_ratio = part
    seed = int(seed) & 0xffffffffffffffff
    cl = out if out is not None else (None if want_cf else torch.empty_like(src))
    cfirst = torch.empty(B, C, M, dtype=torch.float32, device=src.device) if want_cf else None
    with profiler.span("perturb_points", 4.0 * B * C * M * (1 + (cl is not None) + bool(want_cf))):
        call("prifit_perturb_points", ptr(src), B, M, C, ptr(affine), int(bool(rotate_normals)), sigma, clip, ptr(drop_ratio),
             seed & 0xffffffff, seed >> 32, ptr(cl), ptr(cfirst), cur_stream())
    return cl, cfirst


def seg_metrics(scores, target, cat_of_label, restricted=True, totals=None, out=None):
    """The part-segmentation counts of testing.py:139-204 in ONE launch, nothing read back (csrc/seg_metrics.hip).
    scores [B,N,P] float32 part scores, P <= 64 (a view with a row stride >= P is taken as it is); target [B,N] int64 labels;
    cat_of_label [P] int32 DEVICE tensor, the category of each part (-1 = none).  restricted: the arg-max runs over the parts of
    the shape's category (that of its first label) only, first maximum, numpy's NaN order; False: over all P parts.
    totals: int64 [2 + 2 P] device tensor to ACCUMULATE into -- correct, bad, seen_class [P], correct_class [P] -- or None for a
    fresh zeroed one; bad counts the rows whose label (or, restricted, whose shape's first label) has no part / category: the
    caller turns it into an error.  out: optional (pred | None, shape_cat, inter, uni) to write into, inter and uni ZEROED by
    the caller.  -> (pred [B,N] int64, shape_cat [B] int32, inter [B,P] int32, uni [B,P] int32, totals)."""
    require_cuda(scores, target, cat_of_label)
    if scores.dim() != 3 or scores.dtype != torch.float32:
        raise ValueError("seg_metrics: scores must be a float32 [B,N,P] tensor")
    B, N, P = scores.shape
    if P > 64 or B * N == 0:
        raise ValueError("seg_metrics: needs 1 <= P <= 64 parts and at least one point, got %s" % (tuple(scores.shape),))
    if scores.stride(2) != 1 or scores.stride(1) < P or (B > 1 and scores.stride(0) != N * scores.stride(1)):
        scores = scores.contiguous()
    if tuple(target.shape) != (B, N):
        raise ValueError("seg_metrics: target must be [B,N] = %s, got %s" % ((B, N), tuple(target.shape)))
    target = target.long().contiguous()
    if cat_of_label.dtype != torch.int32 or cat_of_label.numel() != P or not cat_of_label.is_contiguous():
        raise ValueError("seg_metrics: cat_of_label must be a contiguous int32 [P] tensor")
    dev = scores.device
    if totals is None:
        totals = torch.zeros(2 + 2 * P, dtype=torch.int64, device=dev)
    elif totals.dtype != torch.int64 or totals.numel() != 2 + 2 * P or not totals.is_cuda or not totals.is_contiguous():
        raise ValueError("seg_metrics: totals must be a contiguous int64 [2 + 2 P] device tensor")
    if out is None:
        pred = torch.empty(B, N, dtype=torch.int64, device=dev)
        counts = zero_pool.zeros(B * (1 + 2 * P), device=dev).view(torch.int32)     # zero bits: one fill for the three
        shape_cat, inter, uni = counts[:B], counts[B:B + B * P].view(B, P), counts[B + B * P:].view(B, P)
    else:
        pred, shape_cat, inter, uni = out
        for name, t, dt, shp in (("pred", pred, torch.int64, (B, N)), ("shape_cat", shape_cat, torch.int32, (B,)),
                                 ("inter", inter, torch.int32, (B, P)), ("uni", uni, torch.int32, (B, P))):
            if t is not None and (t.dtype != dt or tuple(t.shape) != shp or not t.is_cuda or not t.is_contiguous()):
                raise ValueError("seg_metrics: out %s must be a contiguous %s %s device tensor" % (name, dt, shp))
    with profiler.span("seg_metrics", 4.0 * B * N * P):
        call("prifit_seg_metrics", ptr(scores), scores.stride(1), ptr(target), B, N, P, ptr(cat_of_label), int(bool(restricted)),
             ptr(pred), ptr(shape_cat), ptr(inter), ptr(uni), ptr(totals), cur_stream())
    return pred, shape_cat, inter, uni, totals

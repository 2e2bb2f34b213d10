"""MI355X backend behind the call surface of the reference's models/pointnet_util.py.

Same function / class names, constructor arguments, tensor layouts ([B, C, N] in and out) and
state_dict keys as upstream (models/pointnet_util.py:19-314); every op runs as a hand-written HIP
kernel through libprifit_hip.so.  There is no CPU fallback: tensors must live on the GPU.

Differences that are deliberate and documented (SURVEY.md section 8a'):
  * farthest_point_sample / the modules take an optional explicit FPS start index (`fps_start`);
    when omitted a random start is drawn exactly like upstream (:75);
  * internally activations are channels-last and input channels are zero-padded to multiples of 4
    (weights are re-packed on the fly; gradients flow back to the upstream-shaped parameters).
"""
import collections
import contextlib
import ctypes
import os
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import nn_ops, ops
from .. import arena as zero_pool
from .._lib import call, cur_stream, ptr, query
from ..nn_ops import (ConcatWindowsFn, FpRowsFn, FrontEnd, GatherLinearFn, GroupGatherFn, LinearFn, SAGroupDirectFn, SAGroupGatherFn,
                      SharedMLPFn, ThreeInterpolateFn, _mlp_tensors, _ptr_array, _sa_group_launch, front_end_args, sa_group_supported,
                      sa_point_tables)


# ------------------------------------------------------------------ functional surface (:19-107)

def _z(like, *shape):
    """Zero padding blocks from the step's one pre-zeroed pool (prifit_amd/arena.py) instead of a fill launch each."""
    if like.is_cuda and like.dtype == torch.float32:
        return zero_pool.zeros(*shape, device=like.device)
    return like.new_zeros(*shape)

def square_distance(src, dst):
    """upstream :19-40 -- src [B,N,3], dst [B,M,3] -> [B,N,M] (expanded form, bitwise)."""
    return ops.square_distance(src, dst)


def index_points(points, idx):
    """upstream :43-60 -- points [B,N,C], idx [B,S] or [B,S,K] -> [B,S,(K,)C]."""
    B = points.shape[0]
    flat = idx.reshape(B, -1).long()
    out = torch.gather(points, 1, flat.unsqueeze(-1).expand(-1, -1, points.shape[-1]))
    return out.reshape(*idx.shape, points.shape[-1])


def farthest_point_sample(xyz, npoint, start_idx=None):
    """upstream :63-84 -- xyz [B,N,3] -> int64 [B,npoint]."""
    return ops.farthest_point_sample(xyz, npoint, start_idx)


def query_ball_point(radius, nsample, xyz, new_xyz):
    """upstream :87-107 -- int64 [B,S,nsample]."""
    return ops.ball_query_multi([radius], [nsample], xyz, new_xyz, idx64=True)[0]


def _pad4(c):
    return (c + 3) // 4 * 4


_col_index_cache = {}


def _col_index(cols, ncols, device):
    """(map, inv_off, inv_idx) int32 device tensors of a column map `cols` (tuple; entry j = source column of output column j,
    -1 = zero column), cached per device: the map itself and the CSR of its inverse (for every source column the output
    columns it feeds, ascending)."""
    key = (cols, ncols, str(device))
    hit = _col_index_cache.get(key)
    if hit is None:
        inv = [[] for _ in range(ncols)]
        for j, c in enumerate(cols):
            if c >= 0:
                inv[c].append(j)
        off = [0]
        for lst in inv:
            off.append(off[-1] + len(lst))
        flat = [j for lst in inv for j in lst] or [0]
        hit = _col_index_cache[key] = tuple(torch.tensor(t, dtype=torch.int32, device=device) for t in (list(cols), off, flat))
    return hit


class PackColsFn(torch.autograd.Function):
    """out[:, j] = w[:, cols[j]] (cols[j] < 0: a zero column): a column permutation / padding of a weight matrix as one
    launch forward (prifit_pack_cols) and one backward (prifit_unpack_cols: a source column may feed several output columns --
    their gradients are summed).  Slices + cat do the same with a zero-fill and a copy per slice in the backward, index_select
    / index_add_ with 2 + 3 launches per weight: ~30 tiny launches per training step over the first layers."""

    @staticmethod
    def forward(ctx, w, cols):
        w = w.contiguous()
        cmap, inv_off, inv_idx = _col_index(cols, w.shape[1], w.device)
        ctx.idx, ctx.ncols = (inv_off, inv_idx), w.shape[1]
        out = torch.empty(w.shape[0], len(cols), dtype=torch.float32, device=w.device)
        call("prifit_pack_cols", ptr(w), w.shape[0], w.shape[1], ptr(cmap), len(cols), ptr(out), cur_stream())
        return out

    @staticmethod
    def backward(ctx, g):
        inv_off, inv_idx = ctx.idx
        g = g.contiguous()
        gw = torch.empty(g.shape[0], ctx.ncols, dtype=torch.float32, device=g.device)
        call("prifit_unpack_cols", ptr(g), g.shape[0], g.shape[1], ptr(inv_off), ptr(inv_idx), ctx.ncols, ptr(gw), cur_stream())
        return gw, None


class PackAllFn(torch.autograd.Function):
    """PackColsFn for every packed weight of a network at once: ONE launch forward (prifit_pack_cols_multi), one backward.
    apply(specs, *ws) -> tuple of packed matrices; specs[i] = the column map of ws[i]."""

    @staticmethod
    def forward(ctx, specs, *ws):
        ws = [w.contiguous() for w in ws]
        idx = [_col_index(cols, w.shape[1], w.device) for cols, w in zip(specs, ws)]
        outs = [torch.empty(w.shape[0], len(cols), dtype=torch.float32, device=w.device) for cols, w in zip(specs, ws)]
        n = len(ws)
        ints = lambda v: (ctypes.c_int32 * n)(*v)
        call("prifit_pack_cols_multi", n, _ptr_array(ws), ints([w.shape[0] for w in ws]), ints([w.shape[1] for w in ws]),
             _ptr_array([i[0] for i in idx]), ints([len(c) for c in specs]), _ptr_array(outs), cur_stream())
        ctx.idx, ctx.shapes = idx, [tuple(w.shape) for w in ws]
        ctx.set_materialize_grads(False)      # an output nobody used: None in the backward, its job is skipped
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        live = [i for i, g in enumerate(gs) if g is not None]
        gws = [None] * len(gs)
        if live:
            g = [gs[i].contiguous() for i in live]
            out = [torch.empty(ctx.shapes[i], dtype=torch.float32, device=g[0].device) for i in live]
            n = len(live)
            ints = lambda v: (ctypes.c_int32 * n)(*v)
            call("prifit_unpack_cols_multi", n, _ptr_array(g), ints([t.shape[0] for t in g]), ints([t.shape[1] for t in g]),
                 _ptr_array([ctx.idx[i][1] for i in live]), _ptr_array([ctx.idx[i][2] for i in live]),
                 ints([ctx.shapes[i][1] for i in live]), _ptr_array(out), cur_stream())
            for i, o in zip(live, out):
                gws[i] = o
        return (None, *gws)


class PackPlan:
    """The packed weights a network asks for during a forward, remembered (first forward) and then produced together at the
    top of every later forward (`with pack_plan(net):`): 8 + 8 launches of a training step become 1 + 1.  A site that is not in
    the plan -- the first forward, a weight that appeared later -- takes the single launch and joins."""

    def __init__(self):
        self.sites, self.keys, self.results = [], set(), None

    def begin(self):
        self.results = {}
        if self.sites and _PACK_ALL:
            outs = PackAllFn.apply(tuple(c for _, c in self.sites), *[p.reshape(p.shape[0], -1) for p, _ in self.sites])
            self.results = {(id(p), c): o for (p, c), o in zip(self.sites, outs)}

    def lookup(self, w, cols):
        base = w._base if w._base is not None else w
        key = (id(base), cols)
        hit = None if self.results is None else self.results.get(key)
        if hit is not None:
            return hit
        if key not in self.keys and isinstance(base, nn.Parameter) and len(self.sites) < _pack_max_jobs():
            self.sites.append((base, cols))
            self.keys.add(key)
        return None


_PACK_ALL = os.environ.get("PRIFIT_PACK_ALL", "1") != "0"    # 0: one launch per packed weight (A/B)
_plans = weakref.WeakKeyDictionary()
_active_plan = None


def _pack_max_jobs():
    return query("prifit_pack_cols_max_jobs")


@contextlib.contextmanager
def pack_plan(net):
    """Inside: `_pack_cols` serves the weights of `net` from one launch (see PackPlan).  Re-entrant: a forward of `net` inside
    its own forward (activation checkpointing, embed() inside forward) gets its own results and hands the outer ones back."""
    global _active_plan
    plan = _plans.get(net)
    if plan is None:
        plan = _plans[net] = PackPlan()
    outer, _active_plan = _active_plan, plan
    outer_results = plan.results
    plan.begin()
    try:
        yield plan
    finally:
        plan.results = outer_results
        _active_plan = outer


def _pack_cols(w, cols):
    cols = tuple(cols)
    if cols == tuple(range(w.shape[1])):
        return w
    if _active_plan is not None and w.is_cuda:
        hit = _active_plan.lookup(w, cols)
        if hit is not None:
            return hit
    return PackColsFn.apply(w, cols)


def _pack_weight(conv, perm_slices, kp):
    """[Cout, Cin(,1,1)] -> [Cout, kp]: columns re-ordered to the internal row layout, zero padded."""
    w = conv.weight.reshape(conv.weight.shape[0], -1)
    cols = [c for a, b in perm_slices for c in range(a, b)]
    return _pack_cols(w, cols + [-1] * (kp - len(cols)))


# The first layer of a set-abstraction MLP is computed by linearity (no grouped tensor) when the grouped row would
# be wider than the layer's output; PRIFIT_SA_LINEARITY=0 keeps the gather + GEMM form for A/B measurements.
_SA_LINEARITY = os.environ.get("PRIFIT_SA_LINEARITY", "1") != "0"
# Ball query + grouping + the first conv of every per-radius MLP in ONE launch (csrc/sa_group.hip);
# PRIFIT_SA_FUSED=0 keeps the separate ball-query / gather / GEMM launches for A/B measurements.
_SA_FUSED = os.environ.get("PRIFIT_SA_FUSED", "1") != "0"
# direct mode in training: the first layer's BatchNorm backward is fused into its weight-gradient kernel (0: separate
# bn_relu_bwd_apply pass + SAGroupDirectFn autograd, A/B)
_DIRECT_FUSED_BWD = os.environ.get("PRIFIT_SA_DIRECT_FUSED_BWD", "1") != "0"
# gather mode in training: dU / dVc of the first layer come out of ONE kernel with that layer's BatchNorm + ReLU backward
# folded in and the scatter staged in LDS (0: bn_relu_bwd_apply pass + SAGroupGatherFn autograd with global atomics, A/B)
_GATHER_FUSED_BWD = os.environ.get("PRIFIT_SA_GATHER_FUSED_BWD", "1") != "0"
# Direct-mode levels (SA1) in training: the 64-wide first-layer rows of a scale are NOT stored when every consumer can
# re-form them from the L2-resident per-point table U (first layer by linearity, bias folded in) -- the forward product of
# layer 2, the one-pass backward of layer 2 and the first conv's weight-gradient reduction (nn_ops.SharedMLPFn, FrontEnd
# mode "norows").  SA1 at B = 24: 0.6 GB less written and 1.8 GB less read per step (2.4 GB of the step's ~36 GB of HBM traffic).
# MEASURED AND NOT THE DEFAULT: the grouping launches drop from 0.21 to 0.125 ms, but every consumer is SLOWER on
# rows gathered from L2 than on rows streamed from HBM (forward product +6 us, one-pass backward +26 us, weight-gradient
# reduction +22 us per scale): c2 10.09 -> 10.17 ms, c3 15.19 -> 15.30 ms on one box, alternating runs.  These kernels are
# not limited by HBM bytes alone.  PRIFIT_SA_NOROWS=1 turns it on (both arms are tested).
_SA_NOROWS = os.environ.get("PRIFIT_SA_NOROWS", "0") != "0"


def _linearity_rows(feats, xyz, new_xyz, kp):
    """The two row tables every radius of a level multiplies: rows [B N, kp] = [feat | xyz | 0-pad] per point and
    c4 [B S, 4] = [centre | 0] per centre (built once per level, not once per radius)."""
    B, N, _ = xyz.shape
    D = 0 if feats is None else feats.shape[-1]
    S = new_xyz.shape[1]
    parts = ([feats] if feats is not None else []) + [xyz]
    if kp > D + 3:
        parts.append(_z(xyz, B, N, kp - D - 3))
    rows = torch.cat(parts, dim=-1).reshape(B * N, kp)
    c4 = torch.cat([new_xyz, _z(new_xyz, B, S, 1)], dim=-1).reshape(B * S, 4)
    return rows, c4


def _linearity_operands(conv, feats, xyz, new_xyz, kp, feat_first, fold_bias=False, tables=None):
    """U [B,N,C1] = [feat | xyz] W1^T per POINT and Vc [B,S,C1] = c W1x^T per CENTRE (two small GEMMs):
    conv1([feat_j | xyz_j - c_g]) = U_j - Vc_g + bias.  fold_bias: the bias is added to U (then y = U_j - Vc_g).
    tables: `_linearity_rows(...)` of the level when several radii share them."""
    B, N, _ = xyz.shape
    D = 0 if feats is None else feats.shape[-1]
    S = new_xyz.shape[1]
    w = conv.weight.reshape(conv.weight.shape[0], -1)
    C1 = w.shape[0]
    if feat_first:   # upstream MSG order [features, rel_xyz] (:247)
        fcols, xcols = list(range(D)), list(range(D, D + 3))
    else:            # upstream single-scale order [rel_xyz, features] (:131)
        fcols, xcols = list(range(3, 3 + D)), list(range(3))
    rows, c4 = tables if tables is not None else _linearity_rows(feats, xyz, new_xyz, kp)
    w_pt = _pack_cols(w, fcols + xcols + [-1] * (kp - D - 3))
    U = LinearFn.apply(rows, w_pt, conv.bias if fold_bias else None).reshape(B, N, C1)
    Vc = LinearFn.apply(c4, _pack_cols(w, xcols + [-1]), None).reshape(B, S, C1)
    return U, Vc


def _norows_scales(conv_blocks, B, S, nsamples):
    """Per scale of a direct-mode level in training: can its first-layer rows stay unstored?  (64-wide first layer, whole
    64-row tiles per centre, >= 3 layers, the second layer on the streaming forward kernel and the one-pass backward kernel.)"""
    if not (_SA_NOROWS and nn_ops._FUSE_RED and nn_ops._FUSE_BN_APPLY and nn_ops._STREAM):
        return [False] * len(conv_blocks)
    out = []
    for convs, K in zip(conv_blocks, nsamples):
        P = B * S * K
        C1 = convs[0].weight.shape[0]
        ok = (len(convs) >= 3 and C1 == 64 and K % 64 == 0 and P < (1 << 24) and convs[1].weight.shape[1] == 64)
        if ok:
            C2 = convs[1].weight.shape[0]
            ok = bool(query("prifit_gemm_stream_supported", 0, P, C2, 64)) and bool(query("prifit_gemm_stream_bwd_supported", P, C2, 64, 0))
        out.append(ok)
    return out


# How the first layers of a set-abstraction level come about (DESIGN.md 3.2 has the entry points in order).
#   name             what runs                                                               FrontEnd.mode of a scale
#   direct           one fused launch, narrow inputs, weights in registers (data for autograd)   "direct"
#   norows           sa_point_tables + one fused launch in the by-linearity form (data)       "norows" where norows[i], else "direct"
#   gather           U / Vc products + one fused launch (data; U / Vc stay differentiable)    "gather"
#   direct_autograd  SAGroupDirectFn (eval mode, or PRIFIT_SA_DIRECT_FUSED_BWD=0)             "preact"
#   gather_autograd  U / Vc products + SAGroupGatherFn                                        "preact"
#   separate         ball query, then per scale GatherLinearFn where linearity[i] ("preact"), else grouped rows + product (no record)
_LevelRoute = collections.namedtuple("_LevelRoute", "name norows linearity", defaults=(None, None))


def _level_route(conv_blocks, feats, training, B, N, S, nsamples, kp, allow_norows):
    """The route of a level; launches nothing, reads the module switches and query(...) only, at every call (tests flip the
    switches between two calls)."""
    widths = [blk[0].weight.shape[0] for blk in conv_blocks]
    linearity = [_SA_LINEARITY and kp > c for c in widths]       # the grouped row would be wider than the layer's output
    if _SA_FUSED and _SA_LINEARITY and sa_group_supported(N, nsamples, widths):
        D = 0 if feats is None else feats.shape[-1]
        if D in (0, 3, 6) and (feats is None or not feats.requires_grad):
            if not (training and _DIRECT_FUSED_BWD):
                return _LevelRoute("direct_autograd")
            norows = _norows_scales(conv_blocks, B, S, nsamples) if allow_norows else [False]
            return _LevelRoute("norows", norows) if any(norows) else _LevelRoute("direct")
        if all(linearity):
            own_bwd = (training and _GATHER_FUSED_BWD and all(len(blk) >= 2 for blk in conv_blocks) and
                       all(query("prifit_gather_linear_bwd_bn_supported", N, c) for c in widths))
            return _LevelRoute("gather" if own_bwd else "gather_autograd")
    return _LevelRoute("separate", None, linearity)


def _fused_front_end(route, first_convs, training, feats, xyz, new_xyz, radii, nsamples, kp, feat_first):
    """The fused launch of a level (any route but "separate") -> (one FrontEnd per scale, their Y1 [B*S*K, C1]; None where
    the rows are not stored).  On the routes "direct" / "norows" / "gather" the launch is plain data for autograd: the
    SharedMLPFn that consumes Y1 owns the first layer's backward (its BatchNorm backward folded into the weight-gradient
    or dU / dVc kernel); on the "_autograd" routes SAGroup*Fn do."""
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    D = 0 if feats is None else feats.shape[-1]
    R, radii, nsamples = len(first_convs), list(radii), list(nsamples)
    if route.name in ("direct_autograd", "gather_autograd"):
        ts = []
        if route.name == "direct_autograd":
            for c in first_convs:
                ts += [c.weight.reshape(c.weight.shape[0], -1), c.bias]
            out = SAGroupDirectFn.apply(xyz, new_xyz, feats, (radii, nsamples, feat_first, training), *ts)
        else:
            tables = _linearity_rows(feats, xyz, new_xyz, kp)
            for c in first_convs:
                U, Vc = _linearity_operands(c, feats, xyz, new_xyz, kp, feat_first, tables=tables)
                ts += [U, Vc, c.bias]
            out = SAGroupGatherFn.apply(xyz, new_xyz, (radii, nsamples, training), *ts)
        return [FrontEnd("preact", out[2 * i + 1]) for i in range(R)], list(out[0::2])
    if route.name == "direct":
        with torch.no_grad():
            Ws = [c.weight.reshape(c.weight.shape[0], -1).contiguous() for c in first_convs]
            bs = [None if c.bias is None else c.bias.contiguous() for c in first_convs]
            fx = feats is not None and D == 3 and feats.data_ptr() == xyz.data_ptr()
            Ys, slabs, idxs = _sa_group_launch(0, xyz, new_xyz, feats, feat_first, radii, nsamples,
                                               [w.shape[0] for w in Ws], Ws, None, None, bs, feat_xyz=fx)
        tabs = [(None, None)] * R
    else:
        # the by-linearity form of the launch: y = U_j - Vc_g with U = [feat | xyz] W1^T per point, Vc = c W1x^T per centre
        if route.name == "norows":
            # U / Vc are plain data with the bias folded into U (the first conv's weight gradient stays the direct
            # reduction dW1 = dY1^T [feat | rel]); index lists and statistics of every scale, rows only where wanted
            with torch.no_grad():
                Us, Vcs = sa_point_tables(first_convs, feats, xyz, new_xyz, feat_first)
            tabs = [(u, v) if nr else (None, None) for u, v, nr in zip(Us, Vcs, route.norows)]
            bs, rows = [None] * R, [not nr for nr in route.norows]
        else:
            # U / Vc stay differentiable: SharedMLPFn returns dU / dVc
            tables = _linearity_rows(feats, xyz, new_xyz, kp)
            tabs = [_linearity_operands(c, feats, xyz, new_xyz, kp, feat_first, tables=tables) for c in first_convs]
            Us = [u.detach().contiguous() for u, _ in tabs]
            Vcs = [v.detach().contiguous() for _, v in tabs]
            bs, rows = [None if c.bias is None else c.bias.detach().contiguous() for c in first_convs], None
        with torch.no_grad():
            Ys, slabs, idxs = _sa_group_launch(1, xyz, new_xyz, None, True, radii, nsamples,
                                               [u.shape[-1] for u in Us], None, Us, Vcs, bs, rows=rows)
    fronts = []
    for i in range(R):
        if route.name == "gather":
            fronts.append(FrontEnd("gather", slabs[i], idxs[i], B, N, S, nsamples[i], D, U=tabs[i][0], Vc=tabs[i][1]))
        else:
            fronts.append(FrontEnd("direct" if tabs[i][0] is None else "norows", slabs[i], idxs[i], B, N, S, nsamples[i], D,
                                   xyz, new_xyz, feats, feat_first, *tabs[i]))
    return fronts, Ys


def _sa_level(conv_blocks, bn_blocks, npoint, radii, nsamples, training, xyz, feats, fps_start, *, feat_first, rows_perm, concat,
              allow_norows):
    """One sampled set-abstraction level, channels-last: xyz [B,N,3], feats [B,N,D] or None -> (new_xyz [B,S,3], out [B,S,C']):
    farthest-point sampling, then per scale the grouped [feat | rel_xyz] rows through its MLP and the max over each group.
    What the two modules differ in, beside the number of scales:
      feat_first    upstream's column order of the first conv: [features, rel_xyz] (MSG, :247) or [rel_xyz, features] (:131)
      rows_perm     the column slices of the first conv's weight in the order of the internal grouped rows [features, rel_xyz]
      concat        True: the scales' pooled outputs are concatenated -- on the fused routes they are written side by side into
                    column windows of one buffer (ConcatWindowsFn, no copy), else torch.cat; False: the one scale's output is it
      allow_norows  the "norows" route may be taken (the single-scale module has never been wired to it: kept as found)"""
    B, N, _ = xyz.shape
    S = npoint
    D = 0 if feats is None else feats.shape[-1]
    kp = _pad4(D + 3)
    _, new_xyz = ops.farthest_point_sample(xyz, S, fps_start, return_xyz=True)
    route = _level_route(conv_blocks, feats, training, B, N, S, nsamples, kp, allow_norows)
    pooled = []
    if route.name != "separate":
        fronts, ys = _fused_front_end(route, [blk[0] for blk in conv_blocks], training, feats, xyz, new_xyz, radii, nsamples, kp,
                                      feat_first)
        if concat:
            widths = [blk[-1].weight.shape[0] for blk in conv_blocks]
            wide = torch.empty(B * S, sum(widths), dtype=torch.float32, device=xyz.device)
        c0 = 0
        for i, K in enumerate(nsamples):
            cfg, ts = front_end_args(_mlp_cfg(bn_blocks[i], K, training), conv_blocks[i], bn_blocks[i], fronts[i])
            if concat:
                cfg["pool_out"] = wide[:, c0:c0 + widths[i]]
                c0 += widths[i]
            pooled.append(SharedMLPFn.apply(ys[i], cfg, *ts))
        out = ConcatWindowsFn.apply(wide, *pooled) if concat else pooled[0]
        return new_xyz, out.reshape(B, S, -1)
    idxs = ops.ball_query_multi(list(radii), list(nsamples), xyz, new_xyz)  # one pass, all radii
    for i, K in enumerate(nsamples):
        convs, bns = conv_blocks[i], bn_blocks[i]
        if route.linearity[i]:
            # conv1 over the grouped rows without materialising them: project every POINT once (U), every CENTRE once (Vc),
            # then gather C1-wide rows
            U, Vc = _linearity_operands(convs[0], feats, xyz, new_xyz, kp, feat_first)
            y1, slab = GatherLinearFn.apply(U, Vc, convs[0].bias, idxs[i], training)
            cfg, ts = front_end_args(_mlp_cfg(bns, K, training), convs, bns, FrontEnd("preact", slab))
            pooled.append(SharedMLPFn.apply(y1, cfg, *ts))
            continue
        rows = GroupGatherFn.apply(feats, xyz, new_xyz, idxs[i], 0, kp)
        w0 = _pack_weight(convs[0], rows_perm, kp)
        pooled.append(SharedMLPFn.apply(rows, _mlp_cfg(bns, K, training), *_mlp_tensors(convs, bns, w0)))
    out = torch.cat(pooled, dim=-1) if concat else pooled[0]
    return new_xyz, out.reshape(B, S, -1)


_pending_counters = None   # list while a model forward batches the BatchNorm step counters, else None


class batched_bn_counters:
    """`num_batches_tracked += 1` of every BatchNorm touched inside the block as ONE multi-tensor add at exit
    (25 single-element kernels per forward otherwise)."""

    def __enter__(self):
        global _pending_counters
        self.prev, _pending_counters = _pending_counters, []
        return self

    def __exit__(self, *exc):
        global _pending_counters
        todo, _pending_counters = _pending_counters, self.prev
        if todo and exc[0] is None:
            torch._foreach_add_(todo, 1)
        return False


def _mlp_cfg(bns, pool_K, training):
    for bn in bns:
        if training and bn.num_batches_tracked is not None:
            if _pending_counters is not None:
                _pending_counters.append(bn.num_batches_tracked)
            else:
                bn.num_batches_tracked += 1
    return {"pool_K": pool_K, "training": training, "eps": bns[0].eps,
            "momentum": [0.1 if bn.momentum is None else bn.momentum for bn in bns]}


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False, fps_start=None):
    """upstream :110-137 (SSG order [rel_xyz, features]); returns the reference's 4-D tensors."""
    B, N, C = xyz.shape
    fps_idx, new_xyz = ops.farthest_point_sample(xyz, npoint, fps_start, return_xyz=True)
    idx = ops.ball_query_multi([radius], [nsample], xyz, new_xyz)[0]
    D = 0 if points is None else points.shape[-1]
    rows = GroupGatherFn.apply(None if points is None else points.contiguous(), xyz.contiguous(), new_xyz, idx, 1,
                               _pad4(D + 3))
    new_points = rows[:, :D + 3].reshape(B, npoint, nsample, D + 3)
    if returnfps:
        return new_xyz, new_points, index_points(xyz, idx), fps_idx
    return new_xyz, new_points


def sample_and_group_all(xyz, points):
    """upstream :140-157."""
    B, N, C = xyz.shape
    new_xyz = torch.zeros(B, 1, C, device=xyz.device, dtype=xyz.dtype)
    grouped = xyz.view(B, 1, N, C)
    if points is not None:
        grouped = torch.cat([grouped, points.view(B, 1, N, -1)], dim=-1)
    return new_xyz, grouped


# ------------------------------------------------------------------ modules (:160-314)
class PointNetSetAbstraction(nn.Module):
    """upstream :160-201 (single-scale or group_all).  state_dict: mlp_convs.i / mlp_bns.i."""

    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super().__init__()
        self.npoint, self.radius, self.nsample, self.group_all = npoint, radius, nsample, group_all
        self.mlp_convs, self.mlp_bns = nn.ModuleList(), nn.ModuleList()
        last = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv2d(last, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out_channel))
            last = out_channel

    def forward_cl(self, xyz, feats, fps_start=None):
        """channels-last: xyz [B,N,3], feats [B,N,D] or None -> (new_xyz [B,S,3], out [B,S,C'])."""
        if not self.group_all:
            # internal rows are [features, rel_xyz, pad]; upstream order is [rel_xyz, features] (:131)
            D = 0 if feats is None else feats.shape[-1]
            return _sa_level([self.mlp_convs], [self.mlp_bns], self.npoint, [self.radius], [self.nsample], self.training, xyz,
                             feats, fps_start, feat_first=False, rows_perm=[(3, 3 + D), (0, 3)], concat=False, allow_norows=False)
        B, N, _ = xyz.shape
        D = 0 if feats is None else feats.shape[-1]
        kp = _pad4(D + 3)
        new_xyz = torch.zeros(B, 1, 3, device=xyz.device, dtype=xyz.dtype)
        parts = [xyz] + ([feats] if feats is not None else [])  # :154 order [xyz, features]
        if kp > D + 3:
            parts.append(_z(xyz, B, N, kp - D - 3))
        rows = torch.cat(parts, dim=-1).reshape(B * N, kp)
        w0 = _pack_weight(self.mlp_convs[0], [(0, D + 3)], kp)
        out = SharedMLPFn.apply(rows, _mlp_cfg(self.mlp_bns, N, self.training),
                                *_mlp_tensors(self.mlp_convs, self.mlp_bns, w0))
        return new_xyz, out.reshape(B, 1, -1)

    def forward(self, xyz, points, fps_start=None):
        """xyz [B,3,N], points [B,D,N] -> (new_xyz [B,3,S], new_points [B,D',S])."""
        x = xyz.permute(0, 2, 1).contiguous()
        f = points.permute(0, 2, 1).contiguous() if points is not None else None
        nx, out = self.forward_cl(x, f, fps_start)
        return nx.permute(0, 2, 1), out.permute(0, 2, 1)


class PointNetSetAbstractionMsg(nn.Module):
    """upstream :204-261.  state_dict: conv_blocks.i.j / bn_blocks.i.j."""

    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super().__init__()
        self.npoint, self.radius_list, self.nsample_list = npoint, radius_list, nsample_list
        self.conv_blocks, self.bn_blocks = nn.ModuleList(), nn.ModuleList()
        for i in range(len(mlp_list)):
            convs, bns = nn.ModuleList(), nn.ModuleList()
            last = in_channel + 3
            for out_channel in mlp_list[i]:
                convs.append(nn.Conv2d(last, out_channel, 1))
                bns.append(nn.BatchNorm2d(out_channel))
                last = out_channel
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)

    def forward_cl(self, xyz, feats, fps_start=None):
        D = 0 if feats is None else feats.shape[-1]
        # internal rows are [features, rel_xyz, pad]: upstream's own order (:247)
        return _sa_level(self.conv_blocks, self.bn_blocks, self.npoint, self.radius_list, self.nsample_list, self.training, xyz,
                         feats, fps_start, feat_first=True, rows_perm=[(0, D + 3)], concat=True, allow_norows=True)

    def forward(self, xyz, points, fps_start=None):
        x = xyz.permute(0, 2, 1).contiguous()
        f = points.permute(0, 2, 1).contiguous() if points is not None else None
        nx, out = self.forward_cl(x, f, fps_start)
        return nx.permute(0, 2, 1), out.permute(0, 2, 1)


class PointNetFeaturePropagation(nn.Module):
    """upstream :264-314.  state_dict: mlp_convs.i / mlp_bns.i."""

    def __init__(self, in_channel, mlp):
        super().__init__()
        self.mlp_convs, self.mlp_bns = nn.ModuleList(), nn.ModuleList()
        last = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv1d(last, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out_channel))
            last = out_channel

    def forward_cl(self, xyz1, xyz2, points1, points2):
        """xyz1 [B,N,3], xyz2 [B,S,3], points1 [B,N,D1] or None, points2 [B,S,D2] -> [B,N,D']."""
        B, N, _ = xyz1.shape
        S = xyz2.shape[1]
        D2 = points2.shape[-1]
        D1 = 0 if points1 is None else points1.shape[-1]
        kp = _pad4(D1 + D2)
        # internal row layout [interpolated, points1, pad]; upstream concatenates [points1, interpolated] (:306)
        if S > 1 or points1 is not None:
            idx, w = ops.three_nn(xyz1, xyz2) if S > 1 else (None, None)
            rows = FpRowsFn.apply(points2, idx, w, points1, kp)          # interpolation + concatenation + padding: one launch
        else:
            if S == 1:
                interp = points2.expand(B, N, D2).reshape(B * N, D2)
            else:
                idx, w = ops.three_nn(xyz1, xyz2)
                interp = ThreeInterpolateFn.apply(points2, idx, w)
            parts = [interp]
            if points1 is not None:
                parts.append(points1.reshape(B * N, D1))
            if kp > D1 + D2:
                parts.append(_z(interp, B * N, kp - D1 - D2))
            rows = parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)
        if len(self.mlp_convs) == 0:
            return rows[:, :D1 + D2].reshape(B, N, -1)
        w0 = _pack_weight(self.mlp_convs[0], [(D1, D1 + D2), (0, D1)], kp)
        out = SharedMLPFn.apply(rows.contiguous(), _mlp_cfg(self.mlp_bns, 0, self.training),
                                *_mlp_tensors(self.mlp_convs, self.mlp_bns, w0))
        return out.reshape(B, N, -1)

    def forward(self, xyz1, xyz2, points1, points2):
        """xyz1 [B,3,N], xyz2 [B,3,S], points1 [B,D,N], points2 [B,D,S] -> [B,D',N]."""
        p1 = points1.permute(0, 2, 1).contiguous() if points1 is not None else None
        out = self.forward_cl(xyz1.permute(0, 2, 1).contiguous(), xyz2.permute(0, 2, 1).contiguous(), p1,
                              points2.permute(0, 2, 1).contiguous())
        return out.permute(0, 2, 1)

"""Frozen inference for the MSG part-segmentation network.

    frozen = prifit_amd.inference.freeze(model)      # models.pointnet2_part_seg_msg.get_model, reconstruct=False
    frozen = prifit_amd.inference.freeze(model, precision="bf16")     # the on-chip chains on the 16-bit matrix pipe (3.9.2)
    seg, (l1, l2, l3), feat, zero, zero = frozen(xyz, cls_label, fps_start=None)
    seg = frozen.predict(xyz, cls_label)             # [B, N, num_parts] log-probabilities
    part = frozen.labels(xyz, cls_label, shape_cat, cat_of_label)   # [B, N] int32 part labels, one launch for the tail
    emb = frozen.embed(xyz, cls_label)               # [B, N, 128] per-point embedding, row-major, one launch for the tail (3.9.4)
    loss_kept_correct = frozen.probe_step(xyz, cls_label, target)   # --init_cls: loss + conv2's gradient in one launch pair (3.9.3)
    frozen.refresh()                                 # re-fold from the live model (after more training)

With fixed statistics a BatchNorm is a per-channel affine: s = gamma / sqrt(var + eps), bn(W x + b) = (s W) x + ((b - mean) s + beta).
freeze() folds every layer of the network into ONE flat fp32 buffer with one launch (prifit_fold_bn) and brings the first-layer
weights that are consumed column-permuted into the internal row layouts with the existing pack launch (prifit_pack_cols_multi).
The forward then runs on that buffer alone, under no_grad:
  * sampling, ball query + grouping + first conv (prifit_sa_group_linear_fwd), 3-NN, prifit_fp_rows: the entry points of the
    live model, given the folded weights -- the index lists are the live model's, bit for bit;
  * layers 2 and 3 of every SA1 / SA2 scale and the max over the samples: one launch each (prifit_mlp_chain_pool_f32), no
    [P, C] tensor written, the pooled rows side by side in the level's output;
  * SA3, the feature-propagation stacks and the head: one folded product per layer on prifit_gemm_f32 (bias, ReLU on load
    through a unit-scale a_affine), then the existing pool / affine launch;
  * labels() only: fp1, conv1 + bn1, conv2 and the category-restricted arg-max in one launch (prifit_mlp_chain_rows_f32).
  * embed() only: fp1, conv1 + bn1, then extra_conv_emb (optionally F.normalize) and -- with return_labels -- conv2 and the
    arg-max on the same registers, one launch (prifit_mlp_chain_embed_f32): the embedding the primitive fitting consumes,
    written once, row-major.  forward(embed=True) keeps its separate launches.
  * probe_step() only: the same chain ending in the segmentation loss, the gradient of the live conv2 and the accuracy count
    (prifit_probe_head_f32) -- the training half of the tail, for pre-training the classifier layer on the frozen network.
No column statistics, no slabs, no arg-max tensors for a backward, no per-call arithmetic on weights.  There is no fall-back
to the live model: a shape the kernels do not take is an error.

The on-chip chains have one driver each (_chain_pool, _chain_rows, _chain_embed) over a table keyed by precision (_CHAINS):
entry point, queries, profiler tag and where a layer's weight lives.  precision="bf16"  changes their arithmetic
only: prifit_mlp_chain_pool_bf16, prifit_mlp_chain_rows_bf16 and prifit_mlp_chain_embed_bf16 round every layer input to bf16
and accumulate in fp32.  Their
weights are a second flat buffer of 16-bit patterns, written by ONE more launch of refresh() (prifit_pack_bf16_multi) in the
column order the MFMA reads; the biases stay fp32 in `flat`.  Everything else is the fp32 module's, launch for launch."""
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import nn_ops, ops, profiler
from ._lib import call, cur_stream, dll, ptr, query
from .models import pointnet2_part_seg_msg as _msg
from .models.pointnet_util import _col_index, _pad4

_LL = ctypes.c_longlong
_ALIGN = 64      # floats: every region of the flat buffer starts on a 256-byte boundary
_ALIGN16 = 128   # 16-bit words: likewise in the bf16 buffer
PRECISIONS = ("fp32", "bf16")

# precision -> the pool chain's and the row chain's (entry point, _supported and _workspace query = stem + ..., profiler tag); a
# chained layer's (weight, pitch) from its folded entry `ly` and its bf16 copy `w`; whether an untaken scale goes to _stack
_CHAINS = {
    "fp32": {"pool": ("prifit_mlp_chain_pool_f32", "prifit_mlp_chain_pool", "mlp_chain_pool"),
             "rows": ("prifit_mlp_chain_rows_f32", "prifit_mlp_chain_rows", "mlp_chain_rows"),
             "embed": ("prifit_mlp_chain_embed_f32", "prifit_mlp_chain_embed", "mlp_chain_embed"),
             "weight": lambda ly, w: (ly.W, ly.ldw), "pool_fallback": True},
    "bf16": {"pool": ("prifit_mlp_chain_pool_bf16", "prifit_mlp_chain_pool_bf16", "mlp_chain_pool_bf16"),
             "rows": ("prifit_mlp_chain_rows_bf16", "prifit_mlp_chain_rows_bf16", "mlp_chain_rows_bf16"),
             "embed": ("prifit_mlp_chain_embed_bf16", "prifit_mlp_chain_embed_bf16", "mlp_chain_embed_bf16"),
             "weight": lambda ly, w: (w.W, w.ldk), "pool_fallback": False},
}


class _Folded:
    """One (conv [+ BatchNorm]) layer's place in the flat buffer: W' [cout, ldw] at w_off, b' [cout] at b_off."""

    def __init__(self, conv, bn):
        self.conv, self.bn = conv, bn
        self.cout = conv.weight.shape[0]
        self.kin = conv.weight.numel() // self.cout
        self.ldw = _pad4(self.kin)
        self.w_off = self.b_off = -1
        self.W = self.b = None                      # views of the flat buffer (FrozenPartSeg._bind)


class _Packed:
    """A column-packed copy of a folded first-layer weight: out [cout, len(cols)][c][j] = W'[c][cols[j]] (cols[j] < 0: 0)."""

    def __init__(self, layer, cols):
        self.layer, self.cols = layer, tuple(cols)
        self.ldw = len(self.cols)
        self.off = -1
        self.W = None


class _Bf16:
    """The bf16 copy of a chained layer's weight: `src` (a _Folded or a _Packed) with `cols` input columns -> [cout, ldk]
    16-bit patterns at `off` of the bf16 buffer, ldk = cols rounded up to 16; order 0: plain columns (a first layer, fed
    from memory), 1: the accumulator order (a layer fed by the previous product's registers)."""

    def __init__(self, src, cout, cols, order):
        self.src, self.cout, self.cols, self.order = src, cout, cols, order
        self.ldk = (cols + 15) // 16 * 16
        self.off = -1
        self.W = None


def _first_weight(layer, cols, packs):
    """The folded weight of `layer` in the column order `cols`: the fold's own rows when that is what they are (the fold
    pads a row with zero columns to a multiple of 4), else a packed copy."""
    cols = tuple(cols)
    if cols == tuple(range(layer.kin)) + (-1,) * (layer.ldw - layer.kin):
        return layer
    p = _Packed(layer, cols)
    packs.append(p)
    return p


class FrozenPartSeg(nn.Module):
    """The eval-mode forward of a `pointnet2_part_seg_msg.get_model` on folded weights; see the module docstring."""

    def __init__(self, model, precision="fp32"):
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError("FrozenPartSeg: precision must be one of %s, got %r" % (", ".join(PRECISIONS), precision))
        self.precision = precision
        if not isinstance(model, _msg.get_model):
            raise TypeError("freeze() takes a models.pointnet2_part_seg_msg.get_model (the SSG, cls, sem-seg and DGCNN networks "
                            "have no frozen form), got %s" % type(model).__name__)
        if model.reconstruct:
            raise TypeError("freeze() takes a get_model with reconstruct=False: the AtlasNet decoder has no frozen form")
        object.__setattr__(self, "_source", model)            # a reference, not a sub-module: its parameters are not ours
        self.normal_channel = model.normal_channel
        layers, packs = [], []

        def stack(convs, bns):
            out = [_Folded(c, b) for c, b in zip(convs, bns)]
            layers.extend(out)
            return out

        # set abstraction, multi-scale: the first layer of a scale either straight from the upstream weight [C1, D + 3]
        # (narrow inputs) or by linearity, U = [feat | xyz | 0] W^T per point and Vc = [c | 0] Wx^T per centre
        self._sa = []
        for sa in (model.sa1, model.sa2):
            D = sa.conv_blocks[0][0].weight.shape[1] - 3
            scales = []
            for convs, bns in zip(sa.conv_blocks, sa.bn_blocks):
                if len(convs) != 3:
                    raise TypeError("freeze(): a set-abstraction scale with %d layers" % len(convs))
                st = stack(convs, bns)
                if D in (3, 6):
                    first = (_first_weight(st[0], range(D + 3), packs),)
                else:
                    kp = _pad4(D + 3)
                    first = (_first_weight(st[0], list(range(D + 3)) + [-1] * (kp - D - 3), packs),
                             _first_weight(st[0], [D, D + 1, D + 2, -1], packs))
                scales.append((st, first))
            self._sa.append({"npoint": sa.npoint, "radii": list(sa.radius_list), "nsamples": list(sa.nsample_list), "D": D,
                             "scales": scales})
        # the group-all level: rows [xyz | feat | 0]
        st = stack(model.sa3.mlp_convs, model.sa3.mlp_bns)
        self._sa3 = (st, _first_weight(st[0], list(range(st[0].kin)) + [-1] * (st[0].ldw - st[0].kin), packs))
        # feature propagation: rows [interpolated (D2) | points1 (D1) | 0], upstream concatenates [points1 | interpolated]
        self._fp = {}
        d2 = st[-1].cout
        for name in ("fp3", "fp2", "fp1"):
            fp = getattr(model, name)
            st = stack(fp.mlp_convs, fp.mlp_bns)
            d1 = st[0].kin - d2
            kp = _pad4(d1 + d2)
            cols = list(range(d1, d1 + d2)) + list(range(d1)) + [-1] * (kp - d1 - d2)
            self._fp[name] = (st, _first_weight(st[0], cols, packs), d1, d2)
            d2 = st[-1].cout
        self._head = stack([model.conv1], [model.bn1])
        self._conv2, self._emb = stack([model.conv2, model.extra_conv_emb], [None, None])
        # labels(): fp1's rows padded to a multiple of 8 columns (the chain's k step); its first-layer weight in that order
        # is fp1's own packed copy where 4 and 8 pad alike (150 -> 152), one more packed copy otherwise (153 -> 160)
        st, w0, d1, d2 = self._fp["fp1"]
        kp, kp8 = _pad4(d1 + d2), (d1 + d2 + 7) // 8 * 8
        cols8 = list(range(d1, d1 + d2)) + list(range(d1)) + [-1] * (kp8 - d1 - d2)
        self._tail_w0 = w0 if kp8 == kp else _first_weight(st[0], cols8, packs)
        self._tail_kp = kp8
        self._tail = list(st) + list(self._head) + [self._conv2]
        self._layers, self._packs = layers, packs
        if len(layers) > query("prifit_fold_bn_max_jobs"):
            raise TypeError("freeze(): %d layers, prifit_fold_bn takes %d" % (len(layers), query("prifit_fold_bn_max_jobs")))

        # the flat buffer: [W' | b'] of every layer, the packed first-layer weights, then the unit affine (ones, zeros) that
        # turns the product kernel's normalise-on-load into a plain ReLU
        off = 0

        def take(n):
            nonlocal off
            at, off = off, off + (n + _ALIGN - 1) // _ALIGN * _ALIGN
            return at

        for ly in layers:
            ly.w_off, ly.b_off = take(ly.cout * ly.ldw), take(ly.cout)
        for p in packs:
            p.off = take(p.layer.cout * len(p.cols))
        self._unit_c = max(ly.cout for ly in layers)
        self._ones_off, self._zeros_off = take(self._unit_c), take(self._unit_c)
        dev = model.conv1.weight.device
        if dev.type != "cuda":
            raise RuntimeError("freeze() needs the model on the GPU (HIP backend only, no CPU path)")
        flat = torch.empty(off, dtype=torch.float32, device=dev)
        flat[self._ones_off:self._ones_off + self._unit_c] = 1.0
        flat[self._zeros_off:self._zeros_off + self._unit_c] = 0.0
        self.flat = nn.Parameter(flat, requires_grad=False)
        # bf16 only: the chained layers' weights as 16-bit patterns -- an integer buffer, so that .float() / .half() on
        # the module cannot reinterpret it
        self._bf16, self._emb_bf16 = [], []
        if precision == "bf16":
            chained = lambda st: [_Bf16(st[1], st[1].cout, st[1].kin, 0), _Bf16(st[2], st[2].cout, st[2].kin, 1)]
            for lv in self._sa:
                lv["bf16"] = [chained(st) for st, _ in lv["scales"]]
                self._bf16 += [w for pair in lv["bf16"] for w in pair]
            self._tail_bf16 = [_Bf16(self._tail_w0, self._tail[0].cout, self._tail_kp, 0)] + \
                              [_Bf16(ly, ly.cout, ly.kin, 1) for ly in self._tail[1:]]
            self._bf16 += self._tail_bf16
            # embed(): extra_conv_emb, fed by conv1 + bn1's registers like conv2 -- a list of its own, the same pack launch
            self._emb_bf16 = [_Bf16(self._emb, self._emb.cout, self._emb.kin, 1)]
            if len(self._bf16) + len(self._emb_bf16) > query("prifit_pack_bf16_max_jobs"):
                raise TypeError("freeze(): %d chained layers, prifit_pack_bf16_multi takes %d"
                                % (len(self._bf16) + len(self._emb_bf16), query("prifit_pack_bf16_max_jobs")))
            off16 = 0
            for w in self._bf16 + self._emb_bf16:
                w.off, off16 = off16, off16 + (w.cout * w.ldk + _ALIGN16 - 1) // _ALIGN16 * _ALIGN16
            self.register_buffer("flat_bf16", torch.zeros(off16, dtype=torch.int16, device=dev))
        self._bound = None
        nn.Module.train(self, False)
        self.refresh()

    # ------------------------------------------------------------------ module protocol
    def train(self, mode=True):
        if mode:
            raise RuntimeError("FrozenPartSeg is an inference module: train the live model and call refresh()")
        return nn.Module.train(self, False)

    def _bind(self):
        """Views of the flat buffer for every consumer (again after the module moved: `.to()` replaces the parameter's storage)."""
        flat = self.flat.data
        key = (flat.data_ptr(), flat.device) + ((self.flat_bf16.data_ptr(), self.flat_bf16.device) if self._bf16 else ())
        if self._bound == key:
            return flat
        for ly in self._layers:
            ly.W = flat[ly.w_off:ly.w_off + ly.cout * ly.ldw].view(ly.cout, ly.ldw)
            ly.b = flat[ly.b_off:ly.b_off + ly.cout]
        for p in self._packs:
            p.W = flat[p.off:p.off + p.layer.cout * len(p.cols)].view(p.layer.cout, len(p.cols))
        self._ones = flat[self._ones_off:self._ones_off + self._unit_c]
        self._zeros = flat[self._zeros_off:self._zeros_off + self._unit_c]
        for w in self._bf16 + self._emb_bf16:
            w.W = self.flat_bf16[w.off:w.off + w.cout * w.ldk].view(w.cout, w.ldk)
        self._bound = key
        return flat

    @torch.no_grad()
    def refresh(self):
        """Fold the live model's current weights and statistics into the flat buffer: one fold launch for every layer, one
        pack launch for the column-permuted first-layer weights; with precision="bf16" one more launch that writes every
        chained layer's bf16 weight from them."""
        flat = self._bind()
        ls = self._layers
        n = len(ls)
        keep = []                                              # contiguous copies, alive until the launch is enqueued

        def dp(t):
            if t is None:
                return None
            if t.device != flat.device:
                raise RuntimeError("refresh(): the live model is on %s, the frozen one on %s" % (t.device, flat.device))
            t = t.detach()
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.float().contiguous()
                keep.append(t)
            return t.data_ptr()

        arr = lambda vals: (ctypes.c_void_p * n)(*vals)
        bn = lambda ly, name: None if ly.bn is None else getattr(ly.bn, name)
        call("prifit_fold_bn", n, arr([dp(ly.conv.weight) for ly in ls]), (ctypes.c_int32 * n)(*[ly.cout for ly in ls]),
             (ctypes.c_int32 * n)(*[ly.kin for ly in ls]), arr([dp(ly.conv.bias) for ly in ls]),
             arr([dp(bn(ly, "weight")) for ly in ls]), arr([dp(bn(ly, "bias")) for ly in ls]),
             arr([dp(bn(ly, "running_mean")) for ly in ls]), arr([dp(bn(ly, "running_var")) for ly in ls]),
             (ctypes.c_float * n)(*[0.0 if ly.bn is None else float(ly.bn.eps) for ly in ls]),
             (ctypes.c_longlong * n)(*[ly.w_off for ly in ls]), (ctypes.c_int32 * n)(*[ly.ldw for ly in ls]),
             (ctypes.c_longlong * n)(*[ly.b_off for ly in ls]), ptr(flat), _LL(flat.numel()), cur_stream())
        most = query("prifit_pack_cols_max_jobs")
        for lo in range(0, len(self._packs), most):
            ps = self._packs[lo:lo + most]
            m = len(ps)
            maps = [_col_index(p.cols, p.layer.ldw, flat.device)[0] for p in ps]
            call("prifit_pack_cols_multi", m, nn_ops._ptr_array([p.layer.W for p in ps]),
                 (ctypes.c_int32 * m)(*[p.layer.cout for p in ps]), (ctypes.c_int32 * m)(*[p.layer.ldw for p in ps]),
                 nn_ops._ptr_array(maps), (ctypes.c_int32 * m)(*[len(p.cols) for p in ps]), nn_ops._ptr_array([p.W for p in ps]),
                 cur_stream())
        if self._bf16:
            ws = self._bf16 + self._emb_bf16
            m = len(ws)
            if self.flat_bf16.device != flat.device:
                raise RuntimeError("refresh(): flat is on %s, flat_bf16 on %s" % (flat.device, self.flat_bf16.device))
            call("prifit_pack_bf16_multi", m, nn_ops._ptr_array([w.src.W for w in ws]), (ctypes.c_int32 * m)(*[w.cout for w in ws]),
                 (ctypes.c_int32 * m)(*[w.cols for w in ws]), (ctypes.c_int32 * m)(*[w.src.W.stride(0) for w in ws]),
                 (ctypes.c_int32 * m)(*[w.order for w in ws]), nn_ops._ptr_array([w.W for w in ws]), cur_stream())
        return self

    # ------------------------------------------------------------------ the forward
    def forward(self, xyz, cls_label, fps_start=None, include_convex_loss=False, embed=False, **ignored_forward_kwargs):
        """xyz [B, C, N] (C = 6 with normals), cls_label [B, 1, 16] or [B, 16] one-hot -> the live model's eval-mode 5-tuple
        (seg [B,N,parts], (l1 [B,128,512], l2 [B,256,128], l3 [B,1024,1]), feat [B,128,N], zeros(1), zeros(1)); embed=True
        appends (None, None, feat_embed [B,128,N]) like the live model.  The other forward keywords of the live model
        (evaluation=..., quantile=..., ...) steer the fit path only and are ignored."""
        if include_convex_loss:
            raise ValueError("FrozenPartSeg has no fit path: include_convex_loss=True belongs to the live model")
        with torch.no_grad():
            return self._forward(xyz, cls_label, fps_start, embed)

    def predict(self, xyz, cls_label, fps_start=None):
        return self.forward(xyz, cls_label, fps_start)[0]

    def _trunk(self, xyz, cls_label, fps_start):
        """Everything in front of fp1, shared by forward() and labels(): the three set-abstraction levels, fp3 and fp2.
        -> (pts [B,N,C], l0_xyz, l1_xyz, skip [B,N,16+3+C], l1_up, l2_up, l3_points)."""
        self._bind()
        B, _, N = xyz.shape
        pts = xyz.permute(0, 2, 1).contiguous().float()
        l0_xyz = pts[:, :, :3].contiguous() if self.normal_channel else pts
        s1, s2 = fps_start if fps_start is not None else (None, None)
        l1_xyz, l1_points = self._sa_level(self._sa[0], l0_xyz, pts, s1)
        l2_xyz, l2_points = self._sa_level(self._sa[1], l1_xyz, l1_points, s2)
        # SA3 (group all): rows [xyz | feat | 0], three products, max over the cloud's points
        st, w0 = self._sa3
        S2 = l2_xyz.shape[1]
        rows = self._rows([l2_xyz, l2_points], B, S2, w0.W.shape[1])
        l3_points = torch.empty(B, st[-1].cout, dtype=torch.float32, device=pts.device)
        self._stack(rows, False, st, w0.W, S2, l3_points)
        l3_points = l3_points.reshape(B, 1, -1)
        l3_xyz = None                                                        # one centre per cloud: nothing to interpolate between
        l2_up = self._fp_level("fp3", l2_xyz, l3_xyz, l2_points, l3_points)
        l1_up = self._fp_level("fp2", l1_xyz, l2_xyz, l1_points, l2_up)
        onehot = cls_label.reshape(B, 1, 16).expand(B, N, 16).to(pts.dtype)
        skip = torch.cat([onehot, l0_xyz, pts], dim=-1)
        return pts, l0_xyz, l1_xyz, skip, l1_up, l2_up, l3_points

    def _forward(self, xyz, cls_label, fps_start, embed):
        B, _, N = xyz.shape
        pts, l0_xyz, l1_xyz, skip, l1_up, l2_up, l3_points = self._trunk(xyz, cls_label, fps_start)
        l0_up = self._fp_level("fp1", l0_xyz, l1_xyz, skip, l1_up)
        feat = torch.empty(B * N, self._head[0].cout, dtype=torch.float32, device=pts.device)
        self._stack(l0_up.reshape(B * N, -1), False, self._head, self._head[0].W, 0, feat)
        seg = F.log_softmax(self._linear(feat, self._conv2), dim=1).reshape(B, N, -1)
        zero = torch.zeros(2, device=pts.device)
        outs = (seg, (l1_up.permute(0, 2, 1), l2_up.permute(0, 2, 1), l3_points.permute(0, 2, 1)),
                feat.reshape(B, N, -1).permute(0, 2, 1), zero[:1], zero[1:])
        if embed:
            outs += (None, None, self._linear(feat, self._emb).reshape(B, N, -1).permute(0, 2, 1))
        return outs

    def _tail_shape(self):
        """(K0, widths) of the per-point tail; NotImplementedError where the row chain of this precision does not take it."""
        K0, widths = self._tail_kp, [ly.cout for ly in self._tail]
        L = len(widths)
        entry, stem, _ = _CHAINS[self.precision]["rows"]
        if not getattr(dll(), stem + "_supported")(K0, L, (ctypes.c_int32 * L)(*widths)):
            raise NotImplementedError("FrozenPartSeg.labels(): a tail of %d input columns and widths %s is outside "
                                      "%s (4 layers, 128 / 128 / 128 / at most 64 parts, at most 160 "
                                      "columns); there is no fall-back" % (K0, tuple(widths), entry))
        return K0, widths

    def labels(self, xyz, cls_label, shape_cat=None, cat_of_label=None, fps_start=None, return_scores=False):
        """Part labels straight from the frozen network: xyz [B, C, N], cls_label as forward() -> labels [B, N] int32, with
        return_scores=True also scores [B, N, num_parts], conv2's outputs BEFORE log_softmax (which moves no maximum).
        shape_cat int [B] (device or host) and cat_of_label int [num_parts] restrict each cloud's arg-max to the parts of
        its category, testing.py:141-144 -- an evaluation loop passes SegmentationEvaluator.cat_of_label and
        cat_of_label[target[:, 0]]; a cloud whose category has no part gets -1.  Both None: the arg-max over all parts.
        The first maximum wins, a NaN beats every number (prifit_seg_metrics' rules, bit for bit).
        forward()'s route up to fp1's rows, then ONE launch (_chain_rows) over fp1's two layers, conv1 + bn1
        and conv2: no [B N, 128] tensor, no log_softmax.  No fall-back: NotImplementedError for a tail the kernel refuses."""
        if (shape_cat is None) != (cat_of_label is None):
            raise ValueError("FrozenPartSeg.labels(): shape_cat and cat_of_label go together (both or neither)")
        if xyz.dim() != 3:
            raise ValueError("FrozenPartSeg.labels(): xyz must be [B, C, N], got %s" % (tuple(xyz.shape),))
        B, _, N = xyz.shape
        K0, widths = self._tail_shape()
        parts = widths[-1]
        if shape_cat is not None:
            shape_cat, cat_of_label = torch.as_tensor(shape_cat), torch.as_tensor(cat_of_label)
            for name, t, n in (("shape_cat", shape_cat, B), ("cat_of_label", cat_of_label, parts)):
                if t.dtype.is_floating_point or t.dtype == torch.bool or t.numel() != n:
                    raise ValueError("FrozenPartSeg.labels(): %s must hold %d integers, got %s %s"
                                     % (name, n, t.dtype, tuple(t.shape)))
        with torch.no_grad():
            pts, l0_xyz, l1_xyz, skip, l1_up, _, _ = self._trunk(xyz, cls_label, fps_start)
            dev = pts.device
            if shape_cat is not None:
                shape_cat = shape_cat.reshape(B).to(device=dev, dtype=torch.int32).contiguous()
                cat_of_label = cat_of_label.reshape(parts).to(device=dev, dtype=torch.int32).contiguous()
            rows = self._fp_rows("fp1", l0_xyz, l1_xyz, skip, l1_up, K0)
            out = torch.empty(B, N, dtype=torch.int32, device=dev)
            scores = torch.empty(B, N, parts, dtype=torch.float32, device=dev) if return_scores else None
            self._chain_rows(rows, K0, widths, scores, out, cat_of_label, shape_cat, N)
        return (out, scores) if return_scores else out

    def _embed_shape(self):
        """(K0, widths, parts) of the embedding chain -- fp1's two layers, conv1 + bn1, extra_conv_emb, and conv2 as the
        second head; NotImplementedError where the chain of this precision does not take it."""
        K0, widths, parts = self._tail_kp, [ly.cout for ly in self._tail[:-1]] + [self._emb.cout], self._conv2.cout
        L = len(widths)
        entry, stem, _ = _CHAINS[self.precision]["embed"]
        if self._emb.kin != widths[-2] or not getattr(dll(), stem + "_supported")(K0, L, (ctypes.c_int32 * L)(*widths), parts):
            raise NotImplementedError("FrozenPartSeg.embed(): a tail of %d input columns, widths %s and %d parts is outside "
                                      "%s (4 layers of 128, at most 64 parts, at most 160 columns); there is no "
                                      "fall-back" % (K0, tuple(widths), parts, entry))
        return K0, widths, parts

    def embed(self, xyz, cls_label, fps_start=None, l2_norm=None, shape_cat=None, cat_of_label=None, return_labels=False):
        """The per-point embedding the primitive fitting consumes: xyz [B, C, N], cls_label as forward() -> emb [B, N, 128]
        fp32, row-major and contiguous (the layout fit_ops.cluster / convex_loss work on), extra_conv_emb(relu(bn1(conv1(
        fp1(...))))); l2_norm=True divides every point's 128 channels by max(their 2-norm, 1e-12) (F.normalize), None takes the
        live model's `l2_norm`.  return_labels=True: (emb, labels [B, N] int32) from the SAME launch, labels as labels()
        gives them for (shape_cat, cat_of_label) -- both or neither.
        labels()'s route up to fp1's rows, then ONE launch (_chain_embed) over fp1's two layers, conv1 + bn1 and the two
        heads: no [B N, 128] tensor but the embedding itself.  No fall-back: NotImplementedError for a tail the kernel
        refuses."""
        if (shape_cat is None) != (cat_of_label is None):
            raise ValueError("FrozenPartSeg.embed(): shape_cat and cat_of_label go together (both or neither)")
        if shape_cat is not None and not return_labels:
            raise ValueError("FrozenPartSeg.embed(): shape_cat and cat_of_label restrict the labels: pass return_labels=True")
        if xyz.dim() != 3:
            raise ValueError("FrozenPartSeg.embed(): xyz must be [B, C, N], got %s" % (tuple(xyz.shape),))
        B, _, N = xyz.shape
        K0, widths, parts = self._embed_shape()
        if l2_norm is None:
            l2_norm = bool(getattr(self._source, "l2_norm", False))
        if shape_cat is not None:
            shape_cat, cat_of_label = torch.as_tensor(shape_cat), torch.as_tensor(cat_of_label)
            for name, t, n in (("shape_cat", shape_cat, B), ("cat_of_label", cat_of_label, parts)):
                if t.dtype.is_floating_point or t.dtype == torch.bool or t.numel() != n:
                    raise ValueError("FrozenPartSeg.embed(): %s must hold %d integers, got %s %s"
                                     % (name, n, t.dtype, tuple(t.shape)))
        with torch.no_grad():
            pts, l0_xyz, l1_xyz, skip, l1_up, _, _ = self._trunk(xyz, cls_label, fps_start)
            dev = pts.device
            if shape_cat is not None:
                shape_cat = shape_cat.reshape(B).to(device=dev, dtype=torch.int32).contiguous()
                cat_of_label = cat_of_label.reshape(parts).to(device=dev, dtype=torch.int32).contiguous()
            rows = self._fp_rows("fp1", l0_xyz, l1_xyz, skip, l1_up, K0)
            emb = torch.empty(B, N, widths[-1], dtype=torch.float32, device=dev)
            out = torch.empty(B, N, dtype=torch.int32, device=dev) if return_labels else None
            self._chain_embed(rows, K0, widths, parts, emb, bool(l2_norm), out, cat_of_label, shape_cat, N)
        return (emb, out) if return_labels else emb

    def probe_step(self, xyz, cls_label, target, fps_start=None):
        """One iteration of the classifier-layer pre-training (train_partseg_shapenet.py:56-99, `--init_cls`):
        xyz [B, C, N], cls_label as forward(), target [B, N] (or [B N]) int64 part labels -> a device tensor
        (loss, kept rows, correct rows) of the eval-mode network with the LIVE conv2 of the source model, and
        `conv2.weight.grad` / `conv2.bias.grad` of the source model = the gradient of that loss (allocated on first use,
        overwritten after); an optimizer over conv2's two parameters steps on them.  loss is get_loss on the log-probabilities
        (the softmax applied twice); -100 drops a point, any other label outside [0, parts) makes loss and gradient NaN.
        labels()'s route up to fp1's rows, then ONE launch pair (prifit_probe_head_f32): no [B N, 128] tensor, no scores, no
        autograd, no host read-back.  The folded copy of conv2 in the flat buffer is NOT kept up to date: refresh() after the
        last step.  fp32 only (NotImplementedError with precision="bf16", and for a tail the kernel refuses)."""
        if self.precision != "fp32":
            raise NotImplementedError("FrozenPartSeg.probe_step(): fp32 only, this module runs precision=%r" % self.precision)
        if xyz.dim() != 3:
            raise ValueError("FrozenPartSeg.probe_step(): xyz must be [B, C, N], got %s" % (tuple(xyz.shape),))
        B, _, N = xyz.shape
        if not torch.is_tensor(target) or target.dtype != torch.int64:
            raise ValueError("FrozenPartSeg.probe_step(): target must be an int64 tensor, got %s"
                             % (target.dtype if torch.is_tensor(target) else type(target).__name__))
        if tuple(target.shape) not in ((B, N), (B * N,)):
            raise ValueError("FrozenPartSeg.probe_step(): target must be [%d, %d], got %s" % (B, N, tuple(target.shape)))
        K0, widths = self._tail_kp, [ly.cout for ly in self._tail]
        L = len(widths)
        cw = (ctypes.c_int32 * L)(*widths)
        if not dll().prifit_probe_head_supported(K0, L, cw):
            raise NotImplementedError("FrozenPartSeg.probe_step(): a tail of %d input columns and widths %s is outside "
                                      "prifit_probe_head_f32; there is no fall-back" % (K0, tuple(widths)))
        conv2 = self._source.conv2
        w, b = conv2.weight, conv2.bias
        if b is None or w.dtype != torch.float32 or not w.is_contiguous() or w.device != self.flat.device:
            raise RuntimeError("FrozenPartSeg.probe_step(): conv2 of the source model must have a bias and contiguous fp32 "
                               "parameters on %s" % self.flat.device)
        for p in (w, b):
            gr = p.grad
            if gr is None or gr.dtype != torch.float32 or gr.shape != p.shape or not gr.is_contiguous() or gr.data_ptr() % 16:
                p.grad = torch.empty_like(p, memory_format=torch.contiguous_format)
        with torch.no_grad():
            pts, l0_xyz, l1_xyz, skip, l1_up, _, _ = self._trunk(xyz, cls_label, fps_start)
            dev = pts.device
            rows = self._fp_rows("fp1", l0_xyz, l1_xyz, skip, l1_up, K0)
            tgt = target.to(dev).reshape(B * N).contiguous()
            P, kin = B * N, widths[-2]
            Ws = [self._tail_w0.W] + [ly.W for ly in self._tail[1:-1]] + [w.detach()]
            lds = [self._tail_w0.W.stride(0)] + [ly.ldw for ly in self._tail[1:-1]] + [kin]
            bs = [ly.b for ly in self._tail[:-1]] + [b.detach()]
            out = torch.empty(4, dtype=torch.float32, device=dev)
            ws = torch.empty(dll().prifit_probe_head_workspace(P, K0, L, cw), dtype=torch.float32, device=dev)
            flops = 2.0 * P * (sum(k * c for k, c in zip([K0] + widths[:-1], widths)) + kin * widths[-1])
            with profiler.span(profiler.tag("probe_head", P, K0, *widths), flops):
                call("prifit_probe_head_f32", ptr(rows), _LL(K0), _LL(P), K0, L, cw, nn_ops._ptr_array(Ws), (ctypes.c_longlong * L)(*lds),
                     nn_ops._ptr_array(bs), ptr(tgt), ptr(w.grad), _LL(kin), ptr(b.grad), ptr(out), ptr(ws), cur_stream())
        return out[:3]

    def _rows(self, parts, B, n, kp):
        """[B n, kp] rows = the parts side by side, zero padded (the zeros are the flat buffer's: no fill launch)."""
        have = sum(p.shape[-1] for p in parts)
        if kp > have:
            parts = parts + [self._zeros[:kp - have].expand(B, n, kp - have)]
        return torch.cat(parts, dim=-1).reshape(B * n, kp)

    def _linear(self, x, ly):
        P = x.shape[0]
        y = torch.empty(P, ly.cout, dtype=torch.float32, device=x.device)
        nn_ops.gemm(nn_ops.NT, P, ly.cout, ly.kin, x, x.stride(0), ly.W, ly.ldw, y, ly.cout, bias=ly.b)
        return y

    def _stack(self, x, preact, layers, w0, pool_K, out):
        """relu(W' . + b') layer after layer on the product kernel, then the max over each pool_K rows (0: none) into
        `out` ([G, C] column window or [P, C]).  preact: x already is layer 0's pre-activation.  The ReLU of a layer is
        applied when the next product loads it (a_affine with unit scale) and by the pool / affine launch at the end."""
        P = x.shape[0]
        unit = None
        for l, ly in enumerate(layers):
            if l == 0 and preact:
                y = x
            else:
                W = w0 if l == 0 else ly.W
                Kin = W.shape[1] if l == 0 else ly.kin
                y = torch.empty(P, ly.cout, dtype=torch.float32, device=x.device)
                nn_ops.gemm(nn_ops.NT, P, ly.cout, Kin, x, x.stride(0), W, W.stride(0), y, ly.cout, a_affine=unit, bias=ly.b)
            x, unit = y, (self._ones, self._zeros)
        C = x.shape[1]
        if pool_K:
            G = P // pool_K
            arg = torch.empty(G, C, dtype=torch.int32, device=x.device)     # the pool launch's required output; never read
            call("prifit_pool_fwd", ptr(x), _LL(x.stride(0)), ptr(self._ones), ptr(self._zeros), G, pool_K, C, 0, ctypes.c_float(0.0),
                 ptr(out), _LL(out.stride(0)), ptr(arg), cur_stream())
        else:
            call("prifit_affine_relu", ptr(x), _LL(x.stride(0)), ptr(self._ones), ptr(self._zeros), P, C, 0, ctypes.c_float(0.0),
                 ptr(out), _LL(out.stride(0)), cur_stream())

    def _sa_level(self, lv, xyz, feats, fps_start):
        """One multi-scale set-abstraction level: xyz [B,N,3], feats [B,N,D] -> (new_xyz [B,S,3], out [B,S,sum C2])."""
        B, N, _ = xyz.shape
        S, radii, nsamples, D = lv["npoint"], lv["radii"], lv["nsamples"], lv["D"]
        scales = lv["scales"]
        R = len(scales)
        widths = [st[0].cout for st, _ in scales]
        if feats.shape[-1] != D:
            raise ValueError("FrozenPartSeg: %d point channels, the frozen model takes %d" % (feats.shape[-1], D))
        if not nn_ops.sa_group_supported(N, nsamples, widths):
            raise NotImplementedError("FrozenPartSeg: clouds of %d points are outside prifit_sa_group_linear_fwd (N <= 2048)" % N)
        _, new_xyz = ops.farthest_point_sample(xyz, S, fps_start, return_xyz=True)
        dev = xyz.device
        bs = [st[0].b for st, _ in scales]
        Ws = Us = Vcs = None
        direct = len(scales[0][1]) == 1
        if direct:
            Ws = [first[0].W for _, first in scales]
        else:
            kp = scales[0][1][0].W.shape[1]
            rows = self._rows([feats, xyz], B, N, kp)
            c4 = self._rows([new_xyz], B, S, 4)
            Us, Vcs = [], []
            for (st, (w_pt, w_c)), C1 in zip(scales, widths):
                U = torch.empty(B * N, C1, dtype=torch.float32, device=dev)
                Vc = torch.empty(B * S, C1, dtype=torch.float32, device=dev)
                nn_ops.gemm(nn_ops.NT, B * N, C1, kp, rows, kp, w_pt.W, kp, U, C1)
                nn_ops.gemm(nn_ops.NT, B * S, C1, 4, c4, 4, w_c.W, 4, Vc, C1)
                Us.append(U)
                Vcs.append(Vc)
        Ys = [torch.empty(B * S * k, c, dtype=torch.float32, device=dev) for k, c in zip(nsamples, widths)]
        idxs = [torch.empty(B, S, k, dtype=torch.int32, device=dev) for k in nsamples]
        pa = nn_ops._ptr_array
        with profiler.span("sa_group_linear"):
            call("prifit_sa_group_linear_fwd", ptr(xyz), ptr(new_xyz), B, N, S, R,
                 (ctypes.c_float * R)(*[float(np.float32(r ** 2)) for r in radii]), (ctypes.c_int * R)(*[int(k) for k in nsamples]),
                 (ctypes.c_int * R)(*widths), 0 if direct else 1, ptr(feats) if direct else None, D if direct else 0, 1,
                 int(direct and D == 3 and feats.data_ptr() == xyz.data_ptr()), pa(Ws) if direct else None, None if direct else pa(Us),
                 None if direct else pa(Vcs), pa(bs), pa(Ys), pa([None] * R), pa(idxs), cur_stream())
        outw = [st[-1].cout for st, _ in scales]
        wide = torch.empty(B * S, sum(outw), dtype=torch.float32, device=dev)
        c0 = 0
        for si, ((st, _), K, Y, C2) in enumerate(zip(scales, nsamples, Ys, outw)):
            win = wide[:, c0:c0 + C2]
            c0 += C2
            if not self._chain_pool(st, lv["bf16"][si] if self._bf16 else (None, None), Y, B * S, K, win, wide.stride(0)):
                self._stack(Y, True, st, None, K, win)
        return new_xyz, wide.reshape(B, S, -1)

    def _chain_pool(self, st, bf16, Y, G, K, win, ldo):
        """Layers 2 + 3 + pool of scale `st` on its first-layer rows Y [G K, C0] in one launch -> win [G, C2] of pitch ldo; False
        (fp32) or NotImplementedError (bf16) where the chain does not take the scale."""
        chain = _CHAINS[self.precision]
        entry, stem, tag = chain["pool"]
        C0, C1, C2 = (ly.cout for ly in st)
        if not query(stem + "_supported", C0, C1, C2, K):
            if chain["pool_fallback"]:
                return False
            raise NotImplementedError("FrozenPartSeg(precision=%r): a scale of widths (%d, %d, %d) over %d samples is "
                                      "outside %s; there is no fall-back" % (self.precision, C0, C1, C2, K, entry))
        (W1, ld1), (W2, ld2) = (chain["weight"](ly, w) for ly, w in zip(st[1:], bf16))
        nws = query(stem + "_workspace", G, K, C0, C1, C2)
        ws = torch.empty(nws, dtype=torch.float32, device=Y.device) if nws else None
        with profiler.span(profiler.tag(tag, G * K, C0, C1, C2), 2.0 * G * K * (C0 * C1 + C1 * C2)):
            call(entry, ptr(Y), _LL(C0), G, K, C0, C1, C2, ptr(W1), _LL(ld1), ptr(st[1].b), ptr(W2), _LL(ld2), ptr(st[2].b),
                 ptr(win), _LL(ldo), ptr(ws), cur_stream())
        return True

    def _chain_rows(self, rows, K0, widths, scores, labels, cat_of_label, shape_cat, N):
        """The per-point tail on fp1's rows [P, K0] in one launch: scores [.., parts] (None: not wanted) and labels."""
        chain = _CHAINS[self.precision]
        entry, stem, tag = chain["rows"]
        P, L = rows.shape[0], len(widths)
        bf16 = self._tail_bf16 if self._bf16 else [None] * L
        Ws, lds = zip(*(chain["weight"](ly, w) for ly, w in zip([self._tail_w0] + self._tail[1:], bf16)))
        nws = getattr(dll(), stem + "_workspace")(P, K0, L, (ctypes.c_int32 * L)(*widths))
        ws = torch.empty(nws, dtype=torch.float32, device=rows.device) if nws else None
        flops = 2.0 * P * sum(k * c for k, c in zip([K0] + widths[:-1], widths))
        with profiler.span(profiler.tag(tag, P, K0, *widths), flops):
            call(entry, ptr(rows), _LL(K0), _LL(P), K0, L, (ctypes.c_int32 * L)(*widths), nn_ops._ptr_array(list(Ws)),
                 (ctypes.c_longlong * L)(*lds), nn_ops._ptr_array([ly.b for ly in self._tail]), ptr(scores), _LL(widths[-1]),
                 ptr(labels), ptr(cat_of_label), ptr(shape_cat), N, ptr(ws), cur_stream())

    def _chain_embed(self, rows, K0, widths, parts, emb, normalize, labels, cat_of_label, shape_cat, N):
        """fp1's rows [P, K0] -> emb [.., 128] (unit rows with `normalize`) and, with `labels`, conv2's restricted arg-max, in
        one launch: layers 1 .. 3 of the tail, then extra_conv_emb and (labels only) conv2 on the same registers."""
        chain = _CHAINS[self.precision]
        entry, stem, tag = chain["embed"]
        P, L = rows.shape[0], len(widths)
        layers = [self._tail_w0] + self._tail[1:-1] + [self._emb, self._conv2]
        bf16 = self._tail_bf16[:-1] + self._emb_bf16 + self._tail_bf16[-1:] if self._bf16 else [None] * (L + 1)
        Ws, lds = zip(*(chain["weight"](ly, w) for ly, w in zip(layers, bf16)))
        CL = parts if labels is not None else 0
        cw = (ctypes.c_int32 * L)(*widths)
        nws = getattr(dll(), stem + "_workspace")(P, K0, L, cw, CL)
        ws = torch.empty(nws, dtype=torch.float32, device=rows.device) if nws else None
        flops = 2.0 * P * (sum(k * c for k, c in zip([K0] + widths[:-1], widths)) + widths[-2] * CL)
        with profiler.span(profiler.tag(tag, P, K0, *widths, CL), flops):
            call(entry, ptr(rows), _LL(K0), _LL(P), K0, L, cw, nn_ops._ptr_array(list(Ws[:L])), (ctypes.c_longlong * L)(*lds[:L]),
                 nn_ops._ptr_array([ly.b for ly in self._tail[:-1]] + [self._emb.b]), ptr(Ws[L]) if CL else None, _LL(lds[L]),
                 ptr(self._conv2.b) if CL else None, CL, ptr(emb), _LL(emb.stride(-2)), int(normalize), None, _LL(0), ptr(labels),
                 ptr(cat_of_label), ptr(shape_cat), N, ptr(ws), cur_stream())

    def _fp_level(self, name, xyz1, xyz2, points1, points2):
        """Feature propagation: xyz1 [B,N,3], xyz2 [B,S,3] (None: S == 1), points1 [B,N,D1], points2 [B,S,D2] -> [B,N,C]."""
        st, w0, _, _ = self._fp[name]
        B, N, _ = xyz1.shape
        rows = self._fp_rows(name, xyz1, xyz2, points1, points2, w0.W.shape[1])
        out = torch.empty(B * N, st[-1].cout, dtype=torch.float32, device=xyz1.device)
        self._stack(rows, False, st, w0.W, 0, out)
        return out.reshape(B, N, -1)

    def _fp_rows(self, name, xyz1, xyz2, points1, points2, kp):
        """The input rows of a feature-propagation stack, [B N, kp] = [interpolated (D2) | points1 (D1) | 0]: 3-NN and one launch."""
        _, _, D1, D2 = self._fp[name]
        B, N, _ = xyz1.shape
        S = points2.shape[1]
        idx = w = None
        if S > 1:
            idx, w = ops.three_nn(xyz1, xyz2)
        points1, points2 = points1.contiguous(), points2.contiguous()
        rows = torch.empty(B * N, kp, dtype=torch.float32, device=xyz1.device)
        call("prifit_fp_rows", ptr(points2), ptr(idx), ptr(w), ptr(points1), B, N, S, D2, D1, kp, ptr(rows), cur_stream())
        return rows


def freeze(model, precision="fp32"):
    """A FrozenPartSeg of `model` (a models.pointnet2_part_seg_msg.get_model on the GPU, reconstruct=False); TypeError for
    every other network.  precision: "fp32" or "bf16" (the on-chip chains in bf16 with fp32 accumulation);
    ValueError for anything else."""
    return FrozenPartSeg(model, precision)

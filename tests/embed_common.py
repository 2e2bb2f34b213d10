"""Helpers of the embedding-chain tests (prifit_mlp_chain_embed_f32 / _bf16, FrozenPartSeg.embed): the seeded net of the label
tests with a 128-wide fifth weight, the fp64 restatement of the chain with its normalisation, the integer layers and the bf16
forward bound of the bf16 tests (re-stated: a test module is not imported), the device side of a launch in guard bands, and the
seeded end-to-end model.  No test lives here; nothing here needs a GPU until a function that launches is called."""
import ctypes

import numpy as np
import torch

U = 2.0 ** -23             # one ulp at 1 in fp32
R16 = 2.0 ** -9            # unit roundoff of bf16
U32 = 2.0 ** -24           # of fp32
W_HID = 128
EPS = 1e-12                # F.normalize's
CASES = [(152, 50), (160, 64), (8, 0), (64, 33), (152, 1)]      # (K0, C_L); C_L = 0: no head A
ROWS = [200, 1]            # 200: seven waves, the last with 8 live rows; 1: a lone live row
GUARD = 1 << 14


def arr(ctype, vals):
    return (ctype * len(vals))(*vals)


# ---------------------------------------------------------------------------------------------- nets
def seeded_net(P, K0, CL, seed):
    """Seeded normal rows and weights: X [P, K0], Ws / bs of widths (128, 128, 128, CL, 128) -- the label tests' net and a
    fifth, 128-wide weight on the third layer's output (W_e).  CL = 0: the fourth entry is None."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((P, K0)).astype(np.float32)
    Ws, bs = [], []
    for l, cout in enumerate((W_HID, W_HID, W_HID, CL, W_HID)):
        kin = W_HID if l else K0
        Ws.append((rng.standard_normal((cout, kin)) / np.sqrt(kin)).astype(np.float32) if cout else None)
        bs.append((0.1 * rng.standard_normal(cout)).astype(np.float32) if cout else None)
    return X, Ws, bs


def int_layer(rng, cout, K):
    """Two non-zeros in {-1, +1} per row, at columns c % K and (5c + 3) % K (moved by one where they coincide); bias in {-1, 0, 1}."""
    W = np.zeros((cout, K), dtype=np.int64)
    c = np.arange(cout)
    k1, k2 = c % K, (5 * c + 3) % K
    k2 = np.where(k2 == k1, (k2 + 1) % K, k2)
    W[c, k1] = rng.choice([-1, 1], cout)
    W[c, k2] = rng.choice([-1, 1], cout)
    return W, rng.integers(-1, 2, cout)


def int_net(P, K0, CL):
    """Integer rows in [-3, 3] and integer layers of widths (128, 128, 128, CL, 128): |a_l| <= 2^(l + 3) - 1, so a_3 <= 31,
    e and z <= 63 -- exact in bf16 and in every fp32 partial sum.  -> X, Ws, bs, a_3, z (None without head A), e (int64)."""
    rng = np.random.default_rng(0)
    a = X = rng.integers(-3, 4, (P, K0))
    Ws, bs, kin = [], [], K0
    for l in range(3):
        W, b = int_layer(rng, W_HID, kin)
        Ws.append(W)
        bs.append(b)
        a = np.maximum(a @ W.T + b, 0)
        assert np.abs(a).max() <= 2 ** (l + 3) - 1
        kin = W_HID
    z = None
    if CL:
        W, b = int_layer(rng, CL, W_HID)
        z = a @ W.T + b
    else:
        W = b = None
    Ws.append(W)
    bs.append(b)
    W, b = int_layer(rng, W_HID, W_HID)
    Ws.append(W)
    bs.append(b)
    e = a @ W.T + b
    assert np.abs(e).max() <= 63
    return X, Ws, bs, a, z, e


def nonzero_enough(ref):
    share = float(np.count_nonzero(ref)) / ref.size
    assert share >= 0.5, "the integer reference is %.0f %% zeros: it would pass a kernel that computes nothing" % (100 * (1 - share))


# ---------------------------------------------------------------------------------------------- fp64 restatement
def fold64(W, b, gamma, beta, mean, var, eps):
    """conv1x1 + eval-mode BatchNorm as one affine, in fp64: W' = s W, b' = (b - mean) s + beta, s = gamma / sqrt(var + eps)."""
    s = gamma / np.sqrt(var + eps)
    return W * s[:, None], (b - mean) * s + beta


def trunk64(X, Ws, bs):
    """a_3 = relu(W_3 relu(W_2 relu(W_1 x + b_1) + b_2) + b_3) in fp64 (np.maximum: a NaN stays)."""
    a = np.asarray(X, dtype=np.float64)
    for W, b in zip(Ws[:3], bs[:3]):
        a = np.maximum(a @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64), 0.0)
    return a


def head64(a, W, b):
    """-> (W a + b, sum_k |a_k| |w_k| + |b|): the product and what one rounding of it is relative to."""
    W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a @ W.T + b, np.abs(a) @ np.abs(W).T + np.abs(b)


def normalize64(e):
    """F.normalize(e, p=2, dim=-1) -> (e / max(||e||, 1e-12), ||e|| [.., 1])."""
    n = np.sqrt(np.sum(e * e, axis=-1, keepdims=True))
    return e / np.maximum(n, EPS), n


def embed64(X, Ws, bs, normalize):
    """The embedding chain in fp64 on (folded) weights (128, 128, 128, [C_L], 128) -> (emb, scale): with `normalize` both
    divided by max(the fp64 norm, 1e-12)."""
    e, scale = head64(trunk64(X, Ws, bs), Ws[-1], bs[-1])
    if normalize:
        en, n = normalize64(e)
        return en, scale / np.maximum(n, EPS)
    return e, scale


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def layer_bound(a, E, W, b):
    """One chained bf16 layer: `a` the exact input (fp64) and E >= |computed input - a| before its rounding -> the bound on
    |computed pre-activation - (W a + b)|.  Rounding the input: E' = E + 2^-9 (|a| + E).  Rounding the weight: 2^-9 |w|.
    So the product is off by at most |W| (1 + 2^-9) E' + 2^-9 |W| |a|, and the fp32 accumulation of K products and the bias
    by (K + 2) 2^-24 (sum |a^| |w^| + |b|)."""
    K = W.shape[1]
    aw = np.abs(W)
    Er = E * (1.0 + R16) + R16 * np.abs(a)
    mag = ((np.abs(a) + Er) @ aw.T) * (1.0 + R16) + np.abs(b)
    return (Er @ aw.T) * (1.0 + R16) + R16 * (np.abs(a) @ aw.T) + (K + 2) * U32 * mag


def chain64(a, Ws, bs):
    """The layers in fp64 (ReLU between them, none after the last) -> (pre-activation of the last layer, its bf16 bound)."""
    a = np.asarray(a, dtype=np.float64)
    E = np.zeros_like(a)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)
        z, E = a @ W.T + b, layer_bound(a, E, W, b)
        if l == len(Ws) - 1:
            return z, E
        a = np.maximum(z, 0.0)                                               # 1-Lipschitz: E carries over


def normalize_f32_bound(e):
    """e: fp32 values as fp64 -> (e / max(||e||, 1e-12) in fp64, the bound on what an fp32 evaluation of it may differ by).
    The fp32 sum of 128 non-negative squares, in any order, is off by at most (1 + 2^-24)^128 - 1 < 129 2^-24 relative (one
    rounding per square, at most 127 per add chain), its square root by half of that plus one rounding, the quotient by one
    more: under 67 roundings in all; 70 2^-24 |result| bounds it.  (The chain's worst-case bf16 bound on e itself exceeds
    ||e||, so no bound on the normalised vector follows from it: the normalisation is checked on the kernel's own e.)"""
    en, _ = normalize64(e)
    return en, 70 * U32 * np.abs(en)


# ---------------------------------------------------------------------------------------------- device side
def _gc():
    import guard_common
    return guard_common


def dev(a):
    """A host array in NaN guards on the device."""
    GC = _gc()
    return GC.guarded_like(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda(), GUARD, GUARD)[0]


def dev_rows(X, gap=4):
    """X [P, K] with a row stride of K + gap, NaN in the gap and in the guards."""
    GC = _gc()
    view, _ = GC.guarded_matrix(X.shape[0], X.shape[1], X.shape[1] + gap, GUARD, GUARD)
    view.copy_(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda())
    return view


def pack_bf16(ws, orders):
    """prifit_pack_bf16_multi over fp32 device matrices -> int16 views [rows, cols rounded up to 16]."""
    from prifit_amd._lib import call, cur_stream
    GC = _gc()
    up16 = lambda k: (k + 15) // 16 * 16
    outs = [GC.guarded((w.shape[0] * up16(w.shape[1]) // 2,), 4096, 4096, poison=GC.SENTINEL) for w in ws]
    n = len(ws)
    call("prifit_pack_bf16_multi", n, arr(ctypes.c_void_p, [w.data_ptr() for w in ws]), arr(ctypes.c_int32, [w.shape[0] for w in ws]),
         arr(ctypes.c_int32, [w.shape[1] for w in ws]), arr(ctypes.c_int32, [w.stride(0) for w in ws]), arr(ctypes.c_int32, orders),
         arr(ctypes.c_void_p, [o[0].data_ptr() for o in outs]), cur_stream())
    torch.cuda.synchronize()
    for view, base in outs:
        GC.assert_guards_intact(base, view)
    return [view.view(torch.int16).view(w.shape[0], up16(w.shape[1])) for (view, _), w in zip(outs, ws)]


class EmbedNet:
    """A net of widths (128, 128, 128, [C_L], 128) on the device for one pipe ("f32" / "bf16"): rows in a NaN-gapped matrix,
    weights in NaN guards (bf16: packed by the library, W_1 plain, the others in the accumulator order), fp32 biases in NaN
    guards.  launch() is prifit_mlp_chain_embed_*, rows_launch() prifit_mlp_chain_rows_* on (W_1, W_2, W_3, W_cls)."""

    def __init__(self, pipe, Xn, Wn, bn):
        assert pipe in ("f32", "bf16") and len(Wn) == 5
        self.pipe, (self.P, self.K0) = pipe, Xn.shape
        self.CL = 0 if Wn[3] is None else Wn[3].shape[0]
        self.X = dev_rows(Xn)
        have = [i for i in range(5) if Wn[i] is not None]
        W = [dev(Wn[i]) for i in have]
        if pipe == "bf16":
            W = pack_bf16(W, [0] + [1] * (len(have) - 1))
        self.W, self.b = [None] * 5, [None] * 5
        for i, w in zip(have, W):
            self.W[i], self.b[i] = w, dev(bn[i])

    def outputs(self, lde=W_HID, scores=False, labels=False, lds=None):
        """(emb, scores, labels-as-float) views with their bases, all SENTINEL (a NaN): an unwritten element shows."""
        GC = _gc()
        out = {"emb": GC.guarded_matrix(self.P, W_HID, lde, 4096, 4096, poison=GC.SENTINEL)}
        if scores:
            out["scores"] = GC.guarded_matrix(self.P, self.CL, lds or self.CL, 4096, 4096, poison=GC.SENTINEL)
        if labels:
            out["labels"] = GC.guarded((self.P,), 4096, 4096, poison=GC.SENTINEL)
        return out

    def raw(self, out, normalize, head=True, cat_of_label=None, shape_cat=None, N=None, **over):
        """One call of the entry point -> its return code; `over` replaces arguments by name (the argument-check test)."""
        from prifit_amd._lib import cur_stream, dll
        p = lambda t: None if t is None else t.data_ptr()
        first = lambda k: None if k not in out else out[k][0]
        CL = self.CL if head else 0
        main = [0, 1, 2, 4]
        a = dict(X=p(self.X), ldx=self.X.stride(0), P=self.P, K0=self.K0, L=4, widths=arr(ctypes.c_int32, [W_HID] * 4),
                 W=arr(ctypes.c_void_p, [p(self.W[i]) for i in main]), ldw=arr(ctypes.c_longlong, [self.W[i].stride(0) for i in main]),
                 b=arr(ctypes.c_void_p, [p(self.b[i]) for i in main]), W_cls=p(self.W[3]) if CL else None,
                 ldw_cls=self.W[3].stride(0) if CL else 0, b_cls=p(self.b[3]) if CL else None, CL=CL, emb=p(first("emb")),
                 lde=out["emb"][0].stride(0), normalize=int(normalize), scores=p(first("scores")),
                 lds=out["scores"][0].stride(0) if "scores" in out else 0, labels=p(first("labels")), cat=p(cat_of_label),
                 shape_cat=p(shape_cat), N=self.P if N is None else N, ws=None, stream=cur_stream())
        a.update(over)
        return getattr(dll(), "prifit_mlp_chain_embed_" + self.pipe)(*a.values())

    def launch(self, normalize, lde=W_HID, scores=False, labels=False, head=True, lds=None, **kw):
        """-> (emb [P, 128], scores or None, labels int32 or None) on the device; every guard checked."""
        GC = _gc()
        head = bool(head and self.CL > 0 and (scores or labels))      # head A: only when one of its outputs is asked for
        out = self.outputs(lde, scores and head, labels and head, lds)
        rc = self.raw(out, normalize, head=head, **kw)
        torch.cuda.synchronize()
        assert rc == 0, rc
        for view, base in out.values():
            GC.assert_guards_intact(base, view)
        lab = out["labels"][0].view(torch.int32) if "labels" in out else None
        return out["emb"][0], (out["scores"][0] if "scores" in out else None), lab

    def rows_launch(self, scores=True, labels=True, cat_of_label=None, shape_cat=None, N=None, lds=None):
        """prifit_mlp_chain_rows_* on the same operands -> (scores or None, labels or None)."""
        from prifit_amd._lib import call, cur_stream
        GC = _gc()
        p = lambda t: None if t is None else t.data_ptr()
        s = l = None
        if scores:
            s, s_base = GC.guarded_matrix(self.P, self.CL, lds or self.CL, 4096, 4096, poison=GC.SENTINEL)
        if labels:
            l, l_base = GC.guarded((self.P,), 4096, 4096, poison=GC.SENTINEL)
        W, b = self.W[:4], self.b[:4]
        call("prifit_mlp_chain_rows_" + self.pipe, p(self.X), self.X.stride(0), self.P, self.K0, 4,
             arr(ctypes.c_int32, [W_HID] * 3 + [self.CL]), arr(ctypes.c_void_p, [p(w) for w in W]),
             arr(ctypes.c_longlong, [w.stride(0) for w in W]), arr(ctypes.c_void_p, [p(x) for x in b]), p(s),
             0 if s is None else s.stride(0), p(l), p(cat_of_label), p(shape_cat), self.P if N is None else N, None, cur_stream())
        torch.cuda.synchronize()
        if scores:
            GC.assert_guards_intact(s_base, s)
        if labels:
            GC.assert_guards_intact(l_base, l)
        return s, (None if l is None else l.view(torch.int32))


def separate_route(X, Ws, bs, normalize):
    """The launches the chain replaces, as FrozenPartSeg._stack / _linear run them, with W_e as the last product: fp1's two
    products (the second with the ReLU on load through the unit a_affine) and the ReLU launch, conv1 + bn1 and its ReLU
    launch, extra_conv_emb as a plain product; then F.normalize on the device."""
    from prifit_amd import nn_ops
    P = X.shape[0]
    ones, zeros = torch.ones(W_HID, device="cuda"), torch.zeros(W_HID, device="cuda")

    def product(x, W, b, unit):
        y = torch.empty(P, W.shape[0], dtype=torch.float32, device="cuda")
        nn_ops.gemm(nn_ops.NT, P, W.shape[0], W.shape[1], x, x.stride(0), W, W.stride(0), y, W.shape[0],
                    a_affine=(ones, zeros) if unit else None, bias=b)
        return y

    h = product(X, Ws[0], bs[0], False)
    h = torch.relu(product(h, Ws[1], bs[1], True))
    h = torch.relu(product(h, Ws[2], bs[2], False))
    e = product(h, Ws[-1], bs[-1], False)
    return torch.nn.functional.normalize(e, p=2, dim=1) if normalize else e


# ---------------------------------------------------------------------------------------------- end to end
def seeded_model(normal, seed, l2_norm=False):
    """get_model(50) with seeded weights, BatchNorm gamma / beta and running statistics, all drawn on the CPU."""
    from prifit_amd.models import pointnet2_part_seg_msg as M
    torch.manual_seed(seed)
    net = M.get_model(50, normal_channel=normal, l2_norm=l2_norm)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
    return net.cuda().eval()


def inputs(B, C, N, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(B, C, N, generator=g) * 2 - 1).cuda()
    onehot = torch.eye(16)[torch.randint(0, 16, (B,), generator=g)].reshape(B, 1, 16).cuda()
    start = (torch.randint(0, N, (B,), generator=g).cuda(), torch.randint(0, 512, (B,), generator=g).cuda())
    return xyz, onehot, start


def spy_calls(monkeypatch_ctx, seen):
    """Record the name of every entry point the frozen module launches."""
    import prifit_amd.inference as I
    import prifit_amd.models.pointnet_util as PU
    import prifit_amd.nn_ops as NN
    import prifit_amd.ops as O
    from prifit_amd import _lib

    def spy(name, *a):
        seen.append(name)
        return _lib.call(name, *a)

    for mod in (I, PU, NN, O):
        monkeypatch_ctx.setattr(mod, "call", spy)

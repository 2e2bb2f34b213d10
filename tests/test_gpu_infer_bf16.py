"""GPU: frozen inference in bf16 (FrozenPartSeg(model, precision="bf16"), csrc/infer_bf16.hip) -- the bf16 weight pack against
tensor.to(torch.bfloat16) bit for bit, the two chains on integer data against an int64 numpy evaluation with no tolerance,
on real data against fp64 within a forward error bound the test derives itself, NaN rows and masked k-steps, the labels
against prifit_seg_metrics on the kernel's own scores, and the module end to end against an fp64 run of the folded network
with a CPU bf16 emulation as the yardstick.  Every tensor a kernel reads or writes sits in guard bands."""
import ctypes

import numpy as np
import pytest
import torch

import guard_common as GC

pytestmark = pytest.mark.gpu

R16 = 2.0 ** -9            # unit roundoff of bf16 (8 significant bits, round to nearest)
U32 = 2.0 ** -24           # of fp32
POOL_CASES = [(32, 32, 64, 32, 3), (64, 64, 128, 64, 3), (64, 96, 128, 128, 3), (128, 128, 256, 64, 3), (128, 196, 256, 128, 3),
              (32, 32, 64, 32, 5)]                       # (C0, C1, C2, pool_K, G); G = 5 at pool_K = 32: a partial workgroup
ROWS_CASES = [(152, 50), (160, 64), (152, 1), (8, 50), (64, 33)]      # (K0, C_L)
ROWS_P = [200, 1]
GUARD = 1 << 14


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _up16(k):
    return (k + 15) // 16 * 16


def _src_col(p, order):
    """The input channel that column p of a packed row holds (include/prifit_hip.h, prifit_pack_bf16_multi)."""
    e, h = p & 7, (p >> 3) & 1
    return (p & ~15) + 8 * (e >> 2) + 4 * h + (e & 3) if order else p


def _pack(ws, orders, cols=None):
    """prifit_pack_bf16_multi over fp32 device matrices (row stride = their own) -> int16 views [rows, ldk], each in
    sentinel guards that are checked here."""
    from prifit_amd._lib import call, cur_stream
    cols = [w.shape[1] for w in ws] if cols is None else cols
    outs = [GC.guarded((w.shape[0] * _up16(c) // 2,), 4096, 4096, poison=GC.SENTINEL) for w, c in zip(ws, cols)]
    n = len(ws)
    call("prifit_pack_bf16_multi", n, _arr(ctypes.c_void_p, [w.data_ptr() for w in ws]), _arr(ctypes.c_int32, [w.shape[0] for w in ws]),
         _arr(ctypes.c_int32, cols), _arr(ctypes.c_int32, [w.stride(0) for w in ws]), _arr(ctypes.c_int32, orders),
         _arr(ctypes.c_void_p, [o[0].data_ptr() for o in outs]), cur_stream())
    torch.cuda.synchronize()
    for view, base in outs:
        GC.assert_guards_intact(base, view)
    return [view.view(torch.int16).view(w.shape[0], _up16(c)) for (view, _), w, c in zip(outs, ws, cols)]


def _dev(a):
    """A host array in NaN guards on the device."""
    return GC.guarded_like(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda(), GUARD, GUARD)[0]


def _dev_rows(X, gap=4):
    """X [P, K] with a row stride of K + gap, NaN in the gap and in the guards: what lies behind a row's extent is poison."""
    view, _ = GC.guarded_matrix(X.shape[0], X.shape[1], X.shape[1] + gap, GUARD, GUARD)
    view.copy_(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda())
    return view


def _pool_launch(Xn, W1n, b1n, W2n, b2n, K, ld_gap=0):
    """The pooled bf16 chain on host arrays -> out [G, C2] (numpy fp32); guards asserted."""
    from prifit_amd._lib import call, cur_stream
    (C1, C0), C2 = W1n.shape, W2n.shape[0]
    G = Xn.shape[0] // K
    X, b1, b2 = _dev_rows(Xn), _dev(b1n), _dev(b2n)
    W1, W2 = _pack([_dev(W1n), _dev(W2n)], [0, 1])
    out, base = GC.guarded_matrix(G, C2, C2 + ld_gap, 4096, 4096, poison=GC.SENTINEL)
    call("prifit_mlp_chain_pool_bf16", X.data_ptr(), X.stride(0), G, K, C0, C1, C2, W1.data_ptr(), W1.stride(0), b1.data_ptr(),
         W2.data_ptr(), W2.stride(0), b2.data_ptr(), out.data_ptr(), out.stride(0), None, cur_stream())
    torch.cuda.synchronize()
    GC.assert_guards_intact(base, out)
    return out.cpu().numpy()


class _RowsNet:
    """A tail on the device: rows in a NaN-gapped matrix, bf16 weights packed by the library, fp32 biases in NaN guards."""

    def __init__(self, Xn, Wn, bn):
        self.P, self.K0 = Xn.shape
        self.CL = Wn[-1].shape[0]
        self.X = _dev_rows(Xn)
        self.W = _pack([_dev(w) for w in Wn], [0, 1, 1, 1])
        self.b = [_dev(b) for b in bn]

    def launch(self, scores=True, labels=False, cat_of_label=None, shape_cat=None, N=None, lds=None):
        """-> (scores [P, C_L] fp32 device or None, labels [P] int32 device or None), both from sentinel guards."""
        from prifit_amd._lib import call, cur_stream
        P, CL = self.P, self.CL
        s = s_base = l_f = l_base = None
        if scores:
            s, s_base = GC.guarded_matrix(P, CL, lds or CL, 4096, 4096, poison=GC.SENTINEL)
        if labels:
            l_f, l_base = GC.guarded((P,), 4096, 4096, poison=GC.SENTINEL)
        p = lambda t: None if t is None else t.data_ptr()
        call("prifit_mlp_chain_rows_bf16", self.X.data_ptr(), self.X.stride(0), P, self.K0, 4,
             _arr(ctypes.c_int32, [w.shape[0] for w in self.W]), _arr(ctypes.c_void_p, [w.data_ptr() for w in self.W]),
             _arr(ctypes.c_longlong, [w.stride(0) for w in self.W]), _arr(ctypes.c_void_p, [b.data_ptr() for b in self.b]), p(s),
             0 if s is None else s.stride(0), p(l_f), p(cat_of_label), p(shape_cat), P if N is None else N, None, cur_stream())
        torch.cuda.synchronize()
        if scores:
            GC.assert_guards_intact(s_base, s)
        if labels:
            GC.assert_guards_intact(l_base, l_f)
        return s, (None if l_f is None else l_f.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 1. pack
def _specials():
    bits = np.array([0x00000000, 0x80000000, 0x7fc00000, 0x7f800000, 0xff800000,
                     0x7f7f7fff, 0x7f7f8000, 0xff7f7fff, 0xff7f8000,      # just below / at the threshold that rounds to inf
                     0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,      # exact ties between two bf16 neighbours: to even
                     0x3f807fff, 0x3f808001, 0x00000001, 0x007fffff, 0x00008000], dtype=np.uint32)
    return bits.view(np.float32)


@pytest.mark.parametrize("cols", [152, 196, 8, 128])
def test_pack_equals_torch_bfloat16_bit_for_bit(cols):
    """Two jobs per width, the plain and the accumulator order, 37 rows (the grid-stride loop ends inside a row), the source
    rows 4 floats apart with NaN in the gap.  Un-permuted, the bit patterns are W.to(torch.bfloat16) of the CPU; every
    padding column is 0.  A NaN is compared as a NaN, not by its payload: the CPU conversion itself has no single pattern
    for it (its vector lanes give 0xffff, its scalar remainder 0x7fc0, depending on the element's position and the CPU)."""
    is_nan16 = lambda x: (x.astype(np.int64) & 0x7fff) > 0x7f80
    rng = np.random.default_rng(cols)
    rows = 37
    Wn = (rng.standard_normal((rows, cols)) * np.exp(rng.uniform(-30, 30, (rows, cols)))).astype(np.float32)
    sp = _specials()
    Wn.reshape(-1)[:len(sp)] = sp                            # the head of the matrix
    Wn.reshape(-1)[-len(sp):] = sp[::-1]                     # and its tail (the last row ends on +0)
    want = torch.from_numpy(Wn).to(torch.bfloat16).view(torch.int16).numpy()
    ldk = _up16(cols)
    for order, got in zip((0, 1), _pack([_dev_rows(Wn), _dev_rows(Wn)], [0, 1], cols=[cols, cols])):
        got = got.cpu().numpy()
        assert got.shape == (rows, ldk)
        src = np.array([_src_col(p, order) for p in range(ldk)])
        assert sorted(src) == list(range(ldk))               # a permutation of the k-steps' columns
        inside = src < cols
        g, w, nan = got[:, inside], want[:, src[inside]], np.isnan(Wn)[:, src[inside]]
        assert np.array_equal(g[~nan], w[~nan]), "order %d" % order
        assert nan.sum() == 2 and np.all(is_nan16(g[nan])) and np.all(is_nan16(w[nan]))
        assert np.all(got[:, ~inside] == 0)


# ---------------------------------------------------------------------------------------------- 2. exact arithmetic
def _int_layer(rng, cout, K):
    """Two non-zeros in {-1, +1} per row, at columns c % K and (5c + 3) % K (moved by one where they coincide); bias in {-1, 0, 1}."""
    W = np.zeros((cout, K), dtype=np.int64)
    c = np.arange(cout)
    k1, k2 = c % K, (5 * c + 3) % K
    k2 = np.where(k2 == k1, (k2 + 1) % K, k2)
    W[c, k1] = rng.choice([-1, 1], cout)
    W[c, k2] = rng.choice([-1, 1], cout)
    return W, rng.integers(-1, 2, cout)


def _nonzero_enough(ref):
    share = float(np.count_nonzero(ref)) / ref.size
    assert share >= 0.5, "the integer reference is %.0f %% zeros: it would pass a kernel that computes nothing" % (100 * (1 - share))


@pytest.mark.parametrize("C0,C1,C2,K,G", POOL_CASES)
def test_pool_chain_is_exact_on_integers(C0, C1, C2, K, G):
    """Inputs in [-3, 3]: |layer 1| <= 7, |layer 2| <= 15 -- integers that bf16 and every fp32 partial sum hold exactly, so a
    wrong column map, a dropped k-step or a padding mistake changes an output and nothing else does."""
    rng = np.random.default_rng(0)
    X = rng.integers(-3, 4, (G * K, C0))
    (W1, b1), (W2, b2) = _int_layer(rng, C1, C0), _int_layer(rng, C2, C1)
    h = np.maximum(np.maximum(X, 0) @ W1.T + b1, 0)
    ref = np.maximum(h @ W2.T + b2, 0).reshape(G, K, C2).max(axis=1)
    assert np.abs(h).max() <= 7 and np.abs(ref).max() <= 15
    _nonzero_enough(ref)
    got = _pool_launch(X, W1, b1, W2, b2, K, ld_gap=8 if G == 5 else 0)
    assert np.array_equal(got.astype(np.float64), ref.astype(np.float64))
    assert np.array_equal(got.view(np.int32), ref.astype(np.float32).view(np.int32))


@pytest.mark.parametrize("K0,CL", ROWS_CASES)
@pytest.mark.parametrize("P", ROWS_P)
def test_rows_chain_is_exact_on_integers(P, K0, CL):
    """|layer l| <= 2^(l + 2) - 1 <= 63.  P = 200: 7 waves, the last with 8 live rows; P = 1: one live row.  The rows are 4
    floats apart with NaN between them: K0 = 152 and 8 end inside a k-step, whose upper half must not be loaded."""
    rng = np.random.default_rng(0)
    a = X = rng.integers(-3, 4, (P, K0))
    Ws, bs, kin = [], [], K0
    for l, cout in enumerate((128, 128, 128, CL)):
        W, b = _int_layer(rng, cout, kin)
        Ws.append(W)
        bs.append(b)
        a = a @ W.T + b
        assert np.abs(a).max() <= 2 ** (l + 3) - 1
        if l < 3:
            a = np.maximum(a, 0)
        kin = cout
    _nonzero_enough(a)
    scores, labels = _RowsNet(X, Ws, bs).launch(scores=True, labels=True, lds=CL + 3)
    got = scores.cpu().numpy()
    assert np.array_equal(got.view(np.int32), a.astype(np.float32).view(np.int32))
    assert np.array_equal(labels.cpu().numpy(), np.argmax(a, axis=1))        # the first maximum


# ---------------------------------------------------------------------------------------------- 3. real values, derived bound
def _bf16(a):
    """fp64 array -> the bf16 neighbour of its fp32 value, as fp64 (the CPU's tensor.to(torch.bfloat16))."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def _layer_bound(a, E, W, b):
    """One chained layer: `a` the exact input (fp64) and E >= |computed input - a| before its rounding -> the bound on
    |computed pre-activation - (W a + b)|.  Rounding the input: E' = E + 2^-9 (|a| + E).  Rounding the weight: 2^-9 |w|.
    So the product is off by at most |W| (1 + 2^-9) E' + 2^-9 |W| |a|, and the fp32 accumulation of K products and the bias
    by (K + 2) 2^-24 (sum |a^| |w^| + |b|)."""
    K = W.shape[1]
    aw = np.abs(W)
    Er = E * (1.0 + R16) + R16 * np.abs(a)
    mag = ((np.abs(a) + Er) @ aw.T) * (1.0 + R16) + np.abs(b)
    return (Er @ aw.T) * (1.0 + R16) + R16 * (np.abs(a) @ aw.T) + (K + 2) * U32 * mag


def _chain64(a, Ws, bs, emulate=False):
    """The layers in fp64 (ReLU between them, none after the last) -> (pre-activation of the last layer, its bound)."""
    E = np.zeros_like(a)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        W, b = W.astype(np.float64), b.astype(np.float64)
        if emulate:
            z = _bf16(a) @ _bf16(W).T + b
        else:
            z, E = a @ W.T + b, _layer_bound(a, E, W, b)
        if l == len(Ws) - 1:
            return z, E
        a = np.maximum(z, 0.0)                                               # 1-Lipschitz: E carries over


def _real_net(rng, P, widths):
    X = rng.standard_normal((P, widths[0])).astype(np.float32)
    Ws = [(rng.standard_normal((co, ci)) / np.sqrt(ci)).astype(np.float32) for ci, co in zip(widths[:-1], widths[1:])]
    bs = [(0.1 * rng.standard_normal(co)).astype(np.float32) for co in widths[1:]]
    return X, Ws, bs


def _report(what, got, ref, bound, emu):
    err = np.abs(got - ref)
    print("%s: max |kernel - fp64| / bound = %.3f, max |kernel - CPU bf16 emulation| = %.3g (max |fp64| %.3g)"
          % (what, float(np.max(err / bound)), float(np.max(np.abs(got - emu))), float(np.max(np.abs(ref)))))
    assert np.all(np.isfinite(got))
    assert np.all(err <= bound)


@pytest.mark.parametrize("C0,C1,C2,K,G", POOL_CASES)
def test_pool_chain_within_the_forward_bound(C0, C1, C2, K, G):
    """Seeded normal data against fp64 of the un-rounded network.  The max over a group's rows is 1-Lipschitz in the
    largest norm, so the pooled output's bound is the largest bound among the group's rows; the last bias + ReLU on the
    maximum is inside the (K + 2) term."""
    rng = np.random.default_rng(300 + C1 + G)
    X, Ws, bs = _real_net(rng, G * K, (C0, C1, C2))
    a0 = np.maximum(X.astype(np.float64), 0.0)
    z, E = _chain64(a0, Ws, bs)
    ref = np.maximum(z, 0.0).reshape(G, K, C2).max(axis=1)
    bound = E.reshape(G, K, C2).max(axis=1)
    emu = np.maximum(_chain64(a0, Ws, bs, emulate=True)[0], 0.0).reshape(G, K, C2).max(axis=1)
    got = _pool_launch(X, Ws[0], bs[0], Ws[1], bs[1], K).astype(np.float64)
    assert np.all(got >= 0.0)
    _report("pool chain (%d, %d, %d) K=%d G=%d" % (C0, C1, C2, K, G), got, ref, bound, emu)


@pytest.mark.parametrize("K0,CL", ROWS_CASES)
@pytest.mark.parametrize("P", ROWS_P)
def test_rows_chain_within_the_forward_bound(P, K0, CL):
    rng = np.random.default_rng(400 + 7 * K0 + CL + P)
    X, Ws, bs = _real_net(rng, P, (K0, 128, 128, 128, CL))
    ref, bound = _chain64(X.astype(np.float64), Ws, bs)
    emu = _chain64(X.astype(np.float64), Ws, bs, emulate=True)[0]
    got = _RowsNet(X, Ws, bs).launch()[0].cpu().numpy().astype(np.float64)
    _report("rows chain K0=%d C_L=%d P=%d" % (K0, CL, P), got, ref, bound, emu)


# ---------------------------------------------------------------------------------------------- 4. NaN and masking
@pytest.mark.parametrize("K0", [152, 8])
def test_a_nan_row_stays_in_its_row(K0):
    """Rows 37 and 199 (the last live row of the last wave) are NaN: their scores are all NaN and they get the first allowed
    channel; every other row's scores and label are, bit for bit, those of the run without the NaN rows -- and finite,
    with NaN directly behind every row's K0 columns."""
    P, CL, N = 200, 50, 40
    rng = np.random.default_rng(500 + K0)
    X, Ws, bs = _real_net(rng, P, (K0, 128, 128, 128, CL))
    col = torch.tensor([c % 5 for c in range(CL)], dtype=torch.int32).cuda()
    cats = torch.tensor([0, 4, 2, 1, 3], dtype=torch.int32).cuda()
    clean = _RowsNet(X, Ws, bs).launch(labels=True, cat_of_label=col, shape_cat=cats, N=N)
    assert bool(torch.isfinite(clean[0]).all())
    Xp = X.copy()
    Xp[37] = np.nan
    Xp[199, 3] = np.nan                                                     # one element is enough
    s, lab = _RowsNet(Xp, Ws, bs).launch(labels=True, cat_of_label=col, shape_cat=cats, N=N)
    bad = np.zeros(P, dtype=bool)
    bad[[37, 199]] = True
    assert bool(torch.isnan(s[torch.from_numpy(bad).cuda()]).all())
    keep = torch.from_numpy(~bad).cuda()
    assert torch.equal(s[keep].view(torch.int32), clean[0][keep].view(torch.int32)) and torch.equal(lab[keep], clean[1][keep])
    assert int(lab[37]) == 0 and int(lab[199]) == 3                         # the first channel of categories 0 and 3
    free = _RowsNet(Xp, Ws, bs).launch(scores=False, labels=True)[1]
    assert int(free[37]) == 0 and int(free[199]) == 0


# ---------------------------------------------------------------------------------------------- 5. labels
def _metrics_pred(scores, B, N, first_label, cat_of_label, restricted):
    """prifit_seg_metrics' pred on the same scores; the shape's category is that of target[b, 0] = first_label[b]."""
    from prifit_amd import ops
    target = torch.zeros(B, N, dtype=torch.int64, device="cuda")
    target[:, 0] = torch.as_tensor(first_label, device="cuda")
    return ops.seg_metrics(scores.contiguous().reshape(B, N, -1), target, cat_of_label, restricted=restricted)[0].reshape(-1)


def test_labels_equal_seg_metrics_on_the_kernels_own_scores():
    """Three interleaved categories, parts without one, a shape whose first label has none (-1 for its rows), two NaN rows;
    then labels alone, then no window."""
    B, N, K0, CL = 4, 50, 152, 50
    X, Ws, bs = _real_net(np.random.default_rng(77), B * N, (K0, 128, 128, 128, CL))
    X[7] = np.nan
    X[2 * N + 49] = np.nan
    col = np.array([(c * 7 + c // 5) % 3 for c in range(CL)], dtype=np.int32)
    col[[0, 13, 49]] = -1
    first = [int(np.flatnonzero(col == 0)[2]), int(np.flatnonzero(col == 1)[0]), int(np.flatnonzero(col == 2)[5]), 13]
    cat_of_label = torch.from_numpy(col).cuda()
    shape_cat = cat_of_label[torch.tensor(first, device="cuda")].contiguous()
    assert shape_cat.tolist() == [0, 1, 2, -1]
    net = _RowsNet(X, Ws, bs)
    scores, labels = net.launch(labels=True, cat_of_label=cat_of_label, shape_cat=shape_cat, N=N)
    assert bool(torch.isnan(scores[7]).all()) and bool(torch.isnan(scores[2 * N + 49]).all())
    assert torch.equal(labels.long(), _metrics_pred(scores, B, N, first, cat_of_label, True))
    lab = labels.cpu().numpy().reshape(B, N)
    assert np.all(lab[3] == -1)
    for b in range(3):
        assert np.all(col[lab[b]] == b) and len(np.unique(lab[b])) > 1
    assert lab[0, 7] == np.flatnonzero(col == 0)[0] and lab[2, 49] == np.flatnonzero(col == 2)[0]
    alone = net.launch(scores=False, labels=True, cat_of_label=cat_of_label, shape_cat=shape_cat, N=N)[1]
    assert torch.equal(alone, labels)
    free = net.launch(scores=False, labels=True)[1]
    assert torch.equal(free.long(), _metrics_pred(scores, B, N, first, cat_of_label, False))
    assert int(free[7]) == 0 and int(free[2 * N + 49]) == 0 and len(torch.unique(free)) > 3


def test_labels_ties_infinity_and_a_category_without_parts():
    """Channels 3 / 4 (the two lane halves), 8 / 9 (neighbours in a lane) and 21 / 38 (one lane, two blocks) share a row of
    W_4 and a bias that makes them the maximum of their category: exact ties, the lower index wins.  Category 3 has +inf
    in channel 45; category 9 has no part."""
    B, N, K0, CL = 6, 35, 160, 50                          # 210 rows: the last wave has 18 live rows
    X, Ws, bs = _real_net(np.random.default_rng(78), B * N, (K0, 128, 128, 128, CL))
    col = np.array([c % 3 for c in range(CL)], dtype=np.int32)
    col[[3, 4, 20]] = 4
    col[[8, 9, 30]] = 5
    col[[21, 33, 38]] = 6
    col[[40, 45, 47]] = 3
    for lo, hi in ((3, 4), (8, 9), (21, 38)):
        Ws[3][hi] = Ws[3][lo]
        bs[3][lo] = bs[3][hi] = 100.0
    bs[3][45] = np.inf
    cat_of_label = torch.from_numpy(col).cuda()
    shape_cat = torch.tensor([4, 5, 6, 3, 9, 1], dtype=torch.int32, device="cuda")
    scores, labels = _RowsNet(X, Ws, bs).launch(labels=True, cat_of_label=cat_of_label, shape_cat=shape_cat, N=N)
    s = scores.cpu().numpy()
    for lo, hi in ((3, 4), (8, 9), (21, 38)):
        assert np.array_equal(s[:, lo].view(np.int32), s[:, hi].view(np.int32))
    assert np.all(np.isposinf(s[:, 45]))
    lab = labels.cpu().numpy().reshape(B, N)
    assert np.all(lab[0] == 3) and np.all(lab[1] == 8) and np.all(lab[2] == 21) and np.all(lab[3] == 45) and np.all(lab[4] == -1)
    assert np.all(col[lab[5]] == 1)
    pred = _metrics_pred(scores, B, N, [3, 8, 21, 40, 0, 1], cat_of_label, True).reshape(B, N)
    keep = [0, 1, 2, 3, 5]
    assert torch.equal(labels.reshape(B, N).long()[keep], pred[keep])


# ---------------------------------------------------------------------------------------------- 6. end to end
def _seeded_model(normal, seed):
    """get_model(50) with seeded weights, BatchNorm gamma / beta and running statistics away from (1, 0, 0, 1)."""
    from prifit_amd.models import pointnet2_part_seg_msg as M
    torch.manual_seed(seed)
    net = M.get_model(50, normal_channel=normal)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
    return net.cuda().eval()


def _inputs(B, C, N, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(B, C, N, generator=g) * 2 - 1).cuda()
    onehot = torch.eye(16)[torch.randint(0, 16, (B,), generator=g)].reshape(B, 1, 16).cuda()
    start = (torch.randint(0, N, (B,), generator=g).cuda(), torch.randint(0, 512, (B,), generator=g).cuda())
    return xyz, onehot, start


def _gather(table, idx):
    B = table.shape[0]
    flat = idx.reshape(B, -1).long()
    return torch.gather(table, 1, flat.unsqueeze(-1).expand(-1, -1, table.shape[-1])).reshape(*idx.shape, table.shape[-1])


def _cpu_net(frozen, xyz, onehot, fps_start, sa_bf16, tail_bf16):
    """fp64 CPU run of the folded network (index lists, 3-NN and its weights from the GPU entry points) -> (log-probabilities
    [B, N, parts], scores).  sa_bf16: layers 2 and 3 of every SA1 / SA2 scale take their input and weight rounded to bf16 --
    the operands of prifit_mlp_chain_pool_bf16; tail_bf16: the same for all four layers of the per-point tail
    (prifit_mlp_chain_rows_bf16).  Sums and biases stay fp64."""
    from prifit_amd import ops
    cpu = lambda t: t.detach().double().cpu()
    rnd = lambda t: t.float().to(torch.bfloat16).double()
    B, _, N = xyz.shape
    pts_g = xyz.permute(0, 2, 1).contiguous()
    xyz_g = pts_g[:, :, :3].contiguous()
    pts, l0_xyz = cpu(pts_g), cpu(xyz_g)

    def mlp(x, layers, bf16_from=None, last_relu=True):
        for i, ly in enumerate(layers):
            W, b = cpu(ly.W[:, :ly.kin]), cpu(ly.b)
            if bf16_from is not None and i >= bf16_from:
                x, W = rnd(x), rnd(W)
            x = x @ W.t() + b
            if last_relu or i + 1 < len(layers):
                x = torch.relu(x)
        return x

    def sa(lv, xyz_gpu, xyz_c, feats, start):
        _, nx_gpu = ops.farthest_point_sample(xyz_gpu, lv["npoint"], start, return_xyz=True)
        lists = ops.ball_query_multi(lv["radii"], lv["nsamples"], xyz_gpu, nx_gpu)
        centres = cpu(nx_gpu)
        outs = []
        for (st, _), gi, K in zip(lv["scales"], lists, lv["nsamples"]):
            gi = gi.cpu()
            g = torch.cat([_gather(feats, gi), _gather(xyz_c, gi) - centres.unsqueeze(2)], dim=-1)
            y = mlp(g.reshape(B * lv["npoint"] * K, -1), st, 1 if sa_bf16 else None)
            outs.append(y.reshape(B, lv["npoint"], K, -1).amax(dim=2))
        return nx_gpu, centres, torch.cat(outs, dim=-1)

    def fp_rows(x1_gpu, x2_gpu, p1, p2):
        if p2.shape[1] == 1:
            interp = p2.expand(B, p1.shape[1], -1)
        else:
            idx, w = ops.three_nn(x1_gpu, x2_gpu)
            interp = (_gather(p2, idx.cpu()) * cpu(w).unsqueeze(-1)).sum(dim=2)
        x = torch.cat([p1, interp], dim=-1)                                     # upstream's order
        return x.reshape(-1, x.shape[-1])

    l1_gpu, l1_xyz, l1_points = sa(frozen._sa[0], xyz_g, l0_xyz, pts, fps_start[0])
    l2_gpu, l2_xyz, l2_points = sa(frozen._sa[1], l1_gpu, l1_xyz, l1_points, fps_start[1])
    g = torch.cat([l2_xyz, l2_points], dim=-1)
    l3_points = mlp(g.reshape(-1, g.shape[-1]), frozen._sa3[0]).reshape(B, l2_xyz.shape[1], -1).amax(dim=1, keepdim=True)
    l2_up = mlp(fp_rows(None, None, l2_points, l3_points), frozen._fp["fp3"][0]).reshape(B, l2_points.shape[1], -1)
    l1_up = mlp(fp_rows(l1_gpu, l2_gpu, l1_points, l2_up), frozen._fp["fp2"][0]).reshape(B, l1_points.shape[1], -1)
    skip = torch.cat([cpu(onehot).reshape(B, 1, 16).expand(B, N, 16), l0_xyz, pts], dim=-1)
    tail = list(frozen._fp["fp1"][0]) + list(frozen._head) + [frozen._conv2]
    scores = mlp(fp_rows(xyz_g, l1_gpu, skip, l1_up), tail, 0 if tail_bf16 else None, last_relu=False)
    return torch.log_softmax(scores, dim=1).reshape(B, N, -1)


@pytest.fixture(scope="module", params=[(False, 2), (True, 1)], ids=["xyz_B2", "normals_B1"])
def e2e(request):
    from prifit_amd import inference, testing as T
    normal, B = request.param
    net = _seeded_model(normal, 6 if normal else 5)
    f32, b16 = inference.freeze(net), inference.freeze(net, precision="bf16")
    xyz, onehot, start = _inputs(B, 6 if normal else 3, 1024, 11)
    col = T.SegmentationEvaluator().cat_of_label
    shape_cat = onehot.reshape(B, 16).argmax(dim=1)
    torch.cuda.synchronize()
    return dict(net=net, f32=f32, b16=b16, xyz=xyz, onehot=onehot, start=start, col=col, shape_cat=shape_cat, B=B, C=6 if normal else 3)


def _spy(monkeypatch_ctx, seen):
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


def test_module_surface(e2e):
    f32, b16 = e2e["f32"], e2e["b16"]
    assert f32.precision == "fp32" and b16.precision == "bf16"
    assert not list(f32.buffers()) and "flat_bf16" not in f32.state_dict() and list(f32.state_dict()) == ["flat"]
    for a, b in zip(f32._layers, b16._layers):                                 # the fold does not know the precision
        assert torch.equal(a.W, b.W) and torch.equal(a.b, b.b)
    (name, buf), = b16.named_buffers()
    assert name == "flat_bf16" and buf.dtype == torch.int16 and buf.is_cuda and sorted(b16.state_dict()) == ["flat", "flat_bf16"]
    assert len(b16._bf16) == 14
    # every bf16 weight is its fp32 source rounded: un-permuted, bit for bit tensor.to(torch.bfloat16)
    for w in b16._bf16:
        src = w.src.W[:, :w.cols].cpu()
        cols = torch.tensor([_src_col(p, w.order) for p in range(w.ldk)])
        inside = cols < w.cols
        got = w.W.cpu()
        assert torch.equal(got[:, inside], src.to(torch.bfloat16).view(torch.int16)[:, cols[inside]])
        assert bool((got[:, ~inside] == 0).all())
    # .float() leaves the 16-bit patterns alone
    before = buf.clone()
    assert b16.float() is b16 and b16.flat_bf16.dtype == torch.int16 and torch.equal(b16.flat_bf16, before)


def test_routes(e2e, monkeypatch):
    """bf16: five pooled bf16 chains and no fp32 one; labels() ends in one bf16 row chain right behind fp1's prifit_fp_rows;
    forward() keeps its separate-launch tail; refresh() packs once.  fp32: no bf16 entry point at all."""
    f32, b16 = e2e["f32"], e2e["b16"]
    args = (e2e["xyz"], e2e["onehot"])
    seen = []
    with monkeypatch.context() as mp:
        _spy(mp, seen)
        b16(*args, fps_start=e2e["start"])
        fwd = list(seen)
        seen.clear()
        b16.labels(*args, e2e["shape_cat"], e2e["col"], fps_start=e2e["start"])
        lab = list(seen)
        seen.clear()
        b16.refresh()
        ref = list(seen)
        seen.clear()
        f32(*args, fps_start=e2e["start"])
        f32.labels(*args, e2e["shape_cat"], e2e["col"], fps_start=e2e["start"])
        f32.refresh()
        plain = list(seen)
    for names in (fwd, lab):
        assert names.count("prifit_mlp_chain_pool_bf16") == 5 and "prifit_mlp_chain_pool_f32" not in names
        assert names.count("prifit_sa_group_linear_fwd") == 2 and names.count("prifit_fps") == 2
    assert not any("rows" in n and "chain" in n for n in fwd)
    assert fwd[len(fwd) - 1 - fwd[::-1].index("prifit_fp_rows"):].count("prifit_gemm_f32") >= 4      # fp1 x 2, conv1, conv2
    assert lab.count("prifit_mlp_chain_rows_bf16") == 1 and "prifit_mlp_chain_rows_f32" not in lab
    assert lab[len(lab) - 1 - lab[::-1].index("prifit_fp_rows"):] == ["prifit_fp_rows", "prifit_mlp_chain_rows_bf16"]
    assert ref == ["prifit_fold_bn", "prifit_pack_cols_multi", "prifit_pack_bf16_multi"]
    assert not any("bf16" in n for n in plain)
    assert plain.count("prifit_mlp_chain_pool_f32") == 10 and plain.count("prifit_mlp_chain_rows_f32") == 1
    # the launches of the two precisions differ in those names only
    swap = {"prifit_mlp_chain_pool_bf16": "prifit_mlp_chain_pool_f32", "prifit_mlp_chain_rows_bf16": "prifit_mlp_chain_rows_f32"}
    assert [swap.get(n, n) for n in fwd + lab] == plain[:len(fwd) + len(lab)]


def test_index_lists_equal_the_fp32_modules(e2e, monkeypatch):
    """Sampling and 3-NN see positions only: the centre lists, the centres and the 3-NN indices and weights of the bf16
    module are the fp32 module's, bit for bit, on every level."""
    import prifit_amd.ops as O
    rec = []
    fps, nn3 = O.farthest_point_sample, O.three_nn

    def fps_rec(*a, **k):
        out = fps(*a, **k)
        rec.extend(out)
        return out

    def nn3_rec(*a, **k):
        out = nn3(*a, **k)
        rec.extend(out)
        return out

    monkeypatch.setattr(O, "farthest_point_sample", fps_rec)
    monkeypatch.setattr(O, "three_nn", nn3_rec)
    e2e["f32"].labels(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"])
    a = list(rec)
    rec.clear()
    e2e["b16"].labels(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"])
    assert len(a) == len(rec) == 2 * 2 + 2 * 2                                  # 2 x (idx, centres), 2 x (idx, weights)
    for x, y in zip(a, rec):
        assert x.dtype == y.dtype and torch.equal(x, y)


def test_accuracy_against_fp64_with_the_cpu_emulation_as_the_bar(e2e):
    """seg of predict() (bf16 pooled chains, fp32 tail) and scores - logsumexp of labels() (bf16 tail too), each against the
    fp64 run of the folded network; the bar is twice the error of the CPU run with bf16 roundings at exactly the chained
    layers' operands and fp64 sums (the factor 2: fp32 accumulation order and the rounding flips it causes)."""
    b16, args = e2e["b16"], (e2e["xyz"], e2e["onehot"], e2e["start"])
    ref = _cpu_net(b16, *args, False, False)
    seg = b16.predict(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"]).double().cpu()
    scores = b16.labels(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"], return_scores=True)[1]
    logp = torch.log_softmax(scores.double().cpu(), dim=-1)
    for name, got, emu in (("seg (predict)", seg, _cpu_net(b16, *args, True, False)), ("scores - logsumexp (labels)", logp, _cpu_net(b16, *args, True, True))):
        bar = 2.0 * float((emu - ref).abs().max())
        err = float((got - ref).abs().max())
        print("bf16 %s: |GPU - fp64| %.4g, bar %.4g (2 x the CPU bf16 emulation's %.4g); |GPU - emulation| %.4g"
              % (name, err, bar, bar / 2, float((got - emu).abs().max())))
        assert bool(torch.isfinite(got).all())
        assert err <= bar, name
    # the fp32 module on the same inputs, for scale
    seg32 = e2e["f32"].predict(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"]).double().cpu()
    print("fp32 seg: |GPU - fp64| %.4g; labels agree on %.2f %% of the points"
          % (float((seg32 - ref).abs().max()), 100.0 * float((seg32.argmax(-1) == seg.argmax(-1)).double().mean())))


def test_refresh_rewrites_the_bf16_buffer(e2e):
    """The snapshot does not move with the live model; after a training-mode forward (the running statistics move) and a
    changed chained weight, refresh() gives what a fresh freeze gives; the old state brings the old outputs back."""
    from prifit_amd import inference
    net, b16 = e2e["net"], e2e["b16"]
    args = (e2e["xyz"], e2e["onehot"], e2e["shape_cat"], e2e["col"])
    run = lambda m: m.labels(*args, fps_start=e2e["start"], return_scores=True)
    before, bits = run(b16), b16.flat_bf16.clone()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    try:
        net.train()
        with torch.no_grad():
            net(torch.rand(2, e2e["C"], 1024, device="cuda") * 2 - 1, torch.eye(16, device="cuda")[:2].reshape(2, 1, 16))
            net.sa1.conv_blocks[1][2].weight.mul_(1.25)
            net.conv2.bias[3] += 0.5
        net.eval()
        same = run(b16)
        assert torch.equal(same[1], before[1]) and torch.equal(b16.flat_bf16, bits)
        b16.refresh()
        moved = run(b16)
        assert not torch.equal(b16.flat_bf16, bits) and not torch.equal(moved[1], before[1])
        fresh = inference.freeze(net, precision="bf16")
        assert torch.equal(fresh.flat_bf16, b16.flat_bf16)
        again = run(fresh)
        assert torch.equal(again[0], moved[0]) and torch.equal(again[1], moved[1])
    finally:
        net.load_state_dict(state)
        net.eval()
        b16.refresh()
    back = run(b16)
    assert torch.equal(b16.flat_bf16, bits) and torch.equal(back[0], before[0]) and torch.equal(back[1], before[1])

"""GPU: the per-point embedding from the frozen network (FrozenPartSeg.embed, prifit_mlp_chain_embed_f32 / _bf16, csrc/
infer_chain.h mlp_chain_embed_kernel) -- the embedding against an fp64 restatement with the separate-launch route as the
yardstick of its error, both pipes on integer data with no tolerance (the normalisation included), bf16 inside its forward
bound, head A against prifit_mlp_chain_rows_* bit for bit, NaN rows, the argument checks, and the method end to end.  Every
operand sits in guard bands (guard_common); every output starts as a NaN sentinel, so an unwritten element shows."""
import ctypes

import numpy as np
import pytest
import torch

import embed_common as EC
import guard_common as GC

pytestmark = pytest.mark.gpu

PIPES = ["f32", "bf16"]
MAIN = (0, 1, 2, 4)          # layers 1 .. 3 and W_e among the five weights of a net


def _lde(P, K0, CL):
    """One case runs on a pitch of 132: columns 128 .. 131 are guards."""
    return 132 if (P, K0, CL) == (200, 152, 50) else 128


# ---------------------------------------------------------------------------------------------- 1. fp32 against fp64
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("K0,CL", EC.CASES)
@pytest.mark.parametrize("P", EC.ROWS)
def test_embedding_against_fp64_and_the_separate_launches(P, K0, CL, normalize):
    """The chain's largest error against fp64 in units of u (sum_k |a_k| |w_k| + |b|) of the last product -- divided by the
    fp64 norm with normalize = 1 -- is at most twice that of the separate-launch route on the same inputs (W_e as the last
    product, then F.normalize on the device): another summation order over the same fp32 arithmetic."""
    Xn, Wn, bn = EC.seeded_net(P, K0, CL, 2000 + 7 * K0 + CL + P)
    ref, scale = EC.embed64(Xn, Wn, bn, normalize)
    net = EC.EmbedNet("f32", Xn, Wn, bn)
    emb, scores, _ = net.launch(normalize, lde=_lde(P, K0, CL), scores=True)
    assert (scores is None) == (CL == 0)
    got = emb.cpu().numpy().astype(np.float64)
    sep = EC.separate_route(net.X.contiguous(), [net.W[i] for i in MAIN], [net.b[i] for i in MAIN], normalize).cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got))
    e_chain = float(np.max(np.abs(got - ref) / scale))
    e_sep = float(np.max(np.abs(sep - ref) / scale))
    print("embed chain K0=%d C_L=%d P=%d normalize=%d: chain %.3g u, separate launches %.3g u"
          % (K0, CL, P, normalize, e_chain / EC.U, e_sep / EC.U))
    assert e_chain <= 2.0 * e_sep


# ---------------------------------------------------------------------------------------------- 2. exact on integers
@pytest.mark.parametrize("pipe", PIPES)
@pytest.mark.parametrize("K0,CL", EC.CASES)
@pytest.mark.parametrize("P", EC.ROWS)
def test_embed_chain_is_exact_on_integers(P, K0, CL, pipe):
    """|a_3| <= 31, |e| <= 63: integers that bf16 and every fp32 partial sum hold exactly.  normalize = 0: the integer
    reference bit for bit.  normalize = 1: the sum of squares is an integer below 2^24 -- exact in any order -- and the square
    root and the division are single correctly rounded operations, so numpy's float32 e / max(sqrt(s), 1e-12) bit for bit."""
    X, Ws, bs, a3, z, e = EC.int_net(P, K0, CL)
    EC.nonzero_enough(e)
    net = EC.EmbedNet(pipe, X, Ws, bs)
    emb, scores, labels = net.launch(0, lde=_lde(P, K0, CL), scores=True, labels=True)
    e32 = e.astype(np.float32)
    assert np.array_equal(emb.cpu().numpy().view(np.int32), e32.view(np.int32))
    if CL:
        assert np.array_equal(scores.cpu().numpy().view(np.int32), z.astype(np.float32).view(np.int32))
        assert np.array_equal(labels.cpu().numpy(), np.argmax(z, axis=1))
    s = np.sum(e * e, axis=1, keepdims=True)
    assert int(s.max()) < 2 ** 24
    want = e32 / np.maximum(np.sqrt(s.astype(np.float32)), np.float32(1e-12))
    assert want.dtype == np.float32
    EC.nonzero_enough(want)
    got = net.launch(1, lde=_lde(P, K0, CL))[0].cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ---------------------------------------------------------------------------------------------- 3. bf16, real values
@pytest.mark.parametrize("K0,CL", EC.CASES)
@pytest.mark.parametrize("P", EC.ROWS)
def test_bf16_embedding_within_the_forward_bound(P, K0, CL):
    """Seeded normal data against fp64 of the un-rounded network: |kernel - fp64| <= the bound layer_bound carries through
    the four layers.  With normalize = 1 the result is the fp32 normalisation of the kernel's own e (see normalize_f32_bound)."""
    Xn, Wn, bn = EC.seeded_net(P, K0, CL, 3000 + 7 * K0 + CL + P)
    ref, bound = EC.chain64(Xn, [Wn[i] for i in MAIN], [bn[i] for i in MAIN])
    net = EC.EmbedNet("bf16", Xn, Wn, bn)
    got = net.launch(0, lde=_lde(P, K0, CL))[0].cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    print("bf16 embed chain K0=%d C_L=%d P=%d: max |kernel - fp64| / bound = %.3f (max |fp64| %.3g)"
          % (K0, CL, P, float(np.max(err / bound)), float(np.max(np.abs(ref)))))
    assert np.all(np.isfinite(got)) and np.all(err <= bound)
    gotn = net.launch(1, lde=_lde(P, K0, CL))[0].cpu().numpy().astype(np.float64)
    want, nb = EC.normalize_f32_bound(got)
    assert np.all(np.isfinite(gotn)) and np.all(np.abs(gotn - want) <= nb)


# ---------------------------------------------------------------------------------------------- 4. head A = the rows kernel
@pytest.mark.parametrize("pipe", PIPES)
def test_head_a_is_the_rows_kernel(pipe):
    """The operands of test_labels_equal_seg_metrics_on_the_same_scores: cat_of_label interleaves three categories and leaves
    parts without one, the fourth shape has category -1, two input rows are NaN.  scores and labels equal
    prifit_mlp_chain_rows_*'s bit for bit -- with a window, labels alone, and without a window -- and the embedding does
    not depend on head A being there."""
    B, N, K0, CL = 4, 50, 152, 50
    Xn, Wn, bn = EC.seeded_net(B * N, K0, CL, 77)
    Xn[7] = np.nan
    Xn[2 * N + 49] = np.nan
    col = np.array([(c * 7 + c // 5) % 3 for c in range(CL)], dtype=np.int32)
    col[[0, 13, 49]] = -1
    first = [int(np.flatnonzero(col == 0)[2]), int(np.flatnonzero(col == 1)[0]), int(np.flatnonzero(col == 2)[5]), 13]
    cat_of_label = torch.from_numpy(col).cuda()
    shape_cat = cat_of_label[torch.tensor(first, device="cuda")].contiguous()
    assert shape_cat.tolist() == [0, 1, 2, -1]
    net = EC.EmbedNet(pipe, Xn, Wn, bn)
    eq = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    plain = {n: net.launch(n, head=False)[0] for n in (0, 1)}
    for n in (0, 1):
        assert bool(torch.isnan(plain[n][7]).all()) and bool(torch.isnan(plain[n][2 * N + 49]).all())
    win = dict(cat_of_label=cat_of_label, shape_cat=shape_cat, N=N)
    want_s, want_l = net.rows_launch(**win)
    assert bool(torch.isnan(want_s[7]).all()) and bool((want_l.reshape(B, N)[3] == -1).all())
    for n in (0, 1):
        emb, s, l = net.launch(n, scores=True, labels=True, **win)
        assert eq(s, want_s) and torch.equal(l, want_l) and eq(emb, plain[n])
    emb, s, l = net.launch(1, labels=True, **win)                    # labels alone
    assert s is None and torch.equal(l, want_l) and eq(emb, plain[1])
    free_s, free_l = net.rows_launch(lds=CL + 2)                        # no window, padded scores
    emb, s, l = net.launch(0, scores=True, labels=True, lds=CL + 2)
    assert eq(s, free_s) and torch.equal(l, free_l) and eq(emb, plain[0]) and len(torch.unique(free_l)) > 3
    emb, s, l = net.launch(0, scores=True)                           # scores alone
    assert l is None and eq(s, free_s) and eq(emb, plain[0])


# ---------------------------------------------------------------------------------------------- 5. NaN rows
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("pipe", PIPES)
def test_a_nan_row_stays_in_its_row(pipe, normalize):
    """Rows 37 and 199 (the last live row of the last wave; one NaN element is enough) are NaN: those rows of emb are all NaN,
    every other row is, bit for bit, that of the run without them -- and finite, with NaN directly behind every row's K0
    columns."""
    P, K0, CL = 200, 152, 50
    Xn, Wn, bn = EC.seeded_net(P, K0, CL, 500 + normalize)
    clean = EC.EmbedNet(pipe, Xn, Wn, bn).launch(normalize, lde=132, labels=True)[0]
    assert bool(torch.isfinite(clean).all())
    Xp = Xn.copy()
    Xp[37] = np.nan
    Xp[199, 3] = np.nan
    emb = EC.EmbedNet(pipe, Xp, Wn, bn).launch(normalize, lde=132, labels=True)[0]
    bad = torch.zeros(P, dtype=torch.bool, device="cuda")
    bad[[37, 199]] = True
    assert bool(torch.isnan(emb[bad]).all())
    assert torch.equal(emb[~bad].contiguous().view(torch.int32), clean[~bad].contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------- 6. argument checks
@pytest.mark.parametrize("pipe", PIPES)
def test_bad_arguments_return_einval_without_a_launch(pipe):
    """One case per clause of the header's list; no output word changes."""
    P, K0, CL, N = 200, 152, 50, 100
    Xn, Wn, bn = EC.seeded_net(P, K0, CL, 9)
    net = EC.EmbedNet(pipe, Xn, Wn, bn)
    out = net.outputs(lde=132, scores=True, labels=True, lds=52)
    cat = torch.zeros(CL, dtype=torch.int32, device="cuda")
    shp = torch.zeros(P // N, dtype=torch.int32, device="cuda")
    ok = dict(cat_of_label=cat, shape_cat=shp, N=N)
    p = lambda i: net.W[i].data_ptr()
    q = lambda i: net.b[i].data_ptr()
    ptrs = lambda *v: EC.arr(ctypes.c_void_p, list(v))
    ldw = [net.W[i].stride(0) for i in MAIN]
    lls = lambda *v: EC.arr(ctypes.c_longlong, list(v))
    w4 = lambda *v: EC.arr(ctypes.c_int32, list(v))
    emb_ptr = out["emb"][0].data_ptr()
    bad = [
        # what the rows entry rejects of its own arguments
        dict(X=None), dict(X=net.X.data_ptr() + 4), dict(ldx=K0 - 4), dict(ldx=K0 + 2), dict(P=0), dict(P=1 << 31),
        dict(K0=156), dict(K0=168), dict(L=3), dict(widths=None), dict(widths=w4(128, 96, 128, 128)),
        dict(widths=w4(128, 128, 128, 64)), dict(CL=65), dict(CL=-1),
        dict(W=None), dict(W=ptrs(p(0), None, p(2), p(4))), dict(W=ptrs(p(0), p(1), p(2) + 4, p(4))), dict(W=ptrs(p(0), p(1), p(2), None)),
        dict(ldw=None), dict(ldw=lls(K0 - 8, ldw[1], ldw[2], ldw[3])), dict(ldw=lls(ldw[0], ldw[1], ldw[2] + 2, ldw[3])),
        dict(ldw=lls(ldw[0], ldw[1], ldw[2], 120)),
        dict(b=None), dict(b=ptrs(q(0), q(1), q(2), None)), dict(b=ptrs(q(0) + 8, q(1), q(2), q(4))),
        dict(lds=CL - 1), dict(cat=None), dict(shape_cat=None), dict(N=0), dict(N=-4), dict(N=96),
        # the embedding's own
        dict(emb=None), dict(emb=emb_ptr + 4), dict(emb=emb_ptr + 8), dict(lde=124), dict(lde=130),
        # head A asked for but not described, described but not asked for
        dict(CL=0), dict(CL=0, labels=None, cat=None, shape_cat=None), dict(CL=0, scores=None),
        dict(W_cls=None), dict(b_cls=None), dict(W_cls=p(3) + 4), dict(b_cls=q(3) + 4), dict(ldw_cls=120), dict(ldw_cls=net.W[3].stride(0) + 2),
        dict(scores=None, labels=None, cat=None, shape_cat=None),
    ]
    for normalize in (0, 1):
        assert net.raw(dict(out), normalize, **ok) == 0                 # the base call is a good one ...
        torch.cuda.synchronize()
        fresh = net.outputs(lde=132, scores=True, labels=True, lds=52)   # ... and these stay untouched
        for kw in bad:
            assert net.raw(fresh, normalize, **{**ok, **kw}) == -1, kw
        torch.cuda.synchronize()
        for view, base in fresh.values():
            assert bool((base.view(torch.int32) == GC.poison_bits(GC.SENTINEL)).all())


# ---------------------------------------------------------------------------------------------- 7. end to end
@pytest.fixture(scope="module", params=[(False, 2), (True, 1)], ids=["xyz_B2", "normals_B1"])
def e2e(request):
    from prifit_amd import inference, testing as T
    normal, B = request.param
    net = EC.seeded_model(normal, 6 if normal else 5)
    f32, b16 = inference.freeze(net), inference.freeze(net, precision="bf16")
    xyz, onehot, start = EC.inputs(B, 6 if normal else 3, 1024, 11)
    col = T.SegmentationEvaluator().cat_of_label
    shape_cat = onehot.reshape(B, 16).argmax(dim=1)
    torch.cuda.synchronize()
    return dict(net=net, f32=f32, b16=b16, xyz=xyz, onehot=onehot, start=start, col=col, shape_cat=shape_cat, B=B)


def _tail64(frozen, l0_up):
    """fp64 CPU restatement of the tail behind fp1 on given l0_up rows [P, 128]: relu(conv1 + bn1), extra_conv_emb."""
    cpu = lambda t: t.detach().double().cpu().numpy()
    head, emb = frozen._head[0], frozen._emb
    a = np.maximum(cpu(l0_up) @ cpu(head.W[:, :head.kin]).T + cpu(head.b), 0.0)
    return a @ cpu(emb.W[:, :emb.kin]).T + cpu(emb.b)


def test_embed_end_to_end_against_forward(e2e, monkeypatch):
    """embed() against forward(embed=True)[-1] in the row-major layout.  The bar is measured, not fixed: the largest
    difference between forward(embed=True) and the fp64 restatement of the tail on the frozen module's own l0_up rows (what
    forward's two last products do to them); embed(), which forms l0_up itself in another summation order, may differ from
    that restatement by at most twice as much."""
    f32, B = e2e["f32"], e2e["B"]
    args = (e2e["xyz"], e2e["onehot"])
    kept = []
    fp_level = f32._fp_level

    def keep_l0_up(name, *a):
        out = fp_level(name, *a)
        if name == "fp1":
            kept.append(out)
        return out

    with monkeypatch.context() as mp:
        mp.setattr(f32, "_fp_level", keep_l0_up)
        fwd = f32(*args, fps_start=e2e["start"], embed=True)[-1].permute(0, 2, 1)
    assert len(kept) == 1
    ref = torch.from_numpy(_tail64(f32, kept[0].reshape(-1, 128))).reshape(B, 1024, 128)
    emb = f32.embed(*args, fps_start=e2e["start"])
    assert emb.shape == (B, 1024, 128) and emb.dtype == torch.float32 and emb.is_contiguous()
    e_fwd = float((fwd.double().cpu() - ref).abs().max())
    e_emb = float((emb.double().cpu() - ref).abs().max())
    print("embed(): |forward(embed=True) - fp64 tail| %.3g, |embed() - fp64 tail| %.3g, |embed() - forward| %.3g (max |fp64| %.3g)"
          % (e_fwd, e_emb, float((emb - fwd).abs().max()), float(ref.abs().max())))
    assert e_emb <= 2.0 * e_fwd
    # l2_norm=None takes the live model's attribute (False here); True gives unit rows
    assert torch.equal(f32.embed(*args, fps_start=e2e["start"], l2_norm=False), emb)
    unit = f32.embed(*args, fps_start=e2e["start"], l2_norm=True)
    norms = unit.double().norm(dim=-1)
    print("embed(l2_norm=True): max | ||row|| - 1 | = %.3g u" % (float((norms - 1).abs().max()) / EC.U))
    assert float((norms - 1).abs().max()) <= 4 * EC.U
    want = emb.double() / emb.double().norm(dim=-1, keepdim=True).clamp_min(1e-12)
    assert float((unit.double() - want).abs().max()) <= 70 * EC.U32
    e2e["net"].l2_norm = True
    try:
        assert torch.equal(f32.embed(*args, fps_start=e2e["start"]), unit)
    finally:
        e2e["net"].l2_norm = False


@pytest.mark.parametrize("precision", ["f32", "b16"])
def test_embed_labels_are_labels(e2e, precision):
    """return_labels=True: the labels of labels() with the same arguments, from the embedding's launch; the embedding does
    not change with them."""
    m = e2e[precision]
    args = (e2e["xyz"], e2e["onehot"])
    emb = m.embed(*args, fps_start=e2e["start"])
    got, lab = m.embed(*args, fps_start=e2e["start"], shape_cat=e2e["shape_cat"], cat_of_label=e2e["col"], return_labels=True)
    assert lab.shape == (e2e["B"], 1024) and lab.dtype == torch.int32
    assert torch.equal(lab, m.labels(*args, e2e["shape_cat"], e2e["col"], fps_start=e2e["start"])) and torch.equal(got, emb)
    got, lab = m.embed(*args, fps_start=e2e["start"], return_labels=True)
    assert torch.equal(lab, m.labels(*args, fps_start=e2e["start"])) and torch.equal(got, emb)
    with pytest.raises(ValueError):
        m.embed(*args, shape_cat=e2e["shape_cat"], return_labels=True)
    with pytest.raises(ValueError):
        m.embed(*args, shape_cat=e2e["shape_cat"], cat_of_label=e2e["col"][:49], return_labels=True)


def test_bf16_embed_within_the_forward_bound_of_the_fp32_modules(e2e, monkeypatch):
    """On the bf16 module's own fp1 rows R (its trunk runs the pooled chains in bf16, so the fp32 module's rows are other
    rows): |bf16 embed() - fp32 chain on R| <= the forward bound of the four layers on R + |fp32 chain on R - fp64|."""
    f32, b16, B = e2e["f32"], e2e["b16"], e2e["B"]
    kept = []
    fp_rows = b16._fp_rows

    def keep_rows(*a):
        kept.append(fp_rows(*a))
        return kept[-1]

    with monkeypatch.context() as mp:
        mp.setattr(b16, "_fp_rows", keep_rows)
        emb16 = b16.embed(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"])
    R = kept[-1]
    K0, widths, parts = f32._embed_shape()
    assert R.shape == (B * 1024, K0)
    emb32 = torch.empty(B, 1024, 128, device="cuda")
    f32._chain_embed(R, K0, widths, parts, emb32, False, None, None, None, 1024)
    cpu = lambda t: t.detach().double().cpu().numpy()
    layers = [f32._tail_w0] + f32._tail[1:-1] + [f32._emb]
    Ws = [cpu(ly.W)[:, :K0 if i == 0 else 128] for i, ly in enumerate(layers)]
    bs = [cpu(ly.b) for ly in f32._tail[:-1]] + [cpu(f32._emb.b)]
    ref, bound = EC.chain64(cpu(R), Ws, bs)
    g16, g32 = cpu(emb16).reshape(-1, 128), cpu(emb32).reshape(-1, 128)
    e32 = np.abs(g32 - ref)
    print("bf16 embed(): max |bf16 - fp32| %.3g, max |bf16 - fp32| / bound %.3f, |fp32 - fp64| %.3g"
          % (float(np.max(np.abs(g16 - g32))), float(np.max(np.abs(g16 - g32) / (bound + e32))), float(e32.max())))
    assert np.all(np.isfinite(g16)) and np.all(np.abs(g16 - g32) <= bound + e32)


@pytest.mark.parametrize("precision", ["f32", "b16"])
def test_embed_route(e2e, monkeypatch, precision):
    """Exactly one embedding launch, right behind fp1's prifit_fp_rows: no product for fp1, the head, conv2 or the embedding,
    and no row chain.  forward(embed=True) keeps its separate launches."""
    m = e2e[precision]
    entry = "prifit_mlp_chain_embed_" + ("f32" if precision == "f32" else "bf16")
    seen = []
    with monkeypatch.context() as mp:
        EC.spy_calls(mp, seen)
        m.embed(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"], l2_norm=True, return_labels=True)
        emb_calls = list(seen)
        seen.clear()
        m(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"], embed=True)
        fwd_calls = list(seen)
    assert sum(n.startswith("prifit_mlp_chain_embed") for n in emb_calls) == 1 and emb_calls.count(entry) == 1
    assert emb_calls.count("prifit_fp_rows") == 3
    tail = emb_calls[len(emb_calls) - 1 - emb_calls[::-1].index("prifit_fp_rows"):]
    assert tail == ["prifit_fp_rows", entry], tail
    assert not any("chain_rows" in n for n in emb_calls)
    assert not any("chain_embed" in n or "chain_rows" in n for n in fwd_calls)
    assert fwd_calls[len(fwd_calls) - 1 - fwd_calls[::-1].index("prifit_fp_rows"):].count("prifit_gemm_f32") >= 5

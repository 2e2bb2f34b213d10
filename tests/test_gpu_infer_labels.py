"""GPU: part labels from the frozen network (FrozenPartSeg.labels, csrc/infer.hip prifit_mlp_chain_rows_f32) -- the four-layer
row chain's scores against an fp64 numpy restatement with the separate-launch route as the yardstick of its error, its
arg-max against prifit_seg_metrics on the same scores (no tolerance), guard bands round every operand, and the method end
to end against FrozenPartSeg.predict()."""
import ctypes

import numpy as np
import pytest
import torch

import guard_common as GC

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
W_HID = 128


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _net(P, K0, CL, seed):
    """Seeded normal rows and weights of the tail: X [P, K0], W (128, 128, 128, CL) rows, b."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((P, K0)).astype(np.float32)
    Ws, bs, kin = [], [], K0
    for cout in (W_HID, W_HID, W_HID, CL):
        Ws.append((rng.standard_normal((cout, kin)) / np.sqrt(kin)).astype(np.float32))
        bs.append((0.1 * rng.standard_normal(cout)).astype(np.float32))
        kin = cout
    return X, Ws, bs


def _launch(X, Ws, bs, scores=None, labels=None, cat_of_label=None, shape_cat=None, N=None):
    from prifit_amd._lib import call, cur_stream
    P, K0 = X.shape
    p = lambda t: None if t is None else t.data_ptr()
    call("prifit_mlp_chain_rows_f32", X.data_ptr(), X.stride(0), P, K0, 4, _arr(ctypes.c_int32, [W.shape[0] for W in Ws]),
         _arr(ctypes.c_void_p, [W.data_ptr() for W in Ws]), _arr(ctypes.c_longlong, [W.stride(0) for W in Ws]),
         _arr(ctypes.c_void_p, [b.data_ptr() for b in bs]), p(scores), 0 if scores is None else scores.stride(0), p(labels),
         p(cat_of_label), p(shape_cat), P if N is None else N, None, cur_stream())
    torch.cuda.synchronize()


def _ref64(X, Ws, bs):
    """fp64 restatement -> (z_L [P, CL], scale [P, CL]): scale = sum_k |a_k| |w_k| + |b| of the last product -- what one
    rounding of that product is relative to."""
    a = X.astype(np.float64)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        W, b = W.astype(np.float64), b.astype(np.float64)
        if l == len(Ws) - 1:
            return a @ W.T + b, np.abs(a) @ np.abs(W).T + np.abs(b)
        a = np.maximum(a @ W.T + b, 0.0)


def _separate_route(X, Ws, bs):
    """The launches the chain replaces, as FrozenPartSeg._stack / _linear run them: fp1's two products (the second with the
    ReLU on load through the unit a_affine) and the ReLU launch, conv1 + bn1 and its ReLU launch, conv2 as a plain product."""
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
    return product(h, Ws[3], bs[3], False)


# (K0, CL): the issue's three, then the narrowest instantiation and a C_L that ends inside a lane's four channels
@pytest.mark.parametrize("K0,CL", [(152, 50), (160, 64), (152, 1), (8, 50), (64, 33)])
@pytest.mark.parametrize("P", [200, 1])
def test_scores_against_fp64_and_the_separate_launches(P, K0, CL):
    """P = 200: 7 waves, the last with 8 live rows; P = 1: a lone wave with one live row.  The chain's largest error against
    fp64 in units of u (sum_k |a_k| |w_k| + |b|) of the last product is at most twice that of the separate-launch route on
    the same inputs (another summation order over the same fp32 MFMA arithmetic)."""
    Xn, Wn, bn = _net(P, K0, CL, 1000 + 7 * K0 + CL + P)
    ref, scale = _ref64(Xn, Wn, bn)
    X = torch.from_numpy(Xn).cuda()
    Ws, bs = [torch.from_numpy(w).cuda() for w in Wn], [torch.from_numpy(b).cuda() for b in bn]
    scores = torch.full((P, CL), float("nan"), device="cuda")
    _launch(X, Ws, bs, scores=scores)
    got = scores.cpu().numpy().astype(np.float64)
    sep = _separate_route(X, Ws, bs).cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got))
    e_chain = float(np.max(np.abs(got - ref) / scale))
    e_sep = float(np.max(np.abs(sep - ref) / scale))
    print("rows chain K0=%d C_L=%d P=%d: chain %.3g u, separate launches %.3g u" % (K0, CL, P, e_chain / U, e_sep / U))
    assert e_chain <= 2.0 * e_sep


def _metrics_pred(scores, B, N, first_label, cat_of_label, restricted):
    """prifit_seg_metrics' pred on the same scores; the shape's category is that of target[b, 0] = first_label[b]."""
    from prifit_amd import ops
    CL = scores.shape[-1]
    target = torch.zeros(B, N, dtype=torch.int64, device="cuda")
    target[:, 0] = torch.as_tensor(first_label, device="cuda")
    return ops.seg_metrics(scores.reshape(B, N, CL), target, cat_of_label, restricted=restricted)[0].reshape(-1)


def test_labels_equal_seg_metrics_on_the_same_scores():
    """One launch gives scores and labels; prifit_seg_metrics ranks those scores.  cat_of_label interleaves three categories
    and leaves some parts without one; the fourth shape's first label has no category (-1 for all its rows); two input rows
    are NaN (every score NaN: the first allowed channel).  Then the same without a window against restricted=False."""
    B, N, K0, CL = 4, 50, 152, 50
    Xn, Wn, bn = _net(B * N, K0, CL, 77)
    Xn[7] = np.nan                                        # shape 0
    Xn[2 * N + 49] = np.nan                               # shape 2, the last of its rows
    X = torch.from_numpy(Xn).cuda()
    Ws, bs = [torch.from_numpy(w).cuda() for w in Wn], [torch.from_numpy(b).cuda() for b in bn]
    col = np.array([(c * 7 + c // 5) % 3 for c in range(CL)], dtype=np.int32)      # 0 1 2 interleaved, not periodic
    col[[0, 13, 49]] = -1
    first = [int(np.flatnonzero(col == 0)[2]), int(np.flatnonzero(col == 1)[0]), int(np.flatnonzero(col == 2)[5]), 13]
    cat_of_label = torch.from_numpy(col).cuda()
    shape_cat = cat_of_label[torch.tensor(first, device="cuda")].contiguous()       # what an evaluation loop passes
    assert shape_cat.tolist() == [0, 1, 2, -1]
    scores = torch.empty(B * N, CL, device="cuda")
    labels = torch.full((B * N,), -7, dtype=torch.int32, device="cuda")
    _launch(X, Ws, bs, scores=scores, labels=labels, cat_of_label=cat_of_label, shape_cat=shape_cat, N=N)
    assert bool(torch.isnan(scores[7]).all()) and bool(torch.isnan(scores[2 * N + 49]).all())
    pred = _metrics_pred(scores, B, N, first, cat_of_label, True)
    assert torch.equal(labels.long(), pred)
    lab = labels.cpu().numpy().reshape(B, N)
    assert np.all(lab[3] == -1)
    for b in range(3):
        assert np.all(col[lab[b]] == b)                                             # inside the window
        assert len(np.unique(lab[b])) > 1                                           # and decided by the scores
    assert lab[0, 7] == np.flatnonzero(col == 0)[0] and lab[2, 49] == np.flatnonzero(col == 2)[0]
    # labels alone (no scores pointer) are the same labels
    alone = torch.full((B * N,), -7, dtype=torch.int32, device="cuda")
    _launch(X, Ws, bs, labels=alone, cat_of_label=cat_of_label, shape_cat=shape_cat, N=N)
    assert torch.equal(alone, labels)
    # no window
    free = torch.full((B * N,), -7, dtype=torch.int32, device="cuda")
    _launch(X, Ws, bs, labels=free)
    assert torch.equal(free.long(), _metrics_pred(scores, B, N, first, cat_of_label, False))
    assert free[7] == 0 and free[2 * N + 49] == 0 and len(torch.unique(free)) > 3


def test_labels_ties_infinity_and_a_category_without_parts():
    """Channels 3 and 4 (the two lane halves of a block) share one row of W_4 / b_4, as do 8 and 9 (neighbours in one lane)
    and 21 and 38 (one lane, two blocks); each pair carries a bias that makes it the maximum of its category, so every row
    of that shape is a tie: the lower index wins.  Category 3 has +inf in channel 45; category 9 has no part."""
    B, N, K0, CL = 6, 35, 160, 50                          # 210 rows: the last wave has 18 live rows
    Xn, Wn, bn = _net(B * N, K0, CL, 78)
    col = np.array([c % 3 for c in range(CL)], dtype=np.int32)
    col[[3, 4, 20]] = 4
    col[[8, 9, 30]] = 5
    col[[21, 33, 38]] = 6
    col[[40, 45, 47]] = 3
    for lo, hi in ((3, 4), (8, 9), (21, 38)):
        Wn[3][hi] = Wn[3][lo]
        bn[3][lo] = bn[3][hi] = 100.0
    bn[3][45] = np.inf
    cats = [4, 5, 6, 3, 9, 1]
    X = torch.from_numpy(Xn).cuda()
    Ws, bs = [torch.from_numpy(w).cuda() for w in Wn], [torch.from_numpy(b).cuda() for b in bn]
    cat_of_label = torch.from_numpy(col).cuda()
    shape_cat = torch.tensor(cats, dtype=torch.int32, device="cuda")
    scores = torch.empty(B * N, CL, device="cuda")
    labels = torch.full((B * N,), -7, dtype=torch.int32, device="cuda")
    _launch(X, Ws, bs, scores=scores, labels=labels, cat_of_label=cat_of_label, shape_cat=shape_cat, N=N)
    s = scores.cpu().numpy()
    for lo, hi in ((3, 4), (8, 9), (21, 38)):
        assert np.array_equal(s[:, lo].view(np.int32), s[:, hi].view(np.int32))     # exact ties
    assert np.all(np.isposinf(s[:, 45]))
    lab = labels.cpu().numpy().reshape(B, N)
    assert np.all(lab[0] == 3) and np.all(lab[1] == 8) and np.all(lab[2] == 21) and np.all(lab[3] == 45) and np.all(lab[4] == -1)
    assert np.all(col[lab[5]] == 1)
    # prifit_seg_metrics on the same scores: the shapes that have a category (a first label selects it)
    first = [3, 8, 21, 40, 0, 1]
    pred = _metrics_pred(scores, B, N, first, cat_of_label, True).reshape(B, N)
    keep = [0, 1, 2, 3, 5]
    assert torch.equal(labels.reshape(B, N).long()[keep], pred[keep])


def test_guard_bands():
    """X, every W and b in NaN guards, scores [200, 50] with a row stride of 52 and labels in sentinel guards: every guard
    word and the two padding columns of scores unchanged, no output NaN."""
    P, K0, CL, lds, N = 200, 152, 50, 52, 40
    Xn, Wn, bn = _net(P, K0, CL, 79)
    tail = 1 << 14
    X = GC.guarded_like(torch.from_numpy(Xn).cuda(), tail, tail)[0]
    Ws = [GC.guarded_like(torch.from_numpy(w).cuda(), tail, tail)[0] for w in Wn]
    bs = [GC.guarded_like(torch.from_numpy(b).cuda(), tail, tail)[0] for b in bn]
    col = torch.tensor([c % 5 for c in range(CL)], dtype=torch.int32)
    cat_of_label = GC.guarded_like(col.cuda().view(torch.float32), 4096, 4096)[0].view(torch.int32)
    shape_cat = GC.guarded_like(torch.tensor([0, 4, 2, 1, 3], dtype=torch.int32).cuda().view(torch.float32), 4096, 4096)[0].view(torch.int32)
    scores, s_base = GC.guarded_matrix(P, CL, lds, 4096, 4096, poison=GC.SENTINEL)
    lab_f, l_base = GC.guarded((P,), 4096, 4096, poison=GC.SENTINEL)
    labels = lab_f.view(torch.int32)
    _launch(X, Ws, bs, scores=scores, labels=labels, cat_of_label=cat_of_label, shape_cat=shape_cat, N=N)
    GC.assert_guards_intact(s_base, scores)                 # the guards and columns 50, 51 of every row
    GC.assert_guards_intact(l_base, lab_f)
    assert bool(torch.isfinite(scores).all())
    lab = labels.cpu().numpy()
    assert np.all((lab >= 0) & (lab < CL))
    assert np.array_equal(lab % 5, np.repeat([0, 4, 2, 1, 3], N))
    ref, scale = _ref64(Xn, Wn, bn)
    # the data arrived (precision is the first test's subject): the worst case of an fp32 sum of K <= 160 terms is K u of
    # sum |a| |w| = 2e-5, four layers on top of each other stay below 1e-4
    assert np.all(np.abs(scores.cpu().numpy() - ref) <= 1e-4 * scale)


# ---------------------------------------------------------------------------------------------- end to end
def _seeded_model(normal, seed):
    """get_model(50) with seeded weights, BatchNorm gamma / beta and running statistics, all drawn on the CPU: the same
    state on every machine, so the share of undecided points below is a property of the seed."""
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


E2E_SEED = {False: 5, True: 6}


@pytest.fixture(scope="module", params=[(False, 2), (True, 1)], ids=["xyz_B2", "normals_B1"])
def e2e(request):
    from prifit_amd import inference, testing as T
    from test_gpu_inference import _inputs, _ref64 as net_ref64
    normal, B = request.param
    net = _seeded_model(normal, E2E_SEED[normal])
    frozen = inference.freeze(net)
    xyz, onehot, start = _inputs(B, 6 if normal else 3, 1024, 11)
    with torch.no_grad():
        live = net(xyz, onehot, fps_start=start)[0]
    ref_seg = net_ref64(frozen, xyz, onehot, start)[0]
    col = T.SegmentationEvaluator().cat_of_label                        # int64 [50] on the host, as an evaluation loop has it
    shape_cat = onehot.reshape(B, 16).argmax(dim=1)                     # the cloud's category
    torch.cuda.synchronize()
    return dict(net=net, frozen=frozen, xyz=xyz, onehot=onehot, start=start, live=live, ref_seg=ref_seg, col=col,
                shape_cat=shape_cat, B=B)


def test_labels_end_to_end_against_predict(e2e):
    """scores - logsumexp(scores) is predict()'s log-probability within the bar of the existing end-to-end test (twice the
    live route's error against fp64), and labels is the restricted arg-max of predict() wherever the fp64 top-2 gap inside
    the window exceeds twice that bar; at most 1 % of the points may be closer than that.  The seeds were picked on
    an fp64 CPU run of the same network (1 of 2048 points within 1e-5, none of 1024 with normals); found on the GPU with the
    measured bars (1.45e-6 and 1.49e-6): xyz B = 2: 1 of 2048 points left out; normals B = 1: 0 of 1024."""
    frozen, col, shape_cat, B = e2e["frozen"], e2e["col"], e2e["shape_cat"], e2e["B"]
    seg = frozen.predict(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"])
    labels, scores = frozen.labels(e2e["xyz"], e2e["onehot"], shape_cat, col, fps_start=e2e["start"], return_scores=True)
    assert labels.shape == (B, 1024) and labels.dtype == torch.int32 and scores.shape == (B, 1024, 50)
    bar = 2.0 * float((e2e["live"].double().cpu() - e2e["ref_seg"]).abs().max())
    logp = torch.log_softmax(scores.double(), dim=-1)
    diff = float((logp - seg.double()).abs().max())
    print("labels(): |scores - logsumexp - predict| %.3g, bar %.3g" % (diff, bar))
    assert diff <= bar
    allowed = (col.view(1, 1, -1) == shape_cat.cpu().view(-1, 1, 1))
    assert bool(allowed.any(dim=-1).all())
    top2 = e2e["ref_seg"].masked_fill(~allowed, float("-inf")).topk(2, dim=-1).values
    sure = (top2[..., 0] - top2[..., 1]) > 2.0 * bar
    want = seg.cpu().masked_fill(~allowed, float("-inf")).argmax(dim=-1)
    left_out = int((~sure).sum())
    print("labels(): %d of %d points closer than twice the bar" % (left_out, sure.numel()))
    assert left_out <= 0.01 * sure.numel()
    assert torch.equal(labels.cpu().long()[sure], want[sure])
    # without a window: the plain arg-max, on the same points' unrestricted gap
    free = frozen.labels(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"])
    top2 = e2e["ref_seg"].topk(2, dim=-1).values
    sure = (top2[..., 0] - top2[..., 1]) > 2.0 * bar
    assert int((~sure).sum()) <= 0.01 * sure.numel()
    assert torch.equal(free.cpu().long()[sure], seg.cpu().argmax(dim=-1)[sure])


def test_labels_route_and_refresh(e2e, monkeypatch):
    """One chain launch; after fp1's prifit_fp_rows no product, no ReLU launch and no log_softmax.  refresh() after a live
    weight changed moves the scores; the old weights bring the old labels back."""
    import prifit_amd.inference as I
    import prifit_amd.models.pointnet_util as PU
    import prifit_amd.nn_ops as NN
    import prifit_amd.ops as O
    from prifit_amd import _lib
    frozen, net = e2e["frozen"], e2e["net"]
    args = (e2e["xyz"], e2e["onehot"], e2e["shape_cat"], e2e["col"])
    before = frozen.labels(*args, fps_start=e2e["start"], return_scores=True)
    seen = []

    def spy(name, *a):
        seen.append(name)
        return _lib.call(name, *a)

    def no_log_softmax(*a, **k):
        seen.append("log_softmax")
        raise AssertionError("labels() called log_softmax")

    with monkeypatch.context() as mp:
        for mod in (I, PU, NN, O):
            mp.setattr(mod, "call", spy)
        mp.setattr(I.F, "log_softmax", no_log_softmax)
        mp.setattr(torch, "log_softmax", no_log_softmax)
        again = frozen.labels(*args, fps_start=e2e["start"], return_scores=True)
    assert torch.equal(again[0], before[0]) and torch.equal(again[1], before[1])
    assert seen.count("prifit_mlp_chain_rows_f32") == 1 and seen[-1] == "prifit_mlp_chain_rows_f32"
    assert seen.count("prifit_mlp_chain_pool_f32") == 5 and seen.count("prifit_fp_rows") == 3
    tail = seen[len(seen) - 1 - seen[::-1].index("prifit_fp_rows"):]
    assert tail == ["prifit_fp_rows", "prifit_mlp_chain_rows_f32"], tail
    assert "log_softmax" not in seen
    # forward() still takes its own route: no row chain
    seen.clear()
    with monkeypatch.context() as mp:
        for mod in (I, PU, NN, O):
            mp.setattr(mod, "call", spy)
        frozen(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"])
    assert "prifit_mlp_chain_rows_f32" not in seen and seen.count("prifit_mlp_chain_pool_f32") == 5
    # refresh
    saved = net.conv2.bias.detach().clone(), net.fp1.mlp_convs[0].weight.detach().clone()
    try:
        with torch.no_grad():
            net.conv2.bias[3] += 0.5
            net.fp1.mlp_convs[0].weight.mul_(1.25)
        same = frozen.labels(*args, fps_start=e2e["start"], return_scores=True)
        assert torch.equal(same[1], before[1])                          # the snapshot does not move ...
        frozen.refresh()
        moved = frozen.labels(*args, fps_start=e2e["start"], return_scores=True)
        assert not torch.equal(moved[1], before[1])                     # ... refresh() does
        seg = frozen.predict(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"])
        assert float((torch.log_softmax(moved[1], dim=-1) - seg).abs().max()) < 1e-4
    finally:
        with torch.no_grad():
            net.conv2.bias.copy_(saved[0])
            net.fp1.mlp_convs[0].weight.copy_(saved[1])
        frozen.refresh()
    back = frozen.labels(*args, fps_start=e2e["start"], return_scores=True)
    assert torch.equal(back[0], before[0]) and torch.equal(back[1], before[1])


def test_labels_argument_errors(e2e):
    frozen = e2e["frozen"]
    with pytest.raises(ValueError):
        frozen.labels(e2e["xyz"], e2e["onehot"], shape_cat=e2e["shape_cat"])
    with pytest.raises(ValueError):
        frozen.labels(e2e["xyz"], e2e["onehot"], cat_of_label=e2e["col"])
    with pytest.raises(ValueError):
        frozen.labels(e2e["xyz"], e2e["onehot"], e2e["shape_cat"], e2e["col"][:49])
    with pytest.raises(ValueError):
        frozen.labels(e2e["xyz"], e2e["onehot"], e2e["shape_cat"].float(), e2e["col"])

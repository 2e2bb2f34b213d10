"""The restatements of tests/cluster_select_common.py on hand-made inputs whose answers are written out here, and the conditions
under which float32 and float64 take the same discrete decisions, asserted on every input family that
tests/test_gpu_cluster_select_guards.py uses (CPU only).

Measured here: the smallest float64 top-two margin of a label in the separated-cluster shapes (bandwidth 0.3, N >= 63) is
0.66 over all nms and nms_pair cases (the float32 dot products are off by at most 7.8e-7), so nothing is left out there; in
the shapes where every point is its own centre (more centres than the cap at N > 64: the labels are taken over the first 64)
at most 1 point of a case falls under 8 x the float32 error (cap: 1 %; a draw above the cap is drawn again).  Membership leaves out 0 elements of any case."""
import numpy as np
import pytest
import torch

import cluster_select_common as cc
from cluster_select_common import F32, F64

INF = float("inf")


def i64(*v):
    return torch.tensor(v, dtype=torch.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# hand-made inputs
# ---------------------------------------------------------------------------------------------------------------------------
def test_first_extremes_take_the_lowest_index():
    M = torch.tensor([[3.0, 1.0, 1.0, 2.0], [0.0, -0.0, 5.0, 5.0], [7.0, 7.0, 7.0, 7.0]])
    v, i = cc.first_min(M, 1)
    assert v.tolist() == [1.0, 0.0, 7.0] and i.tolist() == [1, 0, 0]          # (+0 and -0 are one value)
    v, i = cc.first_max(M, 1)
    assert v.tolist() == [3.0, 5.0, 7.0] and i.tolist() == [0, 2, 0]
    v, i = cc.first_min(M, 0)
    assert v.tolist() == [0.0, -0.0, 1.0, 2.0] and i.tolist() == [1, 1, 0, 0]


def test_float_key_orders_like_the_floats():
    x = torch.tensor([-INF, -2.0, -1e-30, 0.0, 1e-30, 1.0, 1.0 + 2.0 ** -23, INF])
    k = cc.float_key(x)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert int(cc.float_key(torch.tensor([1.0]))[0]) == 0x3f800000 | 0x80000000
    assert int(cc.float_key(torch.tensor([-1.0]))[0]) == (~0xbf800000) & 0xffffffff


def test_owner_keys_hand_made():
    """Column minima of a symmetric 4 x 4 matrix: column 0 -> 0.0 at row 0, column 1 -> -0.5 at row 2 (not its own diagonal),
    column 2 -> -0.5 at row 1, column 3 -> the tie 0.25 at rows 0 and 3 resolved to row 0."""
    C = torch.tensor([[0.0, 1.0, 2.0, 0.25],
                      [1.0, 0.5, -0.5, 3.0],
                      [2.0, -0.5, 0.0, 1.0],
                      [0.25, 3.0, 1.0, 0.25]])
    keys = cc.owner_keys(C).numpy().view(np.uint64)
    assert [int(k) & 0xffffffff for k in keys] == [0, 2, 1, 0]
    hi = [int(k) >> 32 for k in keys]
    assert hi == [0x80000000, (~0xbf000000) & 0xffffffff, (~0xbf000000) & 0xffffffff, 0x3e800000 | 0x80000000]


def test_pack_mask_hand_made():
    near = torch.zeros(2, 64, dtype=torch.bool)
    near[0, 0] = near[0, 31] = near[0, 33] = True
    near[1, 63] = True
    w = cc.pack_mask(near).numpy().view(np.uint32)
    assert w.tolist() == [[0x80000001, 0x2], [0x0, 0x80000000]]
    assert torch.equal(cc.unpack_mask(cc.pack_mask(near), 64), near)


# five points: 0, 1, 2 close together, 3 and 4 close together (chord distances, symmetric)
D5 = torch.tensor([[0.00, 0.10, 0.10, 1.00, 1.20],
                   [0.10, 0.00, 0.05, 1.10, 1.00],
                   [0.10, 0.05, -0.01, 1.00, 1.00],
                   [1.00, 1.10, 1.00, 0.30, 0.20],
                   [1.20, 1.00, 1.00, 0.20, 0.25]])


def test_nms_select_hand_made():
    """Owners (first row minimum): 0 -> 0, 1 -> 1, 2 -> 2 (-0.01), 3 -> 4 (0.20), 4 -> 3 (0.20).  counts = 1 1 1 1 1.
    thr 0.15: centre 0 sees {0, 1, 2}, all count 1: first = 0; centre 1 -> 0; centre 2 -> 0; centre 3 sees nothing below 0.15:
    every entry 0, first maximum = column 0; centre 4 likewise.  One flag: id 0."""
    out = cc.nms_select(D5, D5 < 0.15, cap=4)
    assert out["owner"].tolist() == [0, 1, 2, 4, 3] and out["counts"].tolist() == [1, 1, 1, 1, 1]
    assert out["flags"].tolist() == [1, 0, 0, 0, 0] and out["count"] == 1 and out["ids"].tolist() == [0, 0, 0, 0]
    # thr 0.22: centres 3 and 4 see each other but not themselves (0.30, 0.25): 3 -> 4, 4 -> 3
    out = cc.nms_select(D5, D5 < 0.22, cap=4)
    assert out["flags"].tolist() == [1, 0, 0, 1, 1] and out["count"] == 3 and out["ids"].tolist() == [0, 3, 4, 0]


def test_nms_select_counts_decide_and_cap_truncates():
    """Owner given (the keys' route): points 0..5 owned by 2, 2, 2, 5, 5, 1 -> counts 0 1 3 0 0 2.  Every centre sees every
    centre: the owning centres 1, 2, 5 all pick the first maximum count: 2.  With a diagonal-only neighbourhood the owning
    centres pick themselves: flags at 1, 2, 5; cap 2 keeps ids 1, 2 and count stays 3."""
    owner = i64(2, 2, 2, 5, 5, 1)
    out = cc.nms_select(None, torch.ones(6, 6, dtype=torch.bool), cap=2, owner=owner)
    assert out["counts"].tolist() == [0, 1, 3, 0, 0, 2] and out["flags"].tolist() == [0, 0, 1, 0, 0, 0]
    assert out["count"] == 1 and out["ids"].tolist() == [2, 0]
    out = cc.nms_select(None, torch.eye(6, dtype=torch.bool), cap=2, owner=owner)
    assert out["flags"].tolist() == [0, 1, 1, 0, 0, 1] and out["count"] == 3 and out["ids"].tolist() == [1, 2]


def test_nms_labels_hand_made():
    """Centres = points 1 and 3 of four 2-D points; dot products written out; a point with equal dot products takes the first centre."""
    X = torch.tensor([[1.0, 0.0], [0.8, 0.6], [0.0, 1.0], [-0.6, 0.8]])
    lab, margin, second, d = cc.nms_labels(X, X, i64(1, 3, 0, 0), 2, cap=4)
    assert torch.allclose(d, torch.tensor([[0.8, -0.6], [1.0, 0.0], [0.6, 0.8], [0.0, 1.0]], dtype=F64))
    assert lab.tolist() == [0, 0, 1, 1] and second.tolist() == [1, 1, 0, 0]
    assert torch.allclose(margin, torch.tensor([1.4, 1.0, 0.2, 1.0], dtype=F64))
    Cen = X.clone()
    X[2] = 0.0                                               # both dot products 0: a tie, the first centre
    lab, margin, _, _ = cc.nms_labels(X, Cen, i64(1, 3, 0, 0), 2, cap=4)
    assert lab[2] == 0 and float(margin[2]) == 0.0
    # a count above the cap: labels over the first `cap` centres only; one centre: margin inf
    lab, margin, _, d = cc.nms_labels(X, X, i64(3, 0), 5, cap=1)
    assert d.shape == (4, 1) and lab.tolist() == [0, 0, 0, 0] and bool(torch.isinf(margin).all())


def test_nms_reference_leaves_out_the_tie_only():
    """Point 2 = (0.1, 0.7): 0.08 + 0.42 and -0.06 + 0.56, equal but for the rounding of the float32 inputs (margin 1.6e-8)."""
    X = torch.tensor([[1.0, 0.0], [0.8, 0.6], [0.1, 0.7], [-0.6, 0.8]])
    dist = 1.0 - torch.eye(4)                                # every point its own owner
    near = torch.eye(4, dtype=torch.bool)
    near[0, 1] = near[2, 1] = near[2, 2] = True
    near[0, 0] = False                                      # 0 -> 1, 1 -> 1, 2 -> first of {1, 2} = 1, 3 -> 3
    out = cc.nms_reference(dist, near, X, X, cap=4)
    assert out["owner"].tolist() == [0, 1, 2, 3] and out["ids"].tolist() == [1, 3, 0, 0] and out["count"] == 2
    assert out["left"].tolist() == [False, False, True, False]
    assert out["used_lo"].tolist() == [1, 1, 0, 0] and out["used_hi"].tolist() == [1, 1, 0, 0]


def test_kth_expected_hand_made():
    M = torch.tensor([[4.0, -1.0, 0.0, -0.0, 4.0, 2.0]])
    assert [float(cc.kth_expected(M, k)) for k in range(1, 7)] == [-1.0, 0.0, 0.0, 2.0, 4.0, 4.0]


def test_membership_hand_made():
    """b = 1, gmax = 0: s = the dot products.  Row (0, ln 3, -20 | dead): e = 1, 3, exp(-13) -> W = e / (4 + exp(-13)); the
    clamped slot has no gradient of its own.  count = 0: all zero."""
    d = torch.tensor([[[0.0, np.log(3.0), -20.0, 9.0]], [[1.0, 2.0, 3.0, 4.0]]], dtype=F64)
    case = dict(dots=d, bw=torch.ones(2), gmax=torch.zeros(2), count=i64(3, 0), gW=torch.tensor([[[1.0, 0.0, 0.0, 5.0]]] * 2))
    W, s, live = cc.membership(d, case["bw"], case["gmax"], case["count"])
    tot = 4.0 + np.exp(-13.0)
    assert torch.allclose(W[0, 0], torch.tensor([1 / tot, 3 / tot, np.exp(-13.0) / tot, 0.0], dtype=F64), rtol=1e-14, atol=0)
    assert float(W[1].abs().max()) == 0.0 and live[0, 0].tolist() == [True, True, True, False]
    ref = cc.membership_reference(case)
    w0, w1 = 1 / tot, 3 / tot
    assert torch.allclose(ref["g64"][0, 0], torch.tensor([w0 * (1 - w0), -w0 * w1, 0.0, 0.0], dtype=F64), rtol=1e-12, atol=0)
    assert float(ref["g64"][1].abs().max()) == 0.0
    assert ref["clamped"][0, 0].tolist() == [False, False, True, False] and not bool(ref["left"].any())


def test_normalize2_hand_made():
    x = torch.tensor([[3.0, 4.0], [0.0, 0.0], [6e-14, 8e-14], [0.0, 1e-20]], dtype=F64)
    y = cc.normalize2(x)
    assert torch.allclose(y, torch.tensor([[0.6, 0.8], [0.0, 0.0], [0.6, 0.8], [0.0, 1.0]], dtype=F64), rtol=1e-14, atol=0)
    case = dict(x=x, g=torch.tensor([[1.0, 0.0]] * 4, dtype=F64))
    _, gx, n1, n2 = cc.normalize2_reference(case)
    # row 0: (g - y (g.y)) / 5 = (1 - 0.36, -0.48) / 5; zero row: y = x / eps / eps, gx = g / eps^2; row 2 (norm 1e-13 < eps): the
    # first normalisation is x / eps (norm 0.1), the second a true one: gx = (g - y (g.y)) / 0.1 / eps
    assert torch.allclose(gx[0], torch.tensor([0.128, -0.096], dtype=F64), rtol=1e-13, atol=0)
    assert torch.allclose(gx[1], torch.tensor([1e24, 0.0], dtype=F64), rtol=1e-13, atol=0)
    assert torch.allclose(gx[2], torch.tensor([0.64e13, -0.48e13], dtype=F64), rtol=1e-12, atol=0)
    assert torch.allclose(n1, torch.tensor([5.0, 0.0, 1e-13, 1e-20], dtype=F64), rtol=1e-14, atol=0)
    assert torch.allclose(n2, torch.tensor([1.0, 0.0, 0.1, 1e-8], dtype=F64), rtol=1e-14, atol=0)


def test_update_hand_made():
    """O / rowsum = (3, 4): out = (0.6, 0.8), |new| = 5 whatever Z is; gO = (g - out (g.out)) / 5 / rowsum,
    g_rowsum = -(gnew . (3, 4)) / rowsum = 0 (gnew is orthogonal to out)."""
    case = dict(O=torch.tensor([[6.0, 8.0]], dtype=F64), rowsum=torch.tensor([2.0], dtype=F64), Z=torch.tensor([[0.0, 1.0]], dtype=F64),
                g=torch.tensor([[1.0, 0.0]], dtype=F64))
    out, nrm, gO, grs = cc.update_reference(case)
    assert torch.allclose(out, torch.tensor([[0.6, 0.8]], dtype=F64), rtol=1e-14, atol=0) and abs(float(nrm) - 5.0) < 1e-14
    assert torch.allclose(gO, torch.tensor([[0.064, -0.048]], dtype=F64), rtol=1e-12, atol=0)
    assert abs(float(grs)) < 1e-16


def test_update_bwd_free_formula():
    """out_free = (0, 1) at an angle to O / rowsum = (3, 4), nrm_free = 2, g = (1, 0): gnew = (1, 0) / 2, gO = gnew / 2,
    g_rowsum = -(0.5 * 6) / 4; with the forward's own out and nrm the formula is the autograd result."""
    case = dict(O=torch.tensor([[6.0, 8.0]], dtype=F64), rowsum=torch.tensor([2.0], dtype=F64), Z=torch.tensor([[0.0, 1.0]], dtype=F64),
                g=torch.tensor([[1.0, 0.0]], dtype=F64), out_free=torch.tensor([[0.0, 1.0]], dtype=F64), nrm_free=torch.tensor([2.0], dtype=F64))
    gO, grs = cc.update_bwd_free(case)
    assert gO.tolist() == [[0.25, 0.0]] and grs.tolist() == [-0.75]
    case = cc.update_inputs((7,), 5, "formula")
    out, nrm, gO64, grs64 = cc.update_reference(case)
    case["out_free"], case["nrm_free"] = out, nrm
    gO, grs = cc.update_bwd_free(case)
    assert float((gO - gO64).abs().max()) < 1e-15 and float((grs - grs64).abs().max()) < 1e-15
    free = cc.update_free_inputs(case, "formula")
    cos = (free["out_free"].double() * out).sum(-1)
    assert float(cos.max()) < 0.95 and float((free["out_free"].double().norm(dim=-1) - 1).abs().max()) < 1e-6


def test_dots_float32_is_sequential_and_symmetric():
    A = cc.separated(40, 32, "dots")
    d32, d64 = cc.dots(A, A, F32), cc.dots(A, A, F64)
    assert d32.dtype == F32 and torch.equal(d32, d32.t())
    acc = np.float32(0.0)
    for k in range(32):
        acc = np.float32(acc + np.float32(A[3, k].item()) * np.float32(A[17, k].item()))
    assert float(d32[3, 17]) == float(acc)
    assert float((d32.double() - d64).abs().max()) < 32 * 2.0 ** -24
    c = cc.chord_input(A)
    assert torch.equal(c, c.t())


# ---------------------------------------------------------------------------------------------------------------------------
# every input family: the decisions float32 and float64 share
# ---------------------------------------------------------------------------------------------------------------------------
STATS = {}


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("D", cc.NMS_D)
@pytest.mark.parametrize("N", cc.NMS_N)
def test_nms_families(N, D, pair):
    case = cc.nms_case(N, D, pair)
    refs = case["refs"]
    for fam, ref in zip(cc.NMS_FAMILY, refs):
        cc.assert_left_out(ref["left"], none=(fam != "own_centre"), what="%s N=%d D=%d" % (fam, N, D))
        assert 1 <= ref["count"] <= N and int(ref["flags"].sum()) == ref["count"] and int(ref["counts"].sum()) == N
        assert ref["ids"][:min(ref["count"], cc.NMS_CAP)].tolist() == sorted(torch.nonzero(ref["flags"]).view(-1).tolist())[:cc.NMS_CAP]
        if fam == "separated" and ref["count"] > 1 and N >= 63:
            STATS["margin"] = min(STATS.get("margin", INF), float(ref["margin"].min()))
        STATS["err32"] = max(STATS.get("err32", 0.0), ref["err32"])
        STATS["left"] = max(STATS.get("left", 0), int(ref["left"].sum()))
    if not pair:
        assert refs[0]["count"] == N and refs[0]["owner"].tolist() == list(range(N))      # every owner keeps itself
        assert (refs[0]["count"] > cc.NMS_CAP) == (N > cc.NMS_CAP)
    assert refs[1]["count"] == 1 and float(refs[1]["labels"].abs().max()) == 0            # one centre remains
    if N >= 63:
        assert 2 <= refs[2]["count"] <= 6                                                 # one per cluster
    print("smallest separated margin %.3g, largest float32 dot error %.3g, most left out %d" % (STATS.get("margin", INF), STATS["err32"], STATS["left"]))


@pytest.mark.parametrize("D", cc.MASK_D)
@pytest.mark.parametrize("N", cc.MASK_N)
def test_nms_mask_families(N, D):
    case = cc.mask_case(N, D)
    dist = cc.chord(case["X"], case["X"], F32)
    for z, none in ((0, False), (1, True)):
        near = dist[z] < case["bw"][z]
        ref = cc.nms_reference(dist[z], near, case["X"][z], case["X"][z])
        cc.assert_left_out(ref["left"], none=none, what="mask N=%d D=%d shape %d" % (N, D, z))
        if z == 0:
            assert ref["count"] == N
            if N == 2176:       # a centre whose pick lies under the mask words 64 .. 67
                assert int(ref["flags"][2048:].sum()) == 128
        hand = cc.handmade_mask(near, ref["counts"])
        ref2 = cc.nms_reference(dist[z], hand, case["X"][z], case["X"][z])
        assert int(ref2["flags"][0]) == 1                    # no neighbour with a count: column 0
        cc.assert_left_out(ref2["left"], none=none, what="hand-made mask N=%d D=%d shape %d" % (N, D, z))
        assert torch.equal(cc.unpack_mask(cc.pack_mask(hand), N), hand)


@pytest.mark.parametrize("family", sorted(cc.FAMILIES))
def test_sym_families(family):
    """What the families are for: collapsed -- all rows within 1e-7, exact ties and negative distances in float32; duplicated --
    the same row in different 128-row tiles; all of them unit rows, keys and mask restated without overflow."""
    n, K = 256, 64
    A = torch.stack([cc.FAMILIES[family](n, K, z) for z in range(2)])
    assert float((A.double().norm(dim=2) - 1).abs().max()) < 1e-6
    C = cc.chord(A, A, F32)
    assert torch.equal(C, C.transpose(1, 2))
    if family == "collapsed":
        assert float((A - A[:, :1]).abs().max()) <= 1e-7
        assert bool((C < 0).any()) and torch.unique(C).numel() < C.numel() // 100
    if family == "duplicated":
        assert torch.equal(A[0, 5], A[0, 133]) and torch.equal(A[0, 127], A[0, 255])
        _, arg = cc.first_min(C[0], 0)
        assert int(arg[133]) in (5, 133)
    keys = cc.owner_keys(C).numpy().view(np.uint64)
    _, arg = cc.first_min(C, 1)
    assert torch.equal(torch.from_numpy((keys & np.uint64(0xffffffff)).astype(np.int64)), arg)
    thr = cc.thresholds(C, 0)
    bits = [int((C[z] < thr[z]).sum()) for z in range(2)]
    assert bits[0] == 0 and bits[1] == n * n
    thr = cc.thresholds(C, 2)
    assert bool((C[0] == thr[0]).any()) and 0 < int((C[0] < thr[0]).sum()) < n * n


@pytest.mark.parametrize("KM", cc.MEM_KM)
@pytest.mark.parametrize("N", cc.MEM_N)
def test_membership_families(N, KM):
    case = cc.membership_case(N, KM)
    ref = cc.membership_reference(case)
    cc.assert_left_out(ref["left"], none=False, what="membership N=%d KM=%d" % (N, KM))
    s, live = ref["s64"], ref["live"]
    assert case["count"].tolist() == [0, 1, (KM + 1) // 2, KM + 7]
    assert not bool(live[0].any()) and bool(live[3].all())
    if N * KM >= 255:
        for z in (2, 3):       # all three regions of the clamp on live elements
            assert bool((s[z][live[z]] < cc.CLAMP_LO).any()) and bool((s[z][live[z]] > cc.CLAMP_HI).any())
            assert bool(((s[z] > cc.CLAMP_LO) & (s[z] < cc.CLAMP_HI))[live[z]].any())
    rows = ref["W64"].sum(-1)
    assert float((rows[1:] - 1).abs().max()) < 1e-12 and float(ref["W64"][0].abs().max()) == 0
    assert float(ref["g64"][~live].abs().max() if bool((~live).any()) else 0) == 0
    assert float(ref["g64"][ref["clamped"]].abs().max() if bool(ref["clamped"].any()) else 0) == 0


@pytest.mark.parametrize("D", cc.ROW_D)
@pytest.mark.parametrize("rows", cc.ROW_ROWS)
def test_normalize2_families(rows, D):
    """Both norms of every row are far from eps on either side (a factor of 5 at the least): float32 and float64 take the same
    branch of both clamps, nothing is left out."""
    case = cc.normalize2_case(rows, D)
    for dtype in (F32, F64):
        y, gx, n1, n2 = cc.normalize2_reference(case, dtype)
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gx).all())
        for n in (n1, n2):
            assert bool(((n >= 5 * cc.EPS_NORM) | (n <= 0.2 * cc.EPS_NORM)).all())
    if rows > 1:
        assert sorted(set(case["cls"].tolist())) == [0, 1, 2, 3]
        assert float(n1[1]) == 0 and abs(float(n1[2]) / 1e-13 - 1) < 1e-5 and abs(float(n1[rows - 1]) / 1e-20 - 1) < 1e-5


@pytest.mark.parametrize("C", cc.KTH_C)
def test_kth_families(C):
    for family in cc.KTH_FAMILIES:
        for k in cc.kth_ks(C):
            M = cc.kth_rows(family, 5, C, k)
            assert M.shape == (5, C) and M.dtype == F32
            kth = cc.kth_expected(M, k)
            below, upto = (M < kth.view(-1, 1)).sum(1), (M <= kth.view(-1, 1)).sum(1)
            assert bool((below < k).all()) and bool((upto >= k).all())
            if family == "distinct" or family == "shared_top_bits":
                assert all(torch.unique(M[r]).numel() == C for r in range(5))
            if family == "three_values" and C > 3 * 256 + 64:
                assert bool((upto > 256).all()) or k > 256        # more keys <= the answer than the fast path's 256 slots
            if family == "kth_duplicated" and C >= 8:
                assert bool(((M == kth.view(-1, 1)).sum(1) >= 3).all())
    assert cc.kth_ks(C)[0] == 1 and cc.kth_ks(C)[-1] == C

"""The cluster-selection kernels -- chord_sym_kernel of csrc/gemm.hip in its three modes, and of csrc/meanshift.hip the k-th
smallest entry, nms / nms_mask / nms_pair, the membership, the double normalisation and the mean-shift update -- at edge
shapes through the C ABI, every float or int tensor a kernel reads inside NaN (int: in-range poison) guard bands, every tensor
it writes inside sentinel guards (tests/guard_common.py), against the restatements of tests/cluster_select_common.py.

Each case asserts, in this order: outputs finite and written, guards intact, exact properties (everything discrete: keys, mask,
owner, counts, flags, ids, count, labels and used outside the left-out points, the k-th value, dead slots, bitwise symmetry),
then the bars: for every continuous quantity max |kernel - fp64| / max |fp64| at most 4 x the same error of the float32
restatement of the formula on the same inputs, computed in the test (floor 4 x 2^-24).  The conditions under which float32
and float64 take the same discrete decisions are asserted on every input family by tests/test_cluster_select_restatement.py.

Measured on an MI355X (the case with the largest ratio of each quantity: kernel error, float32 restatement's error, their
ratio with the restatement's error floored at 2^-24; the bar is a ratio of 4):

  quantity          kernel   fp32     ratio       quantity          kernel   fp32     ratio
  sym_chord         1.1e+01  8.3e+00   1.38        n2_gx:norm_1e-13  1.2e-07  3.9e-08   2.03
  sym_gram          2.4e-07  1.8e-07   1.38        n2_y:norm_1e-20   7.1e-08  4.9e-08   1.20
  mem_W             1.1e-06  1.0e-06   1.06        n2_gx:norm_1e-20  1.4e-07  5.9e-08   2.29
  mem_gdots         1.7e-06  1.5e-06   1.14        upd_out           9.6e-08  4.1e-08   1.61
  n2_y:regular      8.6e-08  6.5e-08   1.31        upd_nrm           1.2e-07  7.6e-08   1.52
  n2_gx:regular     8.4e-08  5.5e-08   1.41        upd_gO            1.3e-07  6.9e-08   1.90
  n2_y:zero         0.0e+00  0.0e+00   0.00        upd_gO_free       1.4e-07  4.8e-08   2.35
  n2_gx:zero        8.3e-08  8.3e-08   1.00        upd_g_rowsum      2.0e-07  4.6e-08   3.29
  n2_y:norm_1e-13   6.9e-08  6.9e-08   1.00        upd_g_rowsum:gap  2.6e-07  1.3e-07   2.04

(sym_chord's worst case is the collapsed cloud, whose float64 distances are ~1e-8 at the largest: both errors are a few ulp
of 1 relative to that; on the separated clusters the chord errors are 1.2e-7 against 9e-8.)  Everything discrete was exact
at the first run and no kernel needed a change.

g_rowsum of the update's backward is identically zero when `out` is the forward's own (the normalisation removes the scale
1 / rowsum): the kernel and float64 autograd both return the rounding of a cancelled sum, errors "relative" to 1e-17.  It is
therefore measured on an `out` at an angle to O (cluster_select_common.update_bwd_free); with the forward's own `out` only
gO is compared.

Mutations of the kernel sources, each run against this module (none committed):
  `<` -> `<=` in the owner_key compare of chord_sym_kernel ........ 4 of 12 cases at n = 256 fail (duplicated, collapsed)
  the lanes' word loop of nms_pick_mask_kernel makes one trip ..... the two N = 2176 cases fail
  `pos < cap` removed in nms_compact_kernel ....................... 23 of 40 float-route cases fail
  min(count[b], KM) -> count[b] in membership_fwd_kernel .......... 21 of 25 cases fail
  N - 1 -> N in the clamped load of nms_owner_kernel .............. survives: the value loaded for c >= N is never used
      (`c < N &&` in the compare), so the mutant computes the same thing; inside guard bands the read past the matrix is a
      legal one, and no test that stays inside its allocations can tell the two apart
  k <= 256 -> k <= 257 in the k-th value's fast path ............... survives: an equivalent mutant.  At k = 257 the candidate
      set is still the 4 x 64 smallest keys per lane, fewer than k, so the bound t0 becomes the top of the bracket, every key of
      the row (C >= 257 of them) is taken, n0 > 256 and the kernel falls through to the general bisection: the same value
"""
import ctypes

import pytest
import torch

import cluster_select_common as cc
from cluster_select_common import F32, F64
from guard_common import BUFS_LEAD, BUFS_TAIL, SENTINEL, Bufs, assert_guards_intact, guarded, padded_stream, poison_bits

pytestmark = pytest.mark.gpu

NAN = float("nan")
LL = ctypes.c_longlong
CAP = cc.NMS_CAP
UNWRITTEN = poison_bits(SENTINEL)
EPS = ctypes.c_float(cc.EPS_NORM)


@pytest.fixture(scope="module")
def A(hiplib):
    assert torch.cuda.is_available()
    from prifit_amd import _lib
    return _lib


def finite(*ts):
    torch.cuda.synchronize()
    for t in ts:
        assert bool(torch.isfinite(t).all()), "non-finite output"


def written(*ts):
    """No word of an int output still holds the sentinel."""
    torch.cuda.synchronize()
    for t in ts:
        assert not bool((t.view(torch.int32) == UNWRITTEN).any()), "output not written"


def exact(name, got, want):
    got, want = got.detach().cpu().to(torch.int64), torch.as_tensor(want).to(torch.int64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = got != want
    assert not bool(bad.any()), "%s: %d of %d differ; first at %s: %d, expected %d" % (
        name, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), int(got[bad][0]), int(want[bad][0]))


def worst(report, name, ek, e32):
    """Keep the case with the largest ratio of a quantity (cc.check's record) and print it."""
    print("%-22s kernel %.3e  fp32 restatement %.3e  ratio %6.3f" % (name, ek, e32, ek / max(e32, cc.EPS32)))
    if name not in report or ek / max(e32, cc.EPS32) > report[name][0] / max(report[name][1], cc.EPS32):
        report[name] = (ek, e32)


def rel_gpu(a, ref):
    d = float((a.double() - ref).abs().max())
    scale = float(ref.abs().max())
    return d / scale if scale > 0 else d


# ---------------------------------------------------------------------------------------------------------------------------
# the symmetric kernel: chord, chord + keys, gram, mask + keys
# ---------------------------------------------------------------------------------------------------------------------------
def strided_input(t, ld, stride):
    """t [B, n, K] -> (view, base): a view with strides (stride, ld, 1) whose pad columns, gaps between shapes and guards hold NaN."""
    B, n, K = t.shape
    flat, base = guarded((B * stride,), BUFS_LEAD, BUFS_TAIL, NAN)
    view = flat.as_strided((B, n, K), (stride, ld, 1))
    view.copy_(t)
    return view, base


def sym_lds(n, K, batch):
    """(lda, ldc) pairs: dense and both padded for every batch count, the two mixed ones once."""
    return [(K, n), (K + 4, n + 4)] + ([(K, n + 4), (K + 4, n)] if batch == 3 else [])


@pytest.mark.parametrize("family", sorted(cc.FAMILIES))
@pytest.mark.parametrize("K", cc.SYM_K)
@pytest.mark.parametrize("n", cc.SYM_N)
def test_symmetric_kernel_in_guards_against_fp64(A, n, K, family):
    """prifit_chord_sym_f32 (with and without owner_key), prifit_gram_sym_f32 and prifit_chord_sym_mask with lda in {K, K + 4},
    ldc in {n, n + 4}, batch strides above n * ld (pad columns and gaps poisoned), batch 1, 3, 9, 11."""
    case = cc.sym_case(family, n, K)
    ref = {k: case[k].cuda() for k in ("chord64", "chord32", "gram64", "gram32")}
    report = {}
    for batch in cc.SYM_BATCH:
        e32 = {q: rel_gpu(ref[q + "32"][:batch], ref[q + "64"][:batch]) for q in ("chord", "gram")}
        C0 = keys0 = None
        masks0, thr0 = {}, {}
        for lda, ldc in sym_lds(n, K, batch):
            sA, sC = n * lda + 8, n * ldc + 12
            Ap, abase = strided_input(case["A"][:batch], lda, sA)

            def run(mode, rot=0):
                g = Bufs()
                keys = None
                if mode in ("chord_keys", "mask"):
                    keys = g.lout((batch, n))
                    keys.fill_(-1)                       # all bits set: the atomic-min identity
                if mode == "mask":
                    if rot not in thr0:
                        thr0[rot] = cc.thresholds(C0, rot)
                        masks0[rot] = cc.pack_mask(C0 < thr0[rot].view(-1, 1, 1))
                    thr = g.fin(thr0[rot])
                    out = g.iout((batch, n, n // 32))
                    A.call("prifit_chord_sym_mask", A.ptr(Ap), LL(lda), LL(sA), A.ptr(thr), A.ptr(out), n, K, batch, A.ptr(keys), A.cur_stream())
                    written(out)
                    obase = None
                else:
                    Cp, obase = padded_stream(batch, n, ldc, sC, SENTINEL)
                    out = Cp[..., :n]
                    if mode == "gram":
                        A.call("prifit_gram_sym_f32", A.ptr(Ap), LL(lda), LL(sA), A.ptr(Cp), LL(ldc), LL(sC), n, K, batch, A.cur_stream())
                    else:
                        A.call("prifit_chord_sym_f32", A.ptr(Ap), LL(lda), LL(sA), A.ptr(Cp), LL(ldc), LL(sC), n, K, batch, A.ptr(keys),
                               A.cur_stream())
                    finite(out)
                    assert_guards_intact(obase, out)
                g.intact()
                assert_guards_intact(abase, Ap, NAN)
                return out, keys

            C, _ = run("chord")
            assert torch.equal(C, C.transpose(1, 2)), "chord matrix not bitwise symmetric"
            if C0 is None:
                C0 = C.cpu().contiguous()
                keys0 = cc.owner_keys(C0)
                worst(report, "sym_chord", rel_gpu(C, ref["chord64"][:batch]), e32["chord"])
            else:
                assert torch.equal(C.cpu(), C0), "chord matrix depends on the leading dimensions"
            C2, keys = run("chord_keys")
            assert torch.equal(C2.cpu(), C0), "chord matrix differs with owner_key"
            exact("keys", keys, keys0)
            G, _ = run("gram")
            assert torch.equal(G, G.transpose(1, 2)), "gram matrix not bitwise symmetric"
            worst(report, "sym_gram", rel_gpu(G, ref["gram64"][:batch]), e32["gram"])
            for rot in range(3):
                mask, keys = run("mask", rot)
                exact("mask (rotation %d)" % rot, mask, masks0[rot])
                exact("keys of the mask mode", keys, keys0)
    cc.assert_bars(report)


# ---------------------------------------------------------------------------------------------------------------------------
# k-th smallest entry of every row
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", cc.KTH_C)
def test_kth_smallest_in_guards(A, C):
    """prifit_kth_smallest_rows against torch.topk on the same float32 matrix: every k of kth_ks(C), 1 / 5 / 37 rows, the six
    row families, 16-byte rows once aligned (float4 loads) and once starting 4 bytes later (scalar loads)."""
    for family in cc.KTH_FAMILIES:
        for rows in cc.KTH_ROWS:
            shared = None
            for k in cc.kth_ks(C):
                if shared is None or family == "kth_duplicated":
                    M = cc.kth_rows(family, rows, C, k)
                    g_in = Bufs()
                    views = []
                    for shift in ((0, 1) if C % 4 == 0 else (0,)):
                        buf = g_in.fin(torch.full((rows * C + 4,), NAN))
                        buf[shift:shift + rows * C] = M.reshape(-1).cuda()
                        views.append(buf[shift:])
                    shared = (M, g_in, views)
                M, g_in, views = shared
                want = cc.kth_expected(M, k)
                for v in views:
                    g = Bufs(lead=1024, tail=8192)
                    out = g.fout((rows,))
                    A.call("prifit_kth_smallest_rows", v.data_ptr(), LL(rows), C, k, A.ptr(out), A.cur_stream())
                    finite(out)
                    g.intact()
                    got = out.cpu()
                    assert bool((got == want).all()), "%s rows=%d C=%d k=%d offset %d bytes: %s, expected %s" % (
                        family, rows, C, k, v.data_ptr() % 16, got.tolist()[:5], want.tolist()[:5])
                if family == "kth_duplicated" or k == cc.kth_ks(C)[-1]:
                    g_in.intact()


# ---------------------------------------------------------------------------------------------------------------------------
# nms: the float routes, the pair form, the mask route
# ---------------------------------------------------------------------------------------------------------------------------
class NmsOut:
    """The outputs of one nms call in sentinel guards; counts | flags | used adjacent in one buffer or in three."""

    def __init__(self, g, B, N, adjacent):
        self.owner, self.labels = g.iout((B, N)), g.iout((B, N))
        self.ids, self.count = g.iout((B, CAP)), g.iout((B,))
        if adjacent:
            z = g.iout((2 * B * N + B * CAP,))
            self.counts, self.flags, self.used = z[:B * N].view(B, N), z[B * N:2 * B * N].view(B, N), z[2 * B * N:].view(B, CAP)
        else:
            self.counts, self.flags, self.used = g.iout((B, N)), g.iout((B, N)), g.iout((B, CAP))

    def nms(self, A, dist, Z, bw, B, N, D, keys):
        A.call("prifit_nms", A.ptr(dist), A.ptr(Z), A.ptr(bw), B, N, D, CAP, A.ptr(keys), A.ptr(self.owner), A.ptr(self.counts),
               A.ptr(self.flags), A.ptr(self.ids), A.ptr(self.count), A.ptr(self.labels), A.ptr(self.used), A.cur_stream())

    def nms_mask(self, A, mask, Z, B, N, D, keys):
        A.call("prifit_nms_mask", A.ptr(mask), A.ptr(Z), B, N, D, CAP, A.ptr(keys), A.ptr(self.owner), A.ptr(self.counts),
               A.ptr(self.flags), A.ptr(self.ids), A.ptr(self.count), A.ptr(self.labels), A.ptr(self.used), A.cur_stream())

    def nms_pair(self, A, dxc, dcc, Cen, X, bw, B, N, D):
        A.call("prifit_nms_pair", A.ptr(dxc), A.ptr(dcc), A.ptr(Cen), A.ptr(X), A.ptr(bw), B, N, D, CAP, A.ptr(self.owner),
               A.ptr(self.counts), A.ptr(self.flags), A.ptr(self.ids), A.ptr(self.count), A.ptr(self.labels), A.ptr(self.used),
               A.cur_stream())

    def check(self, g, refs, what):
        written(self.owner, self.labels, self.ids, self.count, self.counts, self.flags, self.used)
        g.intact()
        for z, r in enumerate(refs):
            for name in ("owner", "counts", "flags", "ids"):
                exact("%s %s of shape %d" % (what, name, z), getattr(self, name)[z], r[name])
            exact("%s count of shape %d" % (what, z), self.count[z], r["count"])
            keep = ~r["left"]
            exact("%s labels of shape %d" % (what, z), self.labels[z].cpu()[keep], r["labels"][keep])
            used = self.used[z].cpu().to(torch.int64)
            assert bool((used >= r["used_lo"]).all()) and bool((used <= r["used_hi"]).all()), "%s used of shape %d" % (what, z)


@pytest.mark.parametrize("D", cc.NMS_D)
@pytest.mark.parametrize("N", cc.NMS_N)
def test_nms_float_routes_in_guards(A, N, D):
    """prifit_nms on a float32 chord matrix: the owner pass from `dist` (owner_key NULL) and from keys (hand-made; at N = 512,
    D % 32 == 0 also dist and keys as the symmetric kernel left them), counts | flags | used adjacent and in three buffers."""
    case = cc.nms_case(N, D)
    B = 3
    g = Bufs()
    dist, Z, bw = g.fin(case["dist_cc"]), g.fin(case["X"]), g.fin(case["bw"])
    keys = g.lin(cc.owner_keys(case["dist_cc"]), 0)
    for use_keys in (False, True):
        for adjacent in (True, False):
            o = NmsOut(g, B, N, adjacent)
            o.nms(A, dist, Z, bw, B, N, D, keys if use_keys else None)
            o.check(g, case["refs"], "keys=%s adjacent=%s" % (use_keys, adjacent))
    if N % 128 == 0 and D % 32 == 0:
        Cg, kk = g.fout((B, N, N)), g.lout((B, N))
        kk.fill_(-1)
        A.call("prifit_chord_sym_f32", A.ptr(Z), LL(D), LL(N * D), A.ptr(Cg), LL(N), LL(N * N), N, D, B, A.ptr(kk), A.cur_stream())
        finite(Cg)
        g.intact()
        Cc = Cg.cpu()
        exact("keys of the symmetric kernel", kk, cc.owner_keys(Cc))
        refs = cc.nms_case_reference(case, Cc, Cc)
        for fam, r in zip(cc.NMS_FAMILY, refs):
            cc.assert_left_out(r["left"], fam != "own_centre", "kernel chord matrix, " + fam)
        o = NmsOut(g, B, N, True)
        o.nms(A, Cg, Z, bw, B, N, D, kk)
        o.check(g, refs, "symmetric kernel's dist and keys")


@pytest.mark.parametrize("D", cc.NMS_D)
@pytest.mark.parametrize("N", cc.NMS_N)
def test_nms_pair_in_guards(A, N, D):
    """prifit_nms_pair: centres that are not the points, the non-symmetric point x centre matrix for the owner pass."""
    case = cc.nms_case(N, D, True)
    B = 3
    g = Bufs()
    dxc, dcc, Cen, X, bw = (g.fin(case[k]) for k in ("dist_xc", "dist_cc", "Cen", "X", "bw"))
    if N > 1:
        assert not torch.equal(case["dist_xc"], case["dist_xc"].transpose(1, 2))
    for adjacent in (True, False):
        o = NmsOut(g, B, N, adjacent)
        o.nms_pair(A, dxc, dcc, Cen, X, bw, B, N, D)
        o.check(g, case["refs"], "pair adjacent=%s" % adjacent)


@pytest.mark.parametrize("D", cc.MASK_D)
@pytest.mark.parametrize("N", cc.MASK_N)
def test_nms_mask_in_guards(A, N, D):
    """prifit_nms_mask on the mask and keys of a guarded prifit_chord_sym_mask call, then on hand-made masks (an all-zero row
    and a row with bits only under zero counts, both of owning centres): the outputs of the float route's restatement on the
    chord matrix the same kernel writes in its chord mode."""
    case = cc.mask_case(N, D)
    B = 2
    g = Bufs()
    Z, bw = g.fin(case["X"]), g.fin(case["bw"])
    Cg = g.fout((B, N, N))
    A.call("prifit_chord_sym_f32", A.ptr(Z), LL(D), LL(N * D), A.ptr(Cg), LL(N), LL(N * N), N, D, B, None, A.cur_stream())
    finite(Cg)
    mask, keys = g.iout((B, N, N // 32)), g.lout((B, N))
    keys.fill_(-1)
    A.call("prifit_chord_sym_mask", A.ptr(Z), LL(D), LL(N * D), A.ptr(bw), A.ptr(mask), N, D, B, A.ptr(keys), A.cur_stream())
    written(mask)
    g.intact()
    Cc = Cg.cpu()
    near = Cc < case["bw"].view(B, 1, 1)
    exact("mask", mask, cc.pack_mask(near))
    keys_ref = cc.owner_keys(Cc)
    exact("keys", keys, keys_ref)
    refs = [cc.nms_reference(Cc[z], near[z], case["X"][z], case["X"][z]) for z in range(B)]
    for z, r in enumerate(refs):
        cc.assert_left_out(r["left"], z == 1, "kernel chord matrix, shape %d" % z)
    o = NmsOut(g, B, N, True)
    o.nms_mask(A, mask, Z, B, N, D, keys)
    o.check(g, refs, "kernel mask")

    hand = torch.stack([cc.handmade_mask(near[z], refs[z]["counts"]) for z in range(B)])
    refs = [cc.nms_reference(Cc[z], hand[z], case["X"][z], case["X"][z]) for z in range(B)]
    hmask, hkeys = g.iin(cc.pack_mask(hand), -1), g.lin(keys_ref, 0)
    o = NmsOut(g, B, N, False)
    o.nms_mask(A, hmask, Z, B, N, D, hkeys)
    o.check(g, refs, "hand-made mask")


# ---------------------------------------------------------------------------------------------------------------------------
# membership
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("KM", cc.MEM_KM)
@pytest.mark.parametrize("N", cc.MEM_N)
def test_membership_in_guards_against_fp64(A, N, KM):
    """prifit_membership_fwd / _bwd at count = 0, 1, a middle value and KM + 7, the exponent below -13, inside and above 75."""
    case = cc.membership_case(N, KM)
    ref = cc.membership_reference(case)
    B = cc.MEM_B
    g = Bufs()
    d, bw, gmax, gW = (g.fin(case[k]) for k in ("dots", "bw", "gmax", "gW"))
    count = g.iin(case["count"], 1)
    W = g.fout((B, N, KM))
    A.call("prifit_membership_fwd", A.ptr(d), A.ptr(bw), A.ptr(gmax), A.ptr(count), B, N, KM, A.ptr(W), A.cur_stream())
    finite(W)
    g.intact()
    Wc, live = W.cpu(), ref["live"]
    assert float(Wc[~live].abs().max() if bool((~live).any()) else 0) == 0.0, "dead slots"
    assert float(Wc[0].abs().max()) == 0.0, "count == 0"
    K = torch.minimum(case["count"], torch.tensor(KM)).view(B, 1).double()
    rows = Wc.double().sum(-1)
    assert bool(((rows - 1).abs()[1:] <= (K[1:] + 1) * 2.0 ** -24).all()), "rows of W do not sum to 1"
    report = {}
    cc.check("mem_W", Wc, ref["W64"], ref["W32"], report)

    Win = g.fin(Wc)
    gd = g.fout((B, N, KM))
    A.call("prifit_membership_bwd", A.ptr(gW), A.ptr(Win), A.ptr(d), A.ptr(bw), A.ptr(gmax), A.ptr(count), B, N, KM, A.ptr(gd), A.cur_stream())
    finite(gd)
    g.intact()
    gc, keep = gd.cpu(), ~ref["left"]
    zero = (~live | ref["clamped"]) & keep
    assert float(gc[zero].abs().max() if bool(zero.any()) else 0) == 0.0, "gdots on dead slots / clamped elements"
    cc.check("mem_gdots", gc * keep, ref["g64"] * keep, ref["g32"] * keep, report)
    cc.assert_bars(report)


# ---------------------------------------------------------------------------------------------------------------------------
# normalize(normalize(x)) and the mean-shift update
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", cc.ROW_D)
@pytest.mark.parametrize("rows", cc.ROW_ROWS)
def test_row_normalize2_in_guards_against_fp64(A, rows, D):
    """prifit_row_normalize2_fwd / _bwd; the bars per class of row (regular, zero, norm 1e-13 < eps, norm 1e-20): the gradient of
    a zero row is g / eps^2, 24 orders of magnitude above a regular row's."""
    case = cc.normalize2_case(rows, D)
    y64, gx64, _, _ = cc.normalize2_reference(case, F64)
    y32, gx32, _, _ = cc.normalize2_reference(case, F32)
    g = Bufs()
    x, gg = g.fin(case["x"]), g.fin(case["g"])
    y, gx = g.fout((rows, D)), g.fout((rows, D))
    A.call("prifit_row_normalize2_fwd", A.ptr(x), D, LL(rows), EPS, A.ptr(y), A.cur_stream())
    A.call("prifit_row_normalize2_bwd", A.ptr(x), A.ptr(gg), D, LL(rows), EPS, A.ptr(gx), A.cur_stream())
    finite(y, gx)
    g.intact()
    yc, gc = y.cpu(), gx.cpu()
    assert float(yc[case["cls"] == 1].abs().max() if bool((case["cls"] == 1).any()) else 0) == 0.0, "zero row"
    report = {}
    for c, name in enumerate(cc.ROW_CLASSES):
        m = case["cls"] == c
        if bool(m.any()):
            cc.check("n2_y:" + name, yc[m], y64[m], y32[m], report)
            cc.check("n2_gx:" + name, gc[m], gx64[m], gx32[m], report)
    cc.assert_bars(report)


def run_update_bwd(A, g, case, out, nrm, B, N, D, gap, report, tag):
    """prifit_meanshift_update_bwd on [B * N] rows with gO_batch_stride = N * D + gap.  out / nrm given (the forward kernel's):
    gO against float64 autograd; g_rowsum is identically zero there (cc.update_bwd_free) and only has to be finite.  out /
    nrm None: the case's free ones, gO and g_rowsum against the formula in float64."""
    free = out is None
    gi, O, rs = g.fin(case["g"]), g.fin(case["O"]), g.fin(case["rowsum"])
    outi, nrmi = g.fin(case["out_free"] if free else out), g.fin(case["nrm_free"] if free else nrm)
    gO = g.mout(B, N * D, N * D + gap)
    grs = g.fout((B * N,))
    A.call("prifit_meanshift_update_bwd", A.ptr(gi), A.ptr(outi), A.ptr(nrmi), A.ptr(O), A.ptr(rs), D, B, N, A.ptr(gO), LL(N * D + gap),
           A.ptr(grs), A.cur_stream())
    finite(gO, grs)
    g.intact()
    if free:
        (gO64, grs64), (gO32, grs32) = cc.update_bwd_free(case, F64), cc.update_bwd_free(case, F32)
        cc.check("upd_g_rowsum" + tag, grs.cpu().reshape(grs64.shape), grs64, grs32, report)
    else:
        gO64, gO32 = cc.update_reference(case, F64)[2], cc.update_reference(case, F32)[2]
    cc.check(("upd_gO_free" if free else "upd_gO") + tag, gO.cpu().reshape(gO64.shape), gO64, gO32, report)


@pytest.mark.parametrize("D", cc.ROW_D)
@pytest.mark.parametrize("rows", cc.ROW_ROWS)
def test_meanshift_update_in_guards_against_fp64(A, rows, D):
    """prifit_meanshift_update_fwd (out, nrm) and _bwd (gO from the forward's out; gO and g_rowsum from a free out) on one batch."""
    case = cc.update_free_inputs(cc.update_inputs((rows,), D, rows), rows)
    out64, nrm64, _, _ = cc.update_reference(case, F64)
    out32, nrm32, _, _ = cc.update_reference(case, F32)
    g = Bufs()
    O, rs, Z = g.fin(case["O"]), g.fin(case["rowsum"]), g.fin(case["Z"])
    out, nrm = g.fout((rows, D)), g.fout((rows,))
    A.call("prifit_meanshift_update_fwd", A.ptr(O), A.ptr(rs), A.ptr(Z), D, LL(rows), A.ptr(out), A.ptr(nrm), A.cur_stream())
    finite(out, nrm)
    g.intact()
    report = {}
    cc.check("upd_out", out.cpu(), out64, out32, report)
    cc.check("upd_nrm", nrm.cpu(), nrm64, nrm32, report)
    run_update_bwd(A, g, case, out.cpu(), nrm.cpu(), 1, rows, D, 0, report, "")
    run_update_bwd(A, g, case, None, None, 1, rows, D, 0, report, "")
    cc.assert_bars(report)


@pytest.mark.parametrize("D", cc.ROW_D)
def test_meanshift_update_bwd_batch_stride_gap(A, D):
    """The backward with B = 3, N = 43 and gO_batch_stride = N * D + 12: the gap between the shapes' gO stays untouched."""
    B, N = cc.UPD_B, cc.UPD_N
    case = cc.update_free_inputs(cc.update_inputs((B * N,), D, "gap"), "gap")
    g = Bufs()
    O, rs, Z = g.fin(case["O"]), g.fin(case["rowsum"]), g.fin(case["Z"])
    out, nrm = g.fout((B * N, D)), g.fout((B * N,))
    A.call("prifit_meanshift_update_fwd", A.ptr(O), A.ptr(rs), A.ptr(Z), D, LL(B * N), A.ptr(out), A.ptr(nrm), A.cur_stream())
    finite(out, nrm)
    report = {}
    run_update_bwd(A, g, case, out.cpu(), nrm.cpu(), B, N, D, cc.UPD_GAP, report, ":gap")
    run_update_bwd(A, g, case, None, None, B, N, D, cc.UPD_GAP, report, ":gap")
    cc.assert_bars(report)

"""The primitive-fitting kernels (csrc/fit.hip, the reductions of csrc/fit_glue.hip) at edge shapes, every float tensor a
kernel reads inside NaN guard bands, every tensor it writes inside sentinel guards (tests/guard_common.py; int tensors
through an int32 view of such a buffer), against the float64 restatements of tests/fit_common.py.

Each case asserts, in this order: outputs finite, guards intact, exact properties (dead slots, integer results, duplicated
targets), then the bars: for every continuous quantity max |kernel - fp64| / max |fp64| at most 4 x the same error of the
float32 restatement of the formula on the same inputs, computed on the CPU in the test (floor 4 x 2^-24).  The conditions
under which float32 and float64 take the same discrete decisions are asserted on every input family by
tests/test_fit_restatement.py.

Measured on an MI355X (the case with the largest ratio of each quantity: kernel error, float32 restatement's error, their
ratio with the restatement's error floored at 2^-24; the bar is a ratio of 4):

  quantity     kernel   fp32     ratio       quantity     kernel   fp32     ratio
  fit_r        6.1e-08  1.0e-07   0.61        nn_sum_d2    2.0e-07  2.2e-08   3.33
  fit_V        9.1e-07  2.3e-06   0.40        nn_g_r       1.4e-07  4.8e-08   2.29
  fit_c        7.9e-08  6.0e-08   1.32        nn_g_V       9.6e-07  8.6e-07   1.12
  fit_gW       1.3e-06  9.8e-07   1.37        nn_g_c       2.9e-07  2.1e-07   1.36
  fit_gW_iso   1.2e-05  5.7e-05   0.21        cmb_loss     2.6e-08  2.6e-08   0.44
  sdf_absmin   8.7e-08  8.3e-08   1.04        cmb_pd       1.4e-10  1.4e-10   0.00
  sdf_fval     8.7e-08  8.3e-08   1.04        cmb_ps       4.3e-08  4.3e-08   0.72
  sdf_sum_sq   1.4e-07  3.4e-08   2.36        cmb_g_d2     7.8e-08  9.4e-09   1.32
  sdf_g_r      1.3e-06  5.7e-07   2.31        cmb_g_sdf    5.3e-08  1.7e-08   0.88
  sdf_g_V      1.8e-07  6.9e-08   2.59        bw           4.8e-08  4.8e-08   0.80
  sdf_g_c      2.3e-07  1.1e-07   2.02        e2e_loss     6.0e-08  6.0e-08   1.00
  sdfm         1.7e-07  1.1e-07   1.53        e2e_dist_st  1.7e-07  4.3e-08   2.82
  sdfm_g_r     2.2e-07  9.2e-08   2.37        e2e_sdf_ts   3.7e-08  4.1e-08   0.61
  sdfm_g_V     2.2e-07  1.6e-07   1.36        e2e_g_r      1.3e-07  1.3e-07   1.00
  sdfm_g_c     2.3e-07  1.5e-07   1.56        e2e_g_V      9.1e-08  9.8e-08   0.92
  nn_idx       0.0e+00  1.6e-07   0.00        e2e_g_c      2.6e-07  2.6e-07   1.00

Before the backward sums of sample_nn_bwd_kernel and sdf_bwd_kernel were reduced across the wave (csrc/fit.hip,
slot_accumulate), these tests measured nn_g_r at 3.1e-07 .. 1.8e-06 against 4.8e-08 .. 1.4e-07 (ratios up to 19), nn_g_c up to 5.8
and the cuboid's sdf_g_r / sdf_g_c at 4.2 .. 8 at M = 1, 7, 8, 1030 and M = 255, 257, different from run to run: up to 600 float
atomics of one sign into one LDS cell in arrival order.
"""
import ctypes

import pytest
import torch

import fit_common as fc
from fit_common import F32, F64
from guard_common import SENTINEL, assert_guards_intact, guarded, guarded_like, poison_bits

pytestmark = pytest.mark.gpu

NAN = float("nan")
LL = ctypes.c_longlong
LEAD, TAIL = 4096, 65536


@pytest.fixture(scope="module")
def F(hiplib):
    assert torch.cuda.is_available()
    from prifit_amd import fit_ops
    return fit_ops


@pytest.fixture(scope="module")
def A(hiplib):
    from prifit_amd import _lib
    return _lib


class Bufs:
    """Guarded buffers of one case: fin / iin = inputs in NaN guards, fout / iout = outputs in SENTINEL guards."""

    def __init__(self):
        self.items = []

    def fin(self, t):
        v, base = guarded_like(t.detach().to(F32).cuda(), LEAD, TAIL, NAN)
        self.items.append((base, v, NAN))
        return v

    def iin(self, t):
        v, base = guarded(tuple(t.shape), LEAD, TAIL, NAN)
        v.view(torch.int32).copy_(t.to(torch.int32).cuda())
        self.items.append((base, v, NAN))
        return v.view(torch.int32)

    def fout(self, shape, zero=False):
        v, base = guarded(tuple(shape), LEAD, TAIL, SENTINEL)
        if zero:
            v.zero_()
        self.items.append((base, v, SENTINEL))
        return v

    def iout(self, shape):
        return self.fout(shape).view(torch.int32)

    def intact(self):
        torch.cuda.synchronize()
        for base, v, poison in self.items:
            assert_guards_intact(base, v, poison)


def finite(*ts):
    torch.cuda.synchronize()
    for t in ts:
        assert bool(torch.isfinite(t).all()), "non-finite output"


# ---------------------------------------------------------------------------------------------------------------------------
# fit, forward and backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in fc.FIT_CASES])
def test_ellipsoid_fit_in_guards_against_fp64(F, A, name):
    case = fc.fit_case(name)
    B, N, KM = case["W"].shape
    canonical = case["canonical"]
    g = Bufs()
    pts, W, rnd = g.fin(case["points"]), g.fin(case["W"]), g.fin(case["rnd"])
    count = g.iin(case["count"])
    sb, sk = (0, 0) if case["rnd"].dim() == 2 else (KM * 9, 9)
    r, V, c = g.fout((B, KM, 3)), g.fout((B, KM, 3, 3)), g.fout((B, KM, 3))
    valid = g.iout((B, KM))
    state = g.fout((B, KM, A.dll().prifit_fit_state_floats()), zero=True)
    A.call("prifit_ellipsoid_fit_fwd", A.ptr(pts), A.ptr(W), A.ptr(count), A.ptr(rnd), LL(sb), LL(sk), int(canonical), B, N, KM,
           A.ptr(r), A.ptr(V), A.ptr(c), A.ptr(valid), A.ptr(state), A.cur_stream())
    finite(r, V, c, state)
    g.intact()

    o64, _ = fc.fit_reference(case)
    if canonical:
        d = o64["det"][o64["valid"]]
        assert bool((d < 0).any()) and bool((d > 0).any())
    live, ok = o64["live"], o64["valid"]
    fc.assert_exact("valid", valid, ok)
    dead = ~live
    rc, Vc, cc = r.cpu(), V.cpu(), c.cpu()
    assert float(rc[dead].abs().max() if dead.any() else 0) == 0 and float(cc[dead].abs().max() if dead.any() else 0) == 0
    assert bool((Vc[dead] == torch.eye(3)).all())
    assert bool((torch.linalg.det(Vc.double())[live] > 0).all())
    col_sign = None
    if not canonical:       # the SVD leaves the column signs free: the reference is evaluated at the kernel's choice
        col_sign = torch.sign((Vc.double() * o64["V"]).sum(-2))
        col_sign[col_sign == 0] = 1.0
    o64, dW64 = fc.fit_reference(case, F64, col_sign)
    o32, dW32 = fc.fit_reference(case, F32, col_sign)
    mk = ok.unsqueeze(-1)
    report = {}
    fc.check("fit_r", rc * mk, o64["r"] * mk, o32["r"] * mk, report)
    fc.check("fit_V", Vc * mk.unsqueeze(-1), o64["V"] * mk.unsqueeze(-1), o32["V"] * mk.unsqueeze(-1), report)
    fc.check("fit_c", cc, o64["c"], o32["c"], report)

    g_r, g_V, g_c = g.fin(case["g_r"]), g.fin(case["g_V"]), g.fin(case["g_c"])
    gW = g.fout((B, N, KM))
    A.call("prifit_ellipsoid_fit_bwd", A.ptr(pts), A.ptr(W), A.ptr(count), A.ptr(valid), A.ptr(rnd), LL(sb), LL(sk), A.ptr(state),
           A.ptr(g_r), A.ptr(g_V), A.ptr(g_c), B, N, KM, A.ptr(gW), A.cur_stream())
    finite(gW)
    g.intact()
    gWc = gW.cpu()
    off = (~ok).unsqueeze(1).expand(B, N, KM)
    assert float(gWc[off].abs().max() if off.any() else 0) == 0.0       # dead and invalid slots, seeds non-zero there
    if case["family"] == "special":
        b, k = B - 1, fc.ISO_SLOT
        fc.check("fit_gW_iso", gWc[b, :, k], dW64[b, :, k], dW32[b, :, k], report)
        keep = torch.ones(B, 1, KM)
        keep[b, 0, k] = 0
        fc.check("fit_gW", gWc * keep, dW64 * keep, dW32 * keep, report)
    else:
        fc.check("fit_gW", gWc, dW64, dW32, report)

    # the autograd wrapper runs the same kernels: the same bits
    Wg = W.detach().requires_grad_(True)
    r2, V2, c2, valid2 = F.EllipsoidFitFn.apply(pts, Wg, count, rnd, bool(canonical))
    ((r2 * g_r).sum() + (V2 * g_V).sum() + (c2 * g_c).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(r2, r) and torch.equal(V2, V) and torch.equal(c2, c) and torch.equal(valid2, valid)
    assert torch.equal(Wg.grad, gW)
    g.intact()
    fc.assert_bars(report)


# ---------------------------------------------------------------------------------------------------------------------------
# SDF reductions and matrix
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ellipsoid", "cuboid"])
@pytest.mark.parametrize("M,KM", fc.SDF_CASES)
def test_sdf_reductions_and_matrix_in_guards_against_fp64(F, A, kind, M, KM):
    from prifit_amd.convex_loss import SdfMatrixFn
    case = fc.sdf_case(kind, M, KM)
    B = 2
    g = Bufs()
    T, r, V, c = (g.fin(case[k]) for k in ("targets", "r", "V", "c"))
    valid, gscale = g.iin(case["valid"]), g.fin(case["gscale"])
    arg, fval, ssum = g.iout((B, M)), g.fout((B, M)), g.fout((B,))
    A.call("prifit_%s_sdf_fwd" % kind, A.ptr(T), B, M, A.ptr(r), A.ptr(V), A.ptr(c), A.ptr(valid), KM, A.ptr(arg), A.ptr(fval),
           A.ptr(ssum), A.cur_stream())
    finite(fval, ssum)
    g.intact()
    red64, _, _ = fc.sdf_reference(case)
    argc = arg.cpu().long()
    cmp = red64["clear"].clone()
    cmp[0, :case["placed"]] = False
    assert bool((argc[cmp] == red64["arg"][cmp]).all()), "argmin differs on a clear point"
    vk = case["valid"].long()
    assert bool((torch.gather(vk, 1, argc.clamp(min=0))[argc >= 0] == 1).all()) and bool(((argc >= 0) == (red64["arg"] >= 0)).all())
    assert bool((argc[1] == -1).all()) and float(fval[1].abs().max()) == 0.0 and float(ssum[1]) == 0.0     # no valid slot
    use = torch.where(red64["clear"], red64["arg"], argc)
    red64, ga64, gb64 = fc.sdf_reference(case, F64, arg=use)
    red32, ga32, gb32 = fc.sdf_reference(case, F32, arg=use)
    report = {}
    clear = red64["clear"]
    fc.check("sdf_absmin", fval.cpu().abs(), red64["absmin"], red32["absmin"], report)
    fc.check("sdf_fval", fval.cpu() * clear, red64["fval"] * clear, red32["fval"] * clear, report)
    fc.check("sdf_sum_sq", ssum.cpu(), red64["sum_sq"], red32["sum_sq"], report)

    g_r, g_V, g_c = g.fout((B, KM, 3), zero=True), g.fout((B, KM, 3, 3), zero=True), g.fout((B, KM, 3), zero=True)
    A.call("prifit_%s_sdf_bwd" % kind, A.ptr(T), B, M, A.ptr(r), A.ptr(V), A.ptr(c), A.ptr(arg), A.ptr(gscale), KM, A.ptr(g_r),
           A.ptr(g_V), A.ptr(g_c), A.cur_stream())
    finite(g_r, g_V, g_c)
    g.intact()
    dead = case["valid"] == 0
    for nm, got, r64, r32 in (("g_r", g_r, ga64[0], ga32[0]), ("g_V", g_V, ga64[1], ga32[1]), ("g_c", g_c, ga64[2], ga32[2])):
        assert float(got.cpu()[dead].abs().max()) == 0.0
        fc.check("sdf_" + nm, got.cpu(), r64, r32, report)

    # the full matrix and its backward through the autograd wrapper; g has exact zeros and non-zero values in dead slots
    leaves = [t.detach().requires_grad_(True) for t in (r, V, c)]
    gm = g.fin(case["g"])
    mat = SdfMatrixFn.apply(T, *leaves, valid, kind == "cuboid")
    mat.backward(gm)
    finite(mat, *[l.grad for l in leaves])
    g.intact()
    assert float(mat.detach().cpu()[dead.unsqueeze(1).expand(B, M, KM)].abs().max()) == 0.0
    fc.check("sdfm", mat.detach().cpu(), red64["full"], red32["full"], report)
    for nm, l, r64, r32 in (("g_r", leaves[0], gb64[0], gb32[0]), ("g_V", leaves[1], gb64[1], gb32[1]), ("g_c", leaves[2], gb64[2], gb32[2])):
        assert float(l.grad.cpu()[dead].abs().max()) == 0.0
        fc.check("sdfm_" + nm, l.grad.cpu(), r64, r32, report)
    fc.assert_bars(report)


# ---------------------------------------------------------------------------------------------------------------------------
# budget, sampling, search
# ---------------------------------------------------------------------------------------------------------------------------
def run_search(A, g, case, cap):
    """Budget + search through the C ABI with guarded buffers -> dict of device tensors."""
    kind = case["kind"]
    pre = "prifit_cuboid_sample" if kind == "cuboid" else "prifit_sample"
    B, KM = case["valid"].shape
    M = case["targets"].shape[1]
    r, V, c, T = (g.fin(case[k]) for k in ("r", "V", "c", "targets"))
    valid = g.iin(case["valid"])
    n, off = g.iout((B, KM)), g.iout((B, KM + 1))
    A.call(pre + "_budget", A.ptr(r), A.ptr(valid), B, KM, cap, A.ptr(n), A.ptr(off), A.cur_stream())
    nn_idx, ssum = g.iout((B, cap)), g.fout((B,))
    ws = g.fout((A.query("prifit_sample_nn_workspace_floats", B, cap),))
    A.call(pre + "_nn_fwd", A.ptr(r), A.ptr(V), A.ptr(c), A.ptr(n), A.ptr(off), B, KM, A.ptr(T), M, cap, A.ptr(nn_idx), A.ptr(ssum),
           A.ptr(ws), A.cur_stream())
    finite(ssum)
    g.intact()
    return dict(pre=pre, r=r, V=V, c=c, T=T, valid=valid, n=n, off=off, nn_idx=nn_idx, sum_d2=ssum)


def check_search(case, k, ref64, ref32, report):
    B, KM = case["valid"].shape
    cap = case["cap"]
    fc.assert_exact("n", k["n"], ref64["n"])
    fc.assert_exact("off", k["off"], ref64["off"])
    idx = k["nn_idx"].cpu()
    for b in range(B):
        assert bool((idx[b, int(ref64["total"][b]):] == poison_bits(SENTINEL)).all()), "nn_idx written behind the shape's total"
    S = ref64["idx"].shape[1]
    hits = fc.check_neighbours("nn_idx", idx[:, :S].clamp(min=-1), ref64, ref32["d2"], case["targets"], case["pairs"], report)
    assert hits >= len(case["pairs"]) * int((ref64["total"] > 0).sum())
    fc.check("nn_sum_d2", k["sum_d2"].cpu(), ref64["sum_d2"], ref32["sum_d2"], report)


@pytest.mark.parametrize("kind", ["ellipsoid", "cuboid"])
@pytest.mark.parametrize("M", fc.NN_M)
def test_budget_sampling_search_in_guards_against_fp64(F, A, kind, M):
    """cap = 600 through the C ABI (the clip n = cap - off and n = 0 behind it), live slots {0}, {0, 3, 31}, none, all 32."""
    KM, cap = 32, 600
    case = fc.nn_case(kind, M, KM, cap)
    B = case["valid"].shape[0]
    g = Bufs()
    k = run_search(A, g, case, cap)
    ref64 = fc.nn_reference(case)
    assert int(ref64["n"][1, 0]) == 100 and ref64["total"].tolist() == [600, 600, 0, 600]
    S = ref64["idx"].shape[1]
    kidx = k["nn_idx"].cpu().long()[:, :S]
    ref64 = fc.nn_reference(case, F64, idx=kidx)
    ref32 = fc.nn_reference(case, F32, idx=kidx)
    report = {}
    check_search(case, k, ref64, ref32, report)
    # the budget without the clip
    full = F.sample_cap(KM)
    n2, off2 = g.iout((B, KM)), g.iout((B, KM + 1))
    A.call(k["pre"] + "_budget", A.ptr(k["r"]), A.ptr(k["valid"]), B, KM, full, A.ptr(n2), A.ptr(off2), A.cur_stream())
    g.intact()
    nf, offf, _ = fc.budget64(kind, case["r"], case["valid"], full)
    fc.assert_exact("n (full cap)", n2, nf)
    fc.assert_exact("off (full cap)", off2, offf)

    gscale = g.fin(case["gscale"])
    g_r, g_V, g_c = g.fout((B, KM, 3), zero=True), g.fout((B, KM, 3, 3), zero=True), g.fout((B, KM, 3), zero=True)
    A.call(k["pre"] + "_nn_bwd", A.ptr(k["r"]), A.ptr(k["V"]), A.ptr(k["c"]), A.ptr(k["n"]), A.ptr(k["off"]), B, KM, A.ptr(k["T"]), M,
           cap, A.ptr(k["nn_idx"]), A.ptr(gscale), A.ptr(g_r), A.ptr(g_V), A.ptr(g_c), A.cur_stream())
    finite(g_r, g_V, g_c)
    g.intact()
    unused = torch.from_numpy((ref64["n"].numpy() == 0))
    for i, (nm, got) in enumerate((("g_r", g_r), ("g_V", g_V), ("g_c", g_c))):
        assert float(got.cpu()[unused].abs().max()) == 0.0
        fc.check("nn_" + nm, got.cpu(), ref64["grads"][i], ref32["grads"][i], report)
    fc.assert_bars(report)


@pytest.mark.parametrize("kind", ["ellipsoid", "cuboid"])
def test_sample_nn_loss_wrapper_with_forty_of_64_slots(F, A, kind):
    """SampleNNLossFn at KM = 64 (sample_cap(64) slots), 40 live, and a shape without a valid slot: forward and autograd."""
    KM, M = 64, 1000
    cap = F.sample_cap(KM)
    assert cap == 16640
    case = fc.nn_case(kind, M, KM, cap)
    g = Bufs()
    r, V, c = (g.fin(case[k]).detach().requires_grad_(True) for k in ("r", "V", "c"))
    T, valid, gscale = g.fin(case["targets"]), g.iin(case["valid"]), case["gscale"].cuda()
    s, total = F.SampleNNLossFn.apply(r, V, c, valid, T, kind == "cuboid")
    nn_idx = s.grad_fn.saved_tensors[6]
    (s * gscale).sum().backward()
    finite(s, r.grad, V.grad, c.grad)
    g.intact()
    ref64 = fc.nn_reference(case, device="cuda")
    S = ref64["idx"].shape[1]
    kidx = nn_idx.long()[:, :S]
    ref64 = fc.nn_reference(case, F64, idx=kidx, device="cuda")
    ref32 = fc.nn_reference(case, F32, idx=kidx.cpu())
    fc.assert_exact("total", total, ref64["total"])
    report = {}
    hits = fc.check_neighbours("nn_idx", kidx.cpu(), ref64, ref32["d2"], case["targets"], case["pairs"], report)
    assert hits >= len(case["pairs"])
    fc.check("nn_sum_d2", s.detach().cpu(), ref64["sum_d2"], ref32["sum_d2"], report)
    dead = case["valid"] == 0
    for i, (nm, leaf) in enumerate((("g_r", r), ("g_V", V), ("g_c", c))):
        assert float(leaf.grad.cpu()[dead].abs().max()) == 0.0
        fc.check("nn_" + nm, leaf.grad.cpu(), ref64["grads"][i], ref32["grads"][i], report)
    fc.assert_bars(report)


# ---------------------------------------------------------------------------------------------------------------------------
# small reductions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,empty", [(1, False), (3, False), (65, False), (3, True)])
def test_chamfer_combine_in_guards(F, B, empty):
    KM, M = 32, 257
    gen = torch.Generator().manual_seed(B)
    valid = (torch.rand(B, KM, generator=gen) < 0.1).int()
    valid[0, 5] = 1
    if B > 1:
        valid[1] = 0                          # a shape without a valid slot
    if empty:
        valid[:] = 0
    total = torch.randint(1, 12000, (B,), generator=gen).int()
    total[-1] = 0                             # a shape with no sample
    d2, sdf = torch.rand(B, generator=gen) * 3, torch.rand(B, generator=gen) * 5
    g = Bufs()
    d2g, sdfg = g.fin(d2).detach().requires_grad_(True), g.fin(sdf).detach().requires_grad_(True)
    loss, part = F.ChamferCombineFn.apply(d2g, g.iin(total), sdfg, g.iin(valid), M)
    (loss * 1.7).backward()
    finite(loss, part, d2g.grad, sdfg.grad)
    g.intact()
    report = {}
    refs = {}
    for dt in (F64, F32):
        a, b = d2.to(dt).requires_grad_(True), sdf.to(dt).requires_grad_(True)
        l, pd, ps = fc.combine64(a, total, b, valid, M, dt)
        if l.requires_grad:
            (l * 1.7).backward()
        z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
        refs[dt] = (l.detach().reshape(1), pd.detach(), ps.detach(), z(a), z(b))
    got = (loss.detach().reshape(1).cpu(), part[0].cpu(), part[1].cpu(), d2g.grad.cpu(), sdfg.grad.cpu())
    for nm, x, r64, r32 in zip(("cmb_loss", "cmb_pd", "cmb_ps", "cmb_g_d2", "cmb_g_sdf"), got, refs[F64], refs[F32]):
        fc.check(nm, x, r64, r32, report)
    if empty:
        assert float(loss.detach()) == 0.0 and float(d2g.grad.abs().max()) == 0.0 and float(sdfg.grad.abs().max()) == 0.0
    none = (valid != 0).sum(1) == 0
    assert float(d2g.grad.cpu()[none].abs().max() if none.any() else 0) == 0.0
    fc.assert_bars(report)


def test_membership_gmax_in_guards(A):
    """N * KM / 4 = 34 float4 per shape: not a multiple of the 16 parts, and the last parts are empty."""
    B, N, KM = 3, 17, 8
    gen = torch.Generator().manual_seed(4)
    dots = torch.randn(B, N, KM, generator=gen)
    count = torch.tensor([5, 0, 8], dtype=torch.int32)
    dots[0, :, 5:] = 100.0                    # dead columns hold the largest values
    bw = torch.tensor([0.3, 0.5, 0.7])
    g = Bufs()
    out = g.fout((B,))
    ws = g.fout((A.query("prifit_membership_gmax_workspace", B),))
    A.call("prifit_membership_gmax", A.ptr(g.fin(dots)), A.ptr(g.fin(bw)), A.ptr(g.iin(count)), B, N, KM, A.ptr(out), A.ptr(ws),
           A.cur_stream())
    g.intact()
    live = torch.arange(KM).view(1, 1, KM) < count.view(B, 1, 1)
    want = dots.masked_fill(~live, float("-inf")).amax(dim=(1, 2)) / (bw * bw)
    assert float(want[1]) == float("-inf")
    assert torch.equal(out.cpu(), want)       # bit-equal to the fp32 maximum divided by bw squared


@pytest.mark.parametrize("with_nuniq", [False, True])
def test_cluster_verdict_in_guards(A, with_nuniq):
    B, cap = 9, 64
    gen = torch.Generator().manual_seed(6)
    for count9, expect_bad in ((70, 1), (20, 0)):
        used = (torch.rand(B, cap, generator=gen) < 0.2).int()
        count = used.sum(1).int()
        count[8] = count9                     # more centres kept than `cap`: nuniq = count
        g = Bufs()
        nuniq = g.iout((B,)) if with_nuniq else None
        bad = g.iout((1,))
        A.call("prifit_cluster_verdict", A.ptr(g.iin(count)), A.ptr(g.iin(used)), B, cap, 25, 32, A.ptr(nuniq), A.ptr(bad),
               A.cur_stream())
        g.intact()
        nu, b = fc.verdict(count, used, cap, 25, 32)
        assert b == expect_bad and int(bad[0]) == b
        if with_nuniq:
            assert nuniq.cpu().tolist() == nu


@pytest.mark.parametrize("N", [1, 255, 1000])
def test_bandwidth_from_kth_in_guards(A, N):
    B = 3
    kth = torch.rand(B, N, generator=torch.Generator().manual_seed(N)) * 0.5
    kth[:, ::3] = 1e-9                         # below the 1e-6 clamp
    kth[1, 0] = -1e-7                          # a chord distance rounded below zero
    g = Bufs()
    out = g.fout((B,))
    A.call("prifit_bandwidth_from_kth", A.ptr(g.fin(kth)), B, N, A.ptr(out), A.cur_stream())
    finite(out)
    g.intact()
    report = {}
    fc.check("bw", out.cpu(), fc.bandwidth64(kth), fc.bandwidth64(kth, F32), report)
    fc.assert_bars(report)


# ---------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ellipsoid", "cuboid"])
def test_analytic_chamfer_distance_against_the_fp64_chain(F, A, kind):
    from prifit_amd.convex_loss import analytic_chamfer_distance
    B, KM, M = 3, 32, 500
    cap = F.sample_cap(KM)
    gen = torch.Generator().manual_seed(11 if kind == "ellipsoid" else 12)
    for _ in range(256):
        r, V, c, valid = fc.prims(B, KM, [(0, 3, 31), (), tuple(range(8))], gen)
        try:
            fc.budget_conditions(fc.budget64(kind, r.to(F32), valid, cap)[2], valid)
            break
        except AssertionError:
            continue
    T = (1.6 * torch.rand(B, M, 3, generator=gen, dtype=F64) - 0.8).to(F32)
    r, V, c = r.to(F32), V.to(F32), c.to(F32)
    g = Bufs()
    case = dict(kind=kind, r=r, V=V, c=c, valid=valid, targets=T, cap=cap, pairs=[])
    k = run_search(A, g, case, cap)                       # the kernels' own discrete choices, for the reference's gradient
    arg, fval, ssum = g.iout((B, M)), g.fout((B, M)), g.fout((B,))
    A.call("prifit_%s_sdf_fwd" % kind, A.ptr(k["T"]), B, M, A.ptr(k["r"]), A.ptr(k["V"]), A.ptr(k["c"]), A.ptr(k["valid"]), KM,
           A.ptr(arg), A.ptr(fval), A.ptr(ssum), A.cur_stream())
    g.intact()
    leaves = [k[n].detach().requires_grad_(True) for n in ("r", "V", "c")]
    loss, (dist_st, sdf_ts) = analytic_chamfer_distance(*leaves, k["valid"], k["T"], cuboid=kind == "cuboid")
    loss.backward()
    finite(loss, dist_st, sdf_ts, *[l.grad for l in leaves])
    g.intact()
    a, i = arg.cpu().long(), k["nn_idx"].cpu().long().clamp(min=-1)
    l64, pd64, ps64, g64, aux = fc.chamfer_chain(kind, r, V, c, valid, T, cap, F64, arg=a, idx=i)
    l32, pd32, ps32, g32, _ = fc.chamfer_chain(kind, r, V, c, valid, T, cap, F32, arg=a, idx=i)
    cmp = aux["clear"]
    assert bool((a[cmp] == aux["arg"][cmp]).all()) and int((~cmp).sum()) <= 0.01 * B * M
    report = {}
    fc.check("e2e_loss", loss.detach().reshape(1).cpu(), l64.reshape(1), l32.reshape(1), report)
    fc.check("e2e_dist_st", dist_st.cpu(), pd64, pd32, report)
    fc.check("e2e_sdf_ts", sdf_ts.cpu(), ps64, ps32, report)
    dead = valid == 0
    for nm, l, r64, r32 in zip(("e2e_g_r", "e2e_g_V", "e2e_g_c"), leaves, g64, g32):
        assert float(l.grad.cpu()[dead].abs().max()) == 0.0
        fc.check(nm, l.grad.cpu(), r64, r32, report)
    fc.assert_bars(report)

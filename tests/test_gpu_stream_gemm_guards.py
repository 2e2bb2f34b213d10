"""The weights-stationary streaming products of csrc/gemm_stream.hip and the fused dA + dW kernel of csrc/gemm_stream_bwd.hip
through the C ABI at the smallest shapes at which each path exists, every tensor a kernel reads inside NaN guard bands (pad
columns of matrices with ld > width included, a different ld per operand), every tensor it writes inside sentinel guards
(tests/guard_common.py), against the float64 restatements of tests/stream_common.py (pinned to torch autograd by
tests/test_stream_restatement.py).

Guards: GUARD_ROWS = 64 rows (one tile: the farthest row an access of a tail tile can be read to reach lies 63 rows behind the
last one) times LD_MAX, the widest leading dimension any case uses, in front of every tensor, and twice that behind it.  No
access that the code can be read to make leaves an allocation: a stray one shows as a changed guard word or a non-finite
result.

Each case asserts, in this order: outputs finite; guards intact bit for bit (pad columns of C / G / Gp included); exact
properties (cand = first occurrence and the stored C bit for bit; the slabs of workgroups beyond the grid are zero; the slabs
of the workgroups that do not own the tail tile are the bits of the t = 0 run, and the tail's rows enter the owner's slab as
the float64 sum of the rows below M alone; bit-equal reruns of prifit_gemm_stream_bwd_f32 and of the TN family;
prifit_gemm_stream_f32 == the tiled prifit_gemm_f32 on the same padded operands); then the bars: error against float64 at
most 4 x the error of the float32 restatement on the same inputs (floored at 2^-24), products and slabs normalised element by
element by the float64 sum of |terms|.  The slabs are compared with the sums of the STORED product (col_stats) or of the stored
gradient under the masks (red_slab), workgroup by workgroup.

Measured on an MI355X (per quantity the case with the largest ratio: kernel error, float32 restatement's error, their ratio
with the restatement's error floored at 2^-24, the case -- (layout,) M or P, N or Cout, K or Cin(, pool_K); the bar is a
ratio of 4; _C / _G / _Gp / _dW and tn* are products, _stats / _slab the per-workgroup slabs):

  quantity           kernel   fp32     ratio   case
  f32_C              3.2e-07  2.9e-07   1.09   (1, 32805, 96, 96)
  f32_stats          2.8e-07  2.2e-07   1.26   (0, 32805, 64, 64)
  pool_C             3.3e-07  3.1e-07   1.05   (32768, 64, 96)
  pool_stats         2.6e-07  2.1e-07   1.24   (32768, 96, 128)
  gather_C           3.0e-07  3.0e-07   0.98   (32768, 128, 64)
  gather_stats       2.4e-07  2.5e-07   0.96   (32768, 128, 64)
  dgrad_G            3.9e-07  3.5e-07   1.12   (32805, 96, 128)
  dgrad_slab         3.3e-07  2.3e-07   1.46   (32805, 96, 128)
  dgrad_bn_G         4.2e-07  3.7e-07   1.14   (32805, 128, 64)
  dgrad_bn_slab      5.1e-07  2.5e-07   2.08   (32805, 128, 64)
  dgrad_pool_G       5.0e-07  4.5e-07   1.09   (32832, 128, 64)
  dgrad_pool_slab    4.0e-07  1.6e-07   2.52   (32832, 96, 64)
  tn                 3.8e-08  1.5e-07   0.25   (32824, 64, 128, 0)
  tn_bn              1.0e-07  3.2e-07   0.32   (32824, 128, 96, 0)
  tn_pool            1.7e-07  5.5e-07   0.30   (32768, 96, 96, 64)
  bwd_Gp             1.9e-07  1.5e-07   1.30   (100, 96, 64, 0)
  bwd_dW             1.8e-06  1.8e-06   1.00   (64, 64, 64, 0)
  bwd_slab           6.6e-07  2.4e-07   2.72   (168, 128, 128, 0)
  bwd_pool_Gp        2.1e-07  2.1e-07   1.00   (64, 128, 96, 64)
  bwd_pool_dW        2.1e-06  2.0e-06   1.05   (64, 128, 128, 64)
  bwd_pool_slab      2.3e-07  1.2e-07   1.84   (192, 128, 96, 64)
  bwd_gather_Gp      2.0e-07  1.7e-07   1.20   (128, 64, 64, 0)
  bwd_gather_dW      3.7e-07  5.0e-07   0.73   (128, 64, 64, 0)
  bwd_gather_slab    5.1e-07  1.7e-07   3.00   (128, 64, 64, 0)

Defects these tests found:
- prifit_gemm_stream_tn_f32 / _tn_bn_f32 / _tn_pool_f32 did not repeat their bits: stream_tn_reduce_kernel added up to 32
  slices of the slab range to `out` with float atomics, in arrival order (all nine test_stream_tn_family cases failed "the
  rerun gives other bits").  Now every slice leaves its sum in the place of its first slab and stream_tn_add_kernel adds the
  slices in order: bit-equal reruns in every case.  VGPR / AGPR / scratch (0) / occupancy of all 52 gemm_stream_kernel and 12
  gemm_stream_bwd_kernel instantiations are unchanged (neither kernel was touched); the step time of bench.py against the
  parent commit is in DESIGN.md beside the streaming kernels' tests.
- The column statistics of a TM = 2 wave (N = 96, 128) were one chain of 32 additions per lane and tile, which rounds a run of
  equal rows (rows 20 .. 109 of every case: a padded ball) 32 times the same way.  Before: f32_stats 1.0e-06 against 2.5e-07
  (ratio 4.10) at NT (32805, 128, 96) and 1.1e-06 against 2.8e-07 (4.05) at NN (32805, 96, 96), the other N >= 96 cases 1.8 ..
  3.9, pool_stats 3.88, gather_stats 2.97; N = 64 (a chain of 16) <= 1.3.  Now the 16 rows of each accumulator tile are summed
  on their own: the ratios above, with unchanged register counts.  The last bits of every BatchNorm statistic of the streaming
  forward change with it, so the digests of tests/test_gpu_atlas.py::test_model_without_reconstruct_matches_recorded_bits
  were recorded again (the library before the change reproduces the old ones).
Nothing else was found.  In particular NO guard word changed in any ragged case, before any kernel was touched: the stores of
gemm_stream_kernel / gemm_stream_bwd_kernel to rows beyond M or P, whose row inside the tile sits in the scalar offset of the
buffer instruction, are dropped, and the pad columns of C / G / Gp stay untouched.  On gfx950 the bounds check of a raw buffer
covers lane offset + scalar offset; the notes in meanshift_fused.hip (Tile64T::load<EXACT>) and ADVICE.md that say otherwise
are not borne out by this chip.  No kernel was changed for it.  (A variant with the row in the lane offset in the tail tile
only was compiled: it raised the VGPR count of every gemm_stream_kernel instantiation, by 2 .. 63, cost occupancy in five and
spilled in six.)  Every cand arg is the first occurrence, every slab beyond the grid is zero, prifit_gemm_stream_bwd_f32
repeats its bits and prifit_gemm_stream_f32 gives the bits of the tiled kernel in all 18 width / layout cases.

What these tests cannot see, and what was not run.  NaN guards show a stray read only if the value read reaches a result: the
Yprev loads of rows beyond M (RED) would be discarded (`vs` is 0 there) -- that they do not happen follows from the stores,
which go through the same addressing and are visible.  The mutation check (the tail mask `row < g.M` read as `row <= g.M`)
was not run; what stands in for it is the per-workgroup comparison of the tail tile's slab with the float64 sums of the stored
rows below M alone, which a row M entering the sums (its value is the bias) would miss by a whole term.
"""
import functools

import pytest
import torch

import bn_common as bc
import stream_common as sc
from bn_common import F32, F64
from guard_common import Bufs

pytestmark = pytest.mark.gpu

GUARD_ROWS = sc.TILE                    # rows behind the last one that a tail tile's access can be read to reach (63) + 1
LD_MAX = max(sc.WIDTHS) + 4 * 6         # ld_of(width, i) below, i <= 5
LEAD = GUARD_ROWS * LD_MAX
TAIL = 2 * GUARD_ROWS * LD_MAX
M_MAX = sc.STREAM_MIN + max(sc.T_SWEEP)


def ld_of(width, i):
    """A different leading dimension (a multiple of 4 floats) for the i-th operand of a call"""
    assert i <= 5
    return width + 4 * (i + 1)


@pytest.fixture(scope="module")
def A(hiplib):
    assert torch.cuda.is_available()
    from prifit_amd import _lib
    return _lib


def bufs():
    return Bufs(LEAD, TAIL)


def finite(*ts):
    torch.cuda.synchronize()
    for t in ts:
        assert bool(torch.isfinite(t).all()), "non-finite output"


def vin(g, v):
    return None if v is None else g.fin(v)


@functools.lru_cache(maxsize=4)
def fwd_inputs(N, K, layout):
    return sc.fwd_case(M_MAX, N, K, layout)


@functools.lru_cache(maxsize=4)
def bwd_inputs(Cout, Cin, pool_K, P=M_MAX):
    return sc.bwd_case(P, Cout, Cin, pool_K)


def check_slabs(rep, name, tag, slab, terms64, terms32, grid, nslab):
    """Slabs beyond the launched grid are zero; the others against the per-workgroup sums of the terms"""
    slab = slab.cpu()
    assert slab.shape[0] == nslab and not bool(slab[grid:].any()), "a slab beyond the grid is not zero"
    r64 = sc.wg_slabs(terms64[0], terms64[1], grid, nslab)
    r32 = sc.wg_slabs(terms32[0], terms32[1], grid, nslab, F32)
    ab = sc.wg_slabs(terms64[0].abs(), terms64[1].abs(), grid, nslab)
    rep.red(name, tag, slab, r64, r32, ab)


def stats_check(rep, name, tag, slab, Cst, M, K, heavy):
    c64, c32 = Cst.cpu().to(F64), Cst.cpu()
    check_slabs(rep, name, tag, slab, sc.stats_terms(c64), sc.stats_terms(c32), sc.launched_grid(M, K, heavy), sc.stream_grid(M, K))


def red_check(rep, name, tag, slab, Gst, c, M, grid, nslab):
    tabs = [c["p_" + k] for k in ("scale", "shift", "mean", "invstd")]
    Gc = Gst.cpu()
    check_slabs(rep, name, tag, slab, sc.red_terms(Gc, c["Yp"][:M], *tabs), sc.red_terms(Gc, c["Yp"][:M], *tabs, dtype=F32), grid, nslab)


# ---------------------------------------------------------------------------------------------------------------------------
# forward: prifit_gemm_stream_f32 (NT / NN), _pool_f32, _gather_f32
# ---------------------------------------------------------------------------------------------------------------------------
def run_fwd(A, c, M, entry="f32", tiled=False):
    """-> (g, C, slab, cand) of one launch on the first M rows of the case"""
    N, K, layout = c["N"], c["K"], c.get("layout", 0)
    g = bufs()
    Bd = g.fin(c["B"], ld_of(c["B"].shape[1], 1))
    scl, shf, bias = vin(g, c["scale"]), vin(g, c["shift"]), vin(g, c["bias"])
    Cd = g.mout(M, N, ld_of(N, 2))
    nslab = A.dll().prifit_gemm_stream_slabs(M, K)
    assert nslab == sc.stream_grid(M, K)
    slab = g.fout((nslab, 2, N))
    cand = None
    if entry == "gather":
        ix = g.iin(c["idx"], c["n_points"] - 1)     # guards: the point no list names, whose row of U is NaN on the device
        U, Vc = g.fin(c["U"]), g.fin(c["Vc"])
        U[:, c["n_points"] - 1] = float("nan")
        A.call("prifit_gemm_stream_gather_f32", M, N, A.ptr(ix), A.ptr(U), A.ptr(Vc), c["n_points"], c["n_centres"], c["rpc"],
               A.ptr(Bd), Bd.stride(0), A.ptr(Cd), Cd.stride(0), A.ptr(scl), A.ptr(shf), A.ptr(bias), A.ptr(slab), A.cur_stream())
        return g, Cd, slab, cand
    Ad = g.fin(c["A"][:M], ld_of(K, 0))
    if tiled:
        A.call("prifit_gemm_f32", layout, M, N, K, A.ptr(Ad), Ad.stride(0), 0, A.ptr(Bd), Bd.stride(0), 0, A.ptr(Cd), Cd.stride(0),
               0, 1, 1, A.ptr(scl), A.ptr(shf), None, None, A.ptr(bias), 0, None, 0, None, None, 0, 0, None, None, 0, A.cur_stream())
    elif entry == "pool":
        cand = g.fout((M // 32, 4, N))
        A.call("prifit_gemm_stream_pool_f32", M, N, K, A.ptr(Ad), Ad.stride(0), A.ptr(Bd), Bd.stride(0), A.ptr(Cd), Cd.stride(0),
               A.ptr(scl), A.ptr(shf), A.ptr(bias), A.ptr(slab), A.ptr(cand), A.cur_stream())
    else:
        A.call("prifit_gemm_stream_f32", layout, M, N, K, A.ptr(Ad), Ad.stride(0), A.ptr(Bd), Bd.stride(0), A.ptr(Cd), Cd.stride(0),
               A.ptr(scl), A.ptr(shf), A.ptr(bias), A.ptr(slab), A.cur_stream())
    return g, Cd, slab, cand


def check_fwd(A, rep, name, tag, c, M, entry="f32", a_rows=None):
    g, Cd, slab, cand = run_fwd(A, c, M, entry)
    finite(Cd, slab)
    g.intact()
    rows = c["A"][:M] if a_rows is None else a_rows
    r64, ab = sc.gemm_fwd(rows, c["B"], c.get("layout", 0), c["scale"], c["shift"], c["bias"])
    r32, _ = sc.gemm_fwd(rows, c["B"], c.get("layout", 0), c["scale"], c["shift"], c["bias"], F32)
    rep.red(name + "_C", tag, Cd, r64, r32, ab)
    stats_check(rep, name + "_stats", tag, slab, Cd, M, c["K"], entry == "pool")
    return g, Cd, slab, cand


@pytest.mark.parametrize("layout", [0, 1], ids=["NT", "NN"])
@pytest.mark.parametrize("N,K", [(N, K) for N in sc.WIDTHS for K in sc.WIDTHS])
def test_stream_f32_all_widths_ragged_in_guards_against_fp64(A, layout, N, K):
    """All nine (N, K) pairs in both layouts at M = 32768 + 37: every WN / TM / KG configuration, with and without the prologue"""
    assert A.dll().prifit_gemm_stream_supported(layout, sc.STREAM_MIN, N, K) == 1
    rep = bc.Report()
    M = sc.STREAM_MIN + sc.T_RAGGED
    c = dict(fwd_inputs(N, K, layout))
    if layout == 1 or (N + K) % 64 == 0:         # without the prologue: the NN products (dA) and a third of the NT ones
        c["scale"] = c["shift"] = None
    if layout == 1:
        c["bias"] = None
    _, Cd, _, _ = check_fwd(A, rep, "f32", (layout, M, N, K), c, M)
    g2, C2, _, _ = run_fwd(A, c, M, tiled=True)
    finite(C2)
    g2.intact()
    assert torch.equal(Cd, C2), "not the bits of the tiled kernel"      # the same k-ordered fp32 MFMA chain
    rep.assert_bars()


@functools.lru_cache(maxsize=2)
def _sweep_base(A, N, K):
    """The t = 0 run of a sweep pair: its slabs, for the comparison with the ragged runs"""
    _, Cd, slab, _ = run_fwd(A, fwd_inputs(N, K, 0), sc.STREAM_MIN)
    torch.cuda.synchronize()
    return Cd.cpu().clone(), slab.cpu().clone()


@pytest.mark.parametrize("t", sc.T_SWEEP)
@pytest.mark.parametrize("N,K", sc.SWEEP_PAIRS)
def test_stream_f32_tail_sweep_in_guards_against_fp64(A, N, K, t):
    rep = bc.Report()
    M = sc.STREAM_MIN + t
    c = fwd_inputs(N, K, 0)
    _, Cd, slab, _ = check_fwd(A, rep, "f32", (0, M, N, K), c, M)
    C0, slab0 = _sweep_base(A, N, K)
    # the rows of the t = 0 problem: the same bits, and the slabs of every workgroup that does not own the tail tile too
    assert torch.equal(Cd.cpu()[:sc.STREAM_MIN], C0)
    grid = sc.launched_grid(M, K, False)
    owner = (sc.STREAM_MIN // sc.TILE) % grid
    keep = torch.ones(slab0.shape[0], dtype=torch.bool)
    if t and owner < keep.numel():
        keep[owner] = False
    # (the owner's slab is compared by check_fwd with the float64 sums of the stored rows below M alone: rows >= M add nothing)
    assert torch.equal(slab.cpu()[:slab0.shape[0]][keep], slab0[keep])
    rep.assert_bars()


@pytest.mark.parametrize("M", [sc.STREAM_MIN, sc.STREAM_MIN + 32])
@pytest.mark.parametrize("N,K", [(128, 64), (64, 96), (96, 128)])
def test_stream_pool_f32_candidates_in_guards_against_fp64(A, N, K, M):
    rep = bc.Report()
    c = fwd_inputs(N, K, 0)
    _, Cd, _, cand = check_fwd(A, rep, "pool", (M, N, K), c, M, "pool")
    finite(cand[:, 0], cand[:, 2])
    vmax, amax, vmin, amin = sc.cand_of(Cd.cpu().contiguous())
    cd = cand.cpu()
    assert torch.equal(cd[:, 0], vmax) and torch.equal(cd[:, 2], vmin), "cand is not the stored C"
    assert torch.equal(cd[:, 1].contiguous().view(torch.int32).long(), amax), "argmax is not the first occurrence"
    assert torch.equal(cd[:, 3].contiguous().view(torch.int32).long(), amin), "argmin is not the first occurrence"
    blk = Cd.cpu()[32:64]
    assert bool((blk == blk[0]).all()) and not bool(amax[1].any()) and not bool(amin[1].any())     # a block of equal rows: row 0 wins
    rep.assert_bars()


def test_stream_gather_f32_in_guards_against_fp64(A):
    rep = bc.Report()
    c = sc.gather_fwd_case(500, 256, 64, 2, 128)
    M = c["M"]
    assert M == sc.STREAM_MIN and int((c["idx"] == -1).sum()) == 1 and int((c["idx"] == c["n_points"]).sum()) == 1
    y1 = sc.gather_rows(c["U"], c["Vc"], c["idx"], c["n_points"], c["n_centres"], c["rpc"])
    check_fwd(A, rep, "gather", (M, c["N"], 64), c, M, "gather", a_rows=y1)
    rep.assert_bars()


# ---------------------------------------------------------------------------------------------------------------------------
# dA: prifit_gemm_stream_dgrad_f32, _dgrad_bn_f32, _dgrad_pool_f32
# ---------------------------------------------------------------------------------------------------------------------------
def run_dgrad(A, c, M, form):
    """G = dY W with the (m1, m2) slabs of the layer below; K = Cout of the case, N = Cin"""
    K, N = c["Cout"], c["Cin"]
    g = bufs()
    W = g.fin(c["W"], ld_of(N, 1))
    Gd = g.mout(M, N, ld_of(N, 2))
    Yp = g.fin(c["Yp"][:M], ld_of(N, 3))
    tabs = [g.fin(c["p_" + k]) for k in ("scale", "shift", "mean", "invstd")]
    nslab = A.dll().prifit_gemm_stream_slabs(M, K)
    slab = g.fout((nslab, 2, N))
    t0, t1, t2, t3 = (A.ptr(x) for x in tabs)
    if form == "plain":
        dY = g.fin(c["G"][:M], ld_of(K, 0))
        A.call("prifit_gemm_stream_dgrad_f32", M, N, K, A.ptr(dY), dY.stride(0), A.ptr(W), W.stride(0), A.ptr(Gd), Gd.stride(0),
               A.ptr(Yp), Yp.stride(0), t0, t1, t2, t3, A.ptr(slab), A.cur_stream())
    elif form == "bn":
        Gin, Y = g.fin(c["G"][:M], ld_of(K, 0)), g.fin(c["Y"][:M], ld_of(K, 0))
        c0, c1, c2, c3, c4 = (A.ptr(g.fin(c[k])) for k in ("scale", "shift", "a", "b", "d"))
        A.call("prifit_gemm_stream_dgrad_bn_f32", M, N, K, A.ptr(Gin), A.ptr(Y), Y.stride(0), A.ptr(W), W.stride(0), A.ptr(Gd),
               Gd.stride(0), c0, c1, c2, c3, c4, A.ptr(Yp), Yp.stride(0), t0, t1, t2, t3, A.ptr(slab), A.cur_stream())
    else:
        pk = c["pool_K"]
        Y = g.fin(c["Y"][:M], ld_of(K, 0))
        arg, T = g.iin(c["arg"][:M // pk], 0), g.fin(c["T"][:M // pk])
        bdw, cb = g.fin(c["bias_dW"]), g.fin(c["b"])
        A.call("prifit_gemm_stream_dgrad_pool_f32", M, N, K, A.ptr(Y), Y.stride(0), A.ptr(W), W.stride(0), A.ptr(Gd), Gd.stride(0),
               A.ptr(bdw), A.ptr(arg), A.ptr(T), A.ptr(cb), pk, A.ptr(Yp), Yp.stride(0), t0, t1, t2, t3, A.ptr(slab), A.cur_stream())
    return g, Gd, slab


def dgrad_refs(c, M, form, dtype):
    if form == "plain":
        dY = c["G"][:M].to(dtype)
        return sc.dgrad(dY, dY.abs(), c["W"], None, dtype)
    if form == "bn":
        return sc.dgrad(*sc.bwd_dy(c, dtype, M), c["W"], None, dtype)
    return sc.dgrad(*sc.bwd_dy(c, dtype, M, with_d=False), c["W"], c["bias_dW"], dtype)


def check_dgrad(A, rep, c, M, form):
    K, N = c["Cout"], c["Cin"]
    tag = (M, N, K)
    g, Gd, slab = run_dgrad(A, c, M, form)
    finite(Gd, slab)
    g.intact()
    r64, ab = dgrad_refs(c, M, form, F64)
    r32, _ = dgrad_refs(c, M, form, F32)
    name = "dgrad" + ("" if form == "plain" else "_" + form)
    rep.red(name + "_G", tag, Gd, r64, r32, ab)
    red_check(rep, name + "_slab", tag, slab, Gd, c, M, sc.launched_grid(M, K, True), sc.stream_grid(M, K))
    return Gd, slab


@pytest.mark.parametrize("N,K", [(N, K) for N in sc.WIDTHS for K in sc.WIDTHS])
def test_stream_dgrad_all_widths_ragged_in_guards_against_fp64(A, N, K):
    rep = bc.Report()
    M = sc.STREAM_MIN + sc.T_RAGGED
    c = bwd_inputs(K, N, 0)
    check_dgrad(A, rep, c, M, "plain")
    check_dgrad(A, rep, c, M, "bn")
    if K != 96:         # (a pooled layer of 96 channels does not exist); whole pooling groups: one more tile than the floor
        cp = dict(bwd_inputs(K, N, 64, sc.STREAM_MIN + 64))
        cp["bias_dW"] = (cp["d"].to(F64) @ cp["W"].to(F64)).to(F32)
        check_dgrad(A, rep, cp, sc.STREAM_MIN + 64, "pool")
    rep.assert_bars()


@pytest.mark.parametrize("t", sc.T_SWEEP)
@pytest.mark.parametrize("N,K", sc.SWEEP_PAIRS)
def test_stream_dgrad_tail_sweep_in_guards_against_fp64(A, N, K, t):
    rep = bc.Report()
    M = sc.STREAM_MIN + t
    c = bwd_inputs(K, N, 0)
    Gd, slab = check_dgrad(A, rep, c, M, "plain")
    _, G0, slab0 = run_dgrad(A, c, sc.STREAM_MIN, "plain")
    assert torch.equal(Gd[:sc.STREAM_MIN], G0)
    grid = sc.launched_grid(M, K, True)
    keep = torch.ones(slab0.shape[0], dtype=torch.bool)
    owner = (sc.STREAM_MIN // sc.TILE) % grid
    if t and owner < keep.numel():
        keep[owner] = False                                   # (its slab is compared with float64 by check_dgrad)
    assert torch.equal(slab.cpu()[:slab0.shape[0]][keep], slab0.cpu()[keep])
    rep.assert_bars()


# ---------------------------------------------------------------------------------------------------------------------------
# dW: prifit_gemm_stream_tn_f32, _tn_bn_f32, _tn_pool_f32
# ---------------------------------------------------------------------------------------------------------------------------
def run_tn(A, c, P, form, out0):
    Mo, No = c["Cout"], c["Cin"]
    g = bufs()
    Ap = g.fin(c["Yp"][:P], ld_of(No, 1))
    out = g.mout(Mo, No, ld_of(No, 2))
    out.copy_(out0)
    ws = g.fout((A.dll().prifit_gemm_stream_tn_workspace(Mo, No, P),))
    ps, pt = g.fin(c["p_scale"]), g.fin(c["p_shift"])
    if form == "plain":
        G = g.fin(c["G"][:P], ld_of(Mo, 0))
        A.call("prifit_gemm_stream_tn_f32", Mo, No, P, A.ptr(G), G.stride(0), A.ptr(Ap), Ap.stride(0), A.ptr(out), out.stride(0),
               A.ptr(ps), A.ptr(pt), A.ptr(ws), A.cur_stream())
    elif form == "bn":
        G, Y = g.fin(c["G"][:P], ld_of(Mo, 0)), g.fin(c["Y"][:P], ld_of(Mo, 0))
        c0, c1, c2, c3, c4 = (A.ptr(g.fin(c[k])) for k in ("scale", "shift", "a", "b", "d"))
        A.call("prifit_gemm_stream_tn_bn_f32", Mo, No, P, A.ptr(G), A.ptr(Y), Y.stride(0), A.ptr(Ap), Ap.stride(0), A.ptr(out),
               out.stride(0), A.ptr(ps), A.ptr(pt), c0, c1, c2, c3, c4, A.ptr(ws), A.cur_stream())
    else:
        pk = c["pool_K"]
        Y = g.fin(c["Y"][:P], ld_of(Mo, 0))
        arg, T = g.iin(c["arg"][:P // pk], 0), g.fin(c["T"][:P // pk])
        cb, cd = g.fin(c["b"]), g.fin(c["d"])
        A.call("prifit_gemm_stream_tn_pool_f32", Mo, No, P, A.ptr(Y), Y.stride(0), A.ptr(Ap), Ap.stride(0), A.ptr(out), out.stride(0),
               A.ptr(ps), A.ptr(pt), A.ptr(arg), A.ptr(T), A.ptr(cb), A.ptr(cd), pk, A.ptr(ws), A.cur_stream())
    return g, out


def tn_refs(c, P, form, out0, dtype):
    if form == "plain":
        dY = c["G"][:P].to(dtype)
        dY, mag = dY, dY.abs()
    else:
        dY, mag = sc.bwd_dy(c, dtype, P)
    return sc.wgrad(dY, mag, c["Yp"][:P], c["p_scale"], c["p_shift"], out0, dtype)


@pytest.mark.parametrize("P", [sc.STREAM_MIN, sc.STREAM_MIN + 8, sc.STREAM_MIN + 56])
@pytest.mark.parametrize("Mo,No", [(128, 96), (96, 96), (64, 128)])
def test_stream_tn_family_in_guards_against_fp64(A, Mo, No, P):
    assert A.dll().prifit_gemm_stream_tn_supported(Mo, No, P) == 1
    rep = bc.Report()
    out0 = (0.5 * torch.randn(Mo, No, generator=bc.gen_of(bc.seed_of(24, Mo, No)))).to(F32)     # `out +=` on a non-zero out
    forms = [("plain", 0), ("bn", 0), ("pool", 8)] + ([("pool", 64)] if P % 64 == 0 else [])
    for form, pk in forms:
        c = bwd_inputs(Mo, No, 0) if form != "pool" else sc.bwd_case(P, Mo, No, pk)
        tag = (P, Mo, No, pk)
        g, out = run_tn(A, c, P, form, out0)
        finite(out)
        g.intact()
        g2, out2 = run_tn(A, c, P, form, out0)
        g2.intact()
        assert torch.equal(out, out2), "the rerun gives other bits"
        r64, ab = tn_refs(c, P, form, out0, F64)
        r32, _ = tn_refs(c, P, form, out0, F32)
        rep.red("tn" + ("" if form == "plain" else "_" + form), tag, out, r64, r32, ab)
    rep.assert_bars()


# ---------------------------------------------------------------------------------------------------------------------------
# the fused dA + dW kernel: prifit_gemm_stream_bwd_f32 (middle layer, pooled layer), _bwd_gather_f32
# ---------------------------------------------------------------------------------------------------------------------------
def run_bwd(A, c, P):
    Cout, Cin, pk = c["Cout"], c["Cin"], c["pool_K"]
    gather = "idx" in c
    assert A.dll().prifit_gemm_stream_bwd_supported(P, Cout, Cin, pk) == 1
    g = bufs()
    Y = g.fin(c["Y"][:P])                        # G, Y: contiguous by contract
    G = None if pk else g.fin(c["G"][:P])
    c0, c1, c2 = (None if pk else A.ptr(g.fin(c[k])) for k in ("scale", "shift", "a"))
    c3, c4 = A.ptr(g.fin(c["b"])), A.ptr(g.fin(c["d"]))
    arg = g.iin(c["arg"][:P // pk], 0) if pk else None
    T = g.fin(c["T"][:P // pk]) if pk else None
    W = g.fin(c["W"], ld_of(Cin, 0))
    t0, t1, t2, t3 = (A.ptr(g.fin(c["p_" + k])) for k in ("scale", "shift", "mean", "invstd"))
    Gp = g.mout(P, Cin, ld_of(Cin, 2))
    nslab = A.dll().prifit_gemm_stream_bwd_slabs(P, Cout, Cin)
    slab, dW = g.fout((nslab, 2, Cin)), g.mout(Cout, Cin, ld_of(Cin, 3))
    ws = g.fout((A.dll().prifit_gemm_stream_bwd_workspace(P, Cout, Cin),))
    if gather:
        ix = g.iin(c["idx"], c["n_points"] - 1)
        U, Vc = g.fin(c["U"]), g.fin(c["Vc"])
        U[:, c["n_points"] - 1] = float("nan")
        A.call("prifit_gemm_stream_bwd_gather_f32", P, Cout, A.ptr(G), A.ptr(Y), c0, c1, c2, c3, c4, A.ptr(W), W.stride(0),
               A.ptr(ix), A.ptr(U), A.ptr(Vc), c["n_points"], c["n_centres"], c["rpc"], t0, t1, t2, t3, A.ptr(Gp), Gp.stride(0),
               A.ptr(slab), A.ptr(dW), dW.stride(0), A.ptr(ws), A.cur_stream())
    else:
        Yp = g.fin(c["Yp"][:P], ld_of(Cin, 1))
        A.call("prifit_gemm_stream_bwd_f32", P, Cout, Cin, A.ptr(G), A.ptr(Y), c0, c1, c2, c3, c4, A.ptr(arg), A.ptr(T), pk,
               A.ptr(W), W.stride(0), A.ptr(Yp), Yp.stride(0), t0, t1, t2, t3, A.ptr(Gp), Gp.stride(0), A.ptr(slab), A.ptr(dW),
               dW.stride(0), A.ptr(ws), A.cur_stream())
    return g, Gp, slab, dW, nslab


def check_bwd(A, rep, c, P, name="bwd"):
    tag = (P, c["Cout"], c["Cin"], c["pool_K"])
    g, Gp, slab, dW, nslab = run_bwd(A, c, P)
    finite(Gp, slab, dW)
    g.intact()
    g2, Gp2, slab2, dW2, _ = run_bwd(A, c, P)
    g2.intact()
    assert torch.equal(Gp, Gp2) and torch.equal(slab, slab2) and torch.equal(dW, dW2), "the rerun gives other bits"
    Yp64 = sc.gather_rows(c["U"], c["Vc"], c["idx"], c["n_points"], c["n_centres"], c["rpc"]) if "idx" in c else c["Yp"][:P]
    ref = {}
    for dt in (F64, F32):
        dY, mag = sc.bwd_dy(c, dt, P)
        ref[dt] = sc.fused_bwd(dY, mag, c["W"], Yp64.to(dt), c["p_scale"], c["p_shift"], dt)
    rep.red(name + "_Gp", tag, Gp, ref[F64][0][0], ref[F32][0][0], ref[F64][0][1])
    rep.red(name + "_dW", tag, dW, ref[F64][1][0], ref[F32][1][0], ref[F64][1][1])
    red_check(rep, name + "_slab", tag, slab, Gp, dict(c, Yp=Yp64.to(F32)), P, nslab, nslab)


@pytest.mark.parametrize("Cout,Cin", sc.BWD_PAIRS)
def test_stream_bwd_all_pairs_ragged_in_guards_against_fp64(A, Cout, Cin):
    rep = bc.Report()
    c = bwd_inputs(Cout, Cin, 0, 168)
    for P in (100, 168):
        check_bwd(A, rep, c, P)
    rep.assert_bars()


@pytest.mark.parametrize("P", [64, 65, 68, 69, 100, 127, 168])
def test_stream_bwd_tail_sweep_in_guards_against_fp64(A, P):
    rep = bc.Report()
    check_bwd(A, rep, bwd_inputs(128, 96, 0, 168), P)
    check_bwd(A, rep, bwd_inputs(64, 64, 0, 168), P)
    rep.assert_bars()


def test_stream_bwd_persistent_loop_with_a_tail_in_guards_against_fp64(A):
    """More tiles than workgroups: every workgroup walks two tiles, the first eight rows of a 1025th tile go to workgroup 0"""
    rep = bc.Report()
    slabs = A.dll().prifit_gemm_stream_bwd_slabs(1 << 22, 64, 64)
    P = 64 * (2 * slabs) + 8
    assert A.dll().prifit_gemm_stream_bwd_slabs(P, 64, 64) == slabs
    check_bwd(A, rep, sc.bwd_case(P, 64, 64, 0), P)
    rep.assert_bars()


@pytest.mark.parametrize("P", [64, 192])
@pytest.mark.parametrize("Cout,Cin", [(128, 128), (128, 96), (64, 64)])
def test_stream_bwd_pooled_in_guards_against_fp64(A, Cout, Cin, P):
    rep = bc.Report()
    check_bwd(A, rep, bwd_inputs(Cout, Cin, 64, 192), P, "bwd_pool")
    rep.assert_bars()


@pytest.mark.parametrize("Cout", [128, 96, 64])
def test_stream_bwd_gather_in_guards_against_fp64(A, Cout):
    rep = bc.Report()
    c = sc.bwd_case(128, Cout, 64, 0, gather=(40, 2, 64, 1))
    assert int((c["idx"] == -1).sum()) == 1 and int((c["idx"] == 40).sum()) == 1
    check_bwd(A, rep, c, 128, "bwd_gather")
    rep.assert_bars()

"""The point-index kernels (csrc/pointops.hip: FPS, ball query, 3-NN, square distance, group gather / scatter, interpolation,
fp_rows, the column packers) and the set-abstraction front end (csrc/sa_group.hip: prifit_sa_group_linear_fwd,
prifit_sa_point_tables, the three prifit_sa_first_layer_dw* forms) through the C ABI at edge shapes, every float tensor a kernel
reads inside NaN guard bands (pad columns included), every index input inside an in-range poison whose row is NaN, every tensor
it writes inside sentinel guards (tests/guard_common.py), against the float64 restatements of tests/sa_front_common.py (pinned
to the oracle and to torch by tests/test_sa_front_restatement.py, which also proves that every case list below reaches the path
it is named for).

Each case asserts, in this order: the return code, outputs finite (index outputs: every entry in [0, N]), guards intact, the
exact properties, then the bars: error against float64 at most 4 x the error of the float32 restatement on the same inputs
(floored at 2^-24), element-wise outputs normalised by max |fp64|, reduced outputs element by element by the float64 sum of
|terms|.  Integer results and moves are exact: on lattice clouds against float64 (see sa_front_common), off the lattice against
prifit_oracle.c_*.  A NaN read from a guard counts as in-ball (`!(d > r2)`) and shows as a wrong index; the row kernels form
0 * x for masked rows, so a stray NaN survives into the output.

Path -> case that reaches it:
  fps_kernel<1 / 2 / 4 / 8 / 16>, ragged last slot    test_fps N = 255 / 257 / 513 / 1025 / 2049, 4095; full: 256, 4096
  ball_query_kernel<R = 1..4, int32 / int64>          test_ball_query, every N: the four radius sets of BALL_RK, idx64 0 and 1
  r2max not last / ring wraps with an unfilled radius BALL_RK[1], [2] / BALL_RK[4] at N = 2047 .. 4097 (all N pass the ring)
  one / two / three LDS tiles, N around the tile      test_ball_query N = 2047, 2048 / 2049 / 4097
  K > N, empty ball, exactly K members, K = 1024      N = 1, 63 with K up to 128 / centre (9, 9, 9) / test_ball_query_exact_k_and_limits
  front end phase 1 (same lists)                      test_ball_query N <= 2048, every case
  three_nn_kernel, > 1 tile, ragged last block        test_three_nn S = 2049, N = 255, 257
  group_gather vector / row8 / scalar                 test_group_gather GATHER_VECTOR / GATHER_ROW8 / GATHER_SCALAR
  fp_rows, rows narrower than 4 / kp % 4 != 0 / S == 1  test_fp_rows D2 = 1, 3 / pad 3, 5 / S = 1 (idx == NULL)
  sa_group_kernel<.., 4>, partial row block           test_front_end_direct / _gather: K in {1, 7, 65} at every width
  sa_group_kernel<.., 4>, whole row blocks, sum K 320 the "full" cases
  sa_group_kernel<.., 8>, three idle waves            test_front_end_eight_waves (B = 8, S = 1021)
  B > 8: blocks with b >= B return                    the B = 9 cases (16 shapes dealt, 7 return)
  gather mode with Y / slab / bias NULL               test_front_end_gather
  sa_point_tables, threads past a radius' row count   test_point_tables, widths (4, 128), (12, 64, 16)
  dw kernels: one / several / surplus blocks          test_first_layer_dw, nblocks 1 / 3 / ceil(P / 256) + 2

Measured on an MI355X (per quantity the case with the largest ratio: kernel error, float32 restatement's error, their ratio
with the restatement's error floored at 2^-24, the case -- the tuples are those of the case tables of sa_front_common with B, and
for the front end (C, K) of the radius, appended; dw*: (P, C, D, feat_first, nblocks); the bar is a ratio of 4; the chain_* rows
are the chained test):

  quantity            kernel   fp32     ratio   case
  nn_weight           7.5e-08  7.5e-08   1.00   ('lattice', 255, 3, 3)
  scatter_dfeat       9.5e-08  8.6e-08   1.10   (64, 8, 76, True, 3)
  interp_dp2          1.7e-07  7.7e-08   2.17   (64, 8, 76, True, 1)
  interp_out          7.4e-08  7.4e-08   1.00   (24, 37, 8, 0, 1)
  fp_rows             7.0e-08  7.0e-08   1.00   (1, 0, 0, 1, 1, 9)
  direct_rows         7.3e-08  6.2e-08   1.18   (6, 0, 3, 1, 65, 64, 1)
  direct_slab_s       7.1e-07  3.4e-07   2.10   (3, 1, 3, 5, 65, 128, 128)
  direct_slab_q       8.3e-07  5.5e-07   1.50   (3, 1, 3, 5, 65, 128, 128)
  gather_rows         6.7e-08  6.7e-08   1.00   ('none', 3, 5, 65, 16, 1)
  gather_slab_s       9.0e-07  3.8e-07   2.38   ('none', 3, 5, 65, 128, 128)
  gather_slab_q       9.7e-07  4.3e-07   2.25   ('none', 3, 5, 65, 128, 128)
  wave8_rows          6.9e-08  1.1e-07   0.61   (8, 1021, 64, 16, 4)
  wave8_slab_s        1.8e-07  1.6e-07   1.11   (8, 1021, 64, 16, 4)
  wave8_slab_q        2.1e-07  2.1e-07   1.00   (8, 1021, 64, 16, 4)
  tables_U            1.5e-07  6.7e-08   2.20   (9, 0, 16, True, 1)
  tables_Vc           6.5e-08  6.5e-08   1.00   (0, 0, 128, False, 3)
  tables_ident        1.6e-07  8.2e-08   1.92   (6, 0, 4, False, 1)
  dw                  6.4e-08  6.4e-08   1.00   (1, 32, 3, 0, 1)
  dw_bn               3.2e-07  2.4e-07   1.33   (1, 64, 6, 1, 1)
  dw_bn_gather        3.2e-07  2.4e-07   1.33   (1, 64, 6, 1, 1)
  chain_U             6.3e-08  7.7e-08   0.81   chain
  chain_Vc            2.8e-08  2.8e-08   0.46   chain
  chain_rows          9.7e-08  1.2e-07   0.79   ('chain', 64, 7)
  chain_slab_s        1.2e-07  1.3e-07   0.90   ('chain', 64, 7)
  chain_slab_q        1.5e-07  1.9e-07   0.79   ('chain', 64, 7)
  chain_dW            1.3e-07  2.0e-07   0.62   chain

Largest difference between two runs of the outputs that add with float atomics in arrival order, in the unit of the bars (the
weight-gradient partials are asserted to repeat their bits; every index result is exact):

  quantity            largest   case
  scatter_dfeat       1.5e-07   (64, 4, 72, False, 3)
  interp_dp2          2.8e-07   (64, 8, 76, True, 3)

Defects these tests found: none.  No guard word was touched and no output was non-finite; every index list, FPS pick, 3-NN
index and distance, gathered row and packed column is exact; every rejection the cases name is in place (a rejected call leaves
every output word at the sentinel); the largest ratio against the float32 restatement is 2.38 (the slabs of a 128-wide radius with
K = 128, where one lane adds 64 rows in one chain before the shuffles), inside the bar of 4, so the summation order of
sa_group_kernel and of the weight-gradient kernel (ratio at most 1.33, at P = 1; 0.07 .. 0.34 at P = 1000) stays as it is.

What these tests cannot see: a stray read whose value is discarded.  The clamped loads of dead slots read an in-range row
and drop it: the rows beyond K of a partial row block (entry K - 1 of the list), rows whose index is outside the cloud (row 0 of
the cloud, of U, of feat), the idle waves' centre (centre S - 1), the weight gradient's rows beyond its range (its first row).
"""
import ctypes

import numpy as np
import pytest
import torch

import bn_common as bc
import prifit_oracle as orc
import sa_front_common as sc
from bn_common import F32, F64
from guard_common import SENTINEL, Bufs, poison_bits
from prifit_amd import synth

pytestmark = pytest.mark.gpu

EINVAL = -1
I32 = torch.int32


@pytest.fixture(scope="module")
def A(hiplib):
    assert torch.cuda.is_available()
    from prifit_amd import _lib
    return _lib


def rc_of(A, name, *args):
    return getattr(A.dll(), name)(*args)


def ok_rc(A, name, *args):
    assert rc_of(A, name, *args) == 0, name


def finite(*ts):
    torch.cuda.synchronize()
    for t in ts:
        assert bool(torch.isfinite(t).all()), "non-finite output"


def in_range(N, *ts):
    torch.cuda.synchronize()
    for t in ts:
        assert bool(((t >= 0) & (t <= N)).all()), "index output outside [0, N]"


def same(a, b):
    return torch.equal(a.cpu(), b.cpu())


def untouched(*ts):
    torch.cuda.synchronize()
    for t in ts:
        w = t.view(I32) if t.dtype != torch.int64 else t.contiguous().view(I32)
        assert bool((w == poison_bits(SENTINEL)).all()), "a rejected call wrote an output"


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def ints(v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def floats(v):
    return (ctypes.c_float * len(v))(*[float(x) for x in v])


def _t(a):
    return torch.from_numpy(np.asarray(a))


def rerun_diff(a, b, absum):
    return bc.red_err(a, b.to("cpu", F64), absum)


# ---------------------------------------------------------------------------------------------------------------------------
# farthest point sampling
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", sc.FPS_N)
def test_fps_in_guards_exactly(A, N):
    for kind in ("lattice", "same", "cube"):
        for B in sc.fps_Bs(N):
            start = torch.tensor([0, N - 1, N // 2][-B:])
            xyz = _t(synth.cloud("cube", B, N, 40 + N)) if kind == "cube" else sc.fps_cloud(kind, B, N)
            for npoint in sorted({1, N}):
                if kind == "cube":
                    want = orc.c_farthest_point_sample(xyz, npoint, start)
                elif kind == "same":                       # every later pick is index 0
                    want = torch.cat([start.view(B, 1), torch.zeros(B, npoint - 1, dtype=torch.int64)], 1)
                else:
                    want = sc.fps(xyz, npoint, start)
                for give in (False, True):
                    g = Bufs()
                    xd, sd, out = g.fin(xyz), g.lin(start.view(B, 1), N // 2), g.lout((B, npoint))
                    new = g.fout((B, npoint, 3)) if give else None
                    ok_rc(A, "prifit_fps", A.ptr(xd), B, N, npoint, A.ptr(sd), A.ptr(out), A.ptr(new), A.cur_stream())
                    in_range(N - 1, out)
                    if give:
                        finite(new)
                    g.intact()
                    assert same(out, want), (kind, N, B, npoint)
                    if give:
                        assert same(new, orc.gather_rows(xyz, want))


def test_fps_rejects_unsupported_arguments(A):
    g = Bufs()
    x, s, out, new = g.fin(torch.zeros(1, 8, 3)), g.lin(torch.zeros(1, 1), 0), g.lout((1, 8)), g.fout((1, 8, 3))
    st = A.cur_stream()
    for N, npoint in ((4097, 4), (0, 4), (8, 0)):
        assert rc_of(A, "prifit_fps", A.ptr(x), 1, N, npoint, A.ptr(s), A.ptr(out), A.ptr(new), st) == EINVAL
    assert rc_of(A, "prifit_fps", None, 1, 8, 4, A.ptr(s), A.ptr(out), A.ptr(new), st) == EINVAL
    assert rc_of(A, "prifit_fps", A.ptr(x), 1, 8, 4, None, A.ptr(out), A.ptr(new), st) == EINVAL
    assert rc_of(A, "prifit_fps", A.ptr(x), 1, 8, 4, A.ptr(s), None, A.ptr(new), st) == EINVAL
    untouched(out, new)
    assert rc_of(A, "prifit_fps", A.ptr(x), 1, 8, 4, A.ptr(s), A.ptr(out), A.ptr(new), st) == 0          # the call they differ from
    in_range(7, out[:, :4])
    g.intact()


# ---------------------------------------------------------------------------------------------------------------------------
# ball query: prifit_ball_query and phase 1 of the front end
# ---------------------------------------------------------------------------------------------------------------------------
def run_ball_query(A, g, xd, cd, B, N, S, r2, ks, idx64):
    outs = [(g.lout if idx64 else g.iout)((B, S, K)) for K in ks]
    ok_rc(A, "prifit_ball_query", A.ptr(xd), A.ptr(cd), B, N, S, len(ks), floats(r2), ints(ks), ptrs(outs), int(idx64), A.cur_stream())
    return outs


def run_front(A, g, xd, cd, B, N, S, r2, ks, widths, mode=0, feat=None, D=0, feat_first=0, feat_xyz=0, W=None, U=None, Vc=None,
              bias=None, want_Y=True, want_slab=True, expect=0):
    """prifit_sa_group_linear_fwd with its outputs in guards -> Y, slab, idx (lists; None where not asked for)"""
    R = len(ks)
    q = A.query("prifit_sa_group_queries_per_slab", B, S)
    Y = [g.fout((B * S * K, C)) if want_Y else None for K, C in zip(ks, widths)]
    slab = [g.fout((B * -(-S // q), 2, C)) if want_slab else None for C in widths]
    idx = [g.iout((B, S, K)) for K in ks]
    none = [None] * R
    rc = rc_of(A, "prifit_sa_group_linear_fwd", A.ptr(xd), A.ptr(cd), B, N, S, R, floats(r2), ints(ks), ints(widths), mode, A.ptr(feat), D,
               feat_first, feat_xyz, ptrs(W or none), ptrs(U or none), ptrs(Vc or none), ptrs(bias or none), ptrs(Y), ptrs(slab),
               ptrs(idx), A.cur_stream())
    assert rc == expect
    return Y, slab, idx


def check_ball(A, xyz, ctr, r2, ks, want, front=True):
    """both entry points on one case: lists exact, equal to each other, guards intact"""
    B, N, _ = xyz.shape
    S = ctr.shape[1]
    g = Bufs()
    xd, cd = g.fin(xyz), g.fin(ctr)
    o32, o64 = run_ball_query(A, g, xd, cd, B, N, S, r2, ks, 0), run_ball_query(A, g, xd, cd, B, N, S, r2, ks, 1)
    fidx = None
    if front and N <= 2048 and sum(ks) <= 320:
        W = [g.fin(torch.ones(16, 3)) for _ in ks]
        Y, slab, fidx = run_front(A, g, xd, cd, B, N, S, r2, ks, [16] * len(ks), W=W)
        finite(*Y, *slab)
    in_range(N, *o32, *o64, *(fidx or []))
    g.intact()
    for r, w in enumerate(want):
        assert same(o64[r], w), ("idx64", N, S, r)
        assert same(o32[r], w.int()), ("idx32", N, S, r)
        if fidx is not None:
            assert same(fidx[r], o32[r]), ("front end", N, S, r)


@pytest.mark.parametrize("N", sc.BALL_N + sc.BALL_N_QUERY_ONLY)
def test_ball_query_and_front_end_lists_in_guards_exactly(A, N):
    for S in sc.ball_Ss(N):
        for r2u, ks in sc.BALL_RK:
            for B in sc.ball_Bs(N):
                xyz, ctr = sc.ball_case(N, S, r2u, B)
                r2 = sc.r2_of(r2u)
                want = [sc.ball_query(xyz, ctr, r, K) for r, K in zip(r2, ks)]
                if S > 1:                                   # the empty ball: every slot equals N
                    assert all(bool((w[:, S - 1] == N).all()) for w in want)
                check_ball(A, xyz, ctr, r2, ks, want)
    # off the lattice: the bit-exact recipe
    B, S = 3, 5
    xyz = _t(synth.cloud("cube", B, N, 50 + N))
    ctr = torch.cat([xyz[:, :S - 1], torch.full((B, 1, 3), sc.FAR)], 1) if N >= S else xyz[:, :1].expand(B, S, 3).contiguous()
    radii, ks = (0.4, 1.2, 0.2), (16, 65, 7)
    r2 = [float(np.float32(r ** 2)) for r in radii]
    check_ball(A, xyz, ctr, r2, ks, [orc.c_query_ball_point(r, K, xyz, ctr) for r, K in zip(radii, ks)])


def test_ball_query_exact_k_and_limits(A):
    # a ball with exactly K members (radius 0: the copies of the centre), K = 64 and one short / one over
    xyz, ctr = sc.ball_case(*sc.EXACT_K_CASE)
    for K in (sc.EXACT_K - 1, sc.EXACT_K, sc.EXACT_K + 1):
        want = sc.ball_query(xyz, ctr, 0.0, K)
        assert int((want[0, 0] == want[0, 0, 0]).sum()) == (2 if K > sc.EXACT_K else 1)
        check_ball(A, xyz, ctr, [0.0], [K], [want])
    # K = 1024 is accepted (more members than K, fewer, K > N) and 1025 is not
    for args in sc.K_MAX_CASES:
        xyz, ctr = sc.ball_case(*args)
        for r2u in (sc.R2_ALL, sc.R2_BIG):
            check_ball(A, xyz, ctr, sc.r2_of([r2u]), [sc.BALL_K_MAX], [sc.ball_query(xyz, ctr, r2u * sc.UNIT2, sc.BALL_K_MAX)], front=False)
    g = Bufs()
    xd, cd, out = g.fin(xyz), g.fin(ctr), g.iout((1, 3, 1025))
    st = A.cur_stream()

    def rc(N=1500, S=3, R=1, ks=(4,), o=(out,), x=xd):
        return rc_of(A, "prifit_ball_query", A.ptr(x), A.ptr(cd), 1, N, S, R, floats([1.0] * len(ks)), ints(ks), ptrs(list(o)), 0, st)
    assert rc() == 0
    out.fill_(poison_bits(SENTINEL))
    for kw in (dict(ks=(1025,)), dict(ks=(0,)), dict(N=0), dict(S=0), dict(R=0), dict(R=5, ks=(4,) * 5, o=(out,) * 5), dict(o=(None,)), dict(x=None)):
        assert rc(**kw) == EINVAL, kw
    untouched(out)
    g.intact()


# ---------------------------------------------------------------------------------------------------------------------------
# three nearest neighbours, square distance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sc.THREE_NN_S)
def test_three_nn_in_guards(A, S):
    rep = bc.Report()
    for N in sc.THREE_NN_N:
        for kind, B in (("lattice", 3), ("lattice", 1), ("cube", 3)):
            if kind == "lattice":
                q, p = sc.nn_case(N, S, B)
                d3, i3 = sc.three_nn(q, p)
                assert bool((d3[:, ::2, 0] == 0).all())                     # queries that coincide with a candidate
            else:
                q, p = _t(synth.cloud("cube", B, N, 60 + N)), _t(synth.cloud("cube", B, S, 61 + S))
                d3, i3 = orc.c_three_nn(q, p)
            for give in (False, True):
                g = Bufs()
                qd, pd = g.fin(q), g.fin(p)
                idx, w, dist = g.iout((B, N, 3)), g.fout((B, N, 3)), (g.fout((B, N, 3)) if give else None)
                ok_rc(A, "prifit_three_nn", A.ptr(qd), A.ptr(pd), B, N, S, A.ptr(idx), A.ptr(dist), A.ptr(w), A.cur_stream())
                in_range(S - 1, idx)
                finite(w, *([dist] if give else []))
                g.intact()
                assert same(idx, i3.int()), (kind, N, S, B)
                if give:
                    assert same(dist, d3.to(F32))
                rep.ew("nn_weight", (kind, N, S, B), w, sc.nn_weights(d3.to(F32)), sc.nn_weights(d3.to(F32), F32))
    rep.assert_bars()


def test_three_nn_rejects_fewer_than_three_candidates(A):
    g = Bufs()
    q, idx, w = g.fin(torch.zeros(1, 4, 3)), g.iout((1, 4, 3)), g.fout((1, 4, 3))
    st = A.cur_stream()
    assert rc_of(A, "prifit_three_nn", A.ptr(q), A.ptr(q), 1, 4, 2, A.ptr(idx), None, A.ptr(w), st) == EINVAL
    assert rc_of(A, "prifit_three_nn", A.ptr(q), A.ptr(q), 1, 0, 4, A.ptr(idx), None, A.ptr(w), st) == EINVAL
    assert rc_of(A, "prifit_three_nn", A.ptr(q), A.ptr(q), 1, 4, 4, A.ptr(idx), None, None, st) == EINVAL
    untouched(idx, w)
    assert rc_of(A, "prifit_three_nn", A.ptr(q), A.ptr(q), 1, 4, 4, A.ptr(idx), None, A.ptr(w), st) == 0       # the call they differ from
    in_range(3, idx)
    finite(w)
    g.intact()


@pytest.mark.parametrize("S", sc.SQDIST_SIZES)
def test_square_distance_in_guards_exactly(A, S):
    for N in sc.SQDIST_SIZES:
        for kind, B in (("lattice", 3), ("lattice", 1), ("cube", 3)):
            if kind == "lattice":
                src, dst = sc.sqdist_case(S, N, B)
                want = sc.sqdist_expanded(src, dst).to(F32)
            else:
                src, dst = _t(synth.cloud("cube", B, S, 70 + S)), _t(synth.cloud("cube", B, N, 71 + N))
                want = orc.c_square_distance(src, dst)
            g = Bufs()
            sd, dd, out = g.fin(src), g.fin(dst), g.fout((B, S, N))
            ok_rc(A, "prifit_square_distance", A.ptr(sd), A.ptr(dd), B, S, N, A.ptr(out), A.cur_stream())
            finite(out)
            g.intact()
            assert same(out, want), (kind, S, N, B)


# ---------------------------------------------------------------------------------------------------------------------------
# group gather / scatter-add, interpolation, fp_rows
# ---------------------------------------------------------------------------------------------------------------------------
def poisoned_rows(t):
    """the device copy's row N - 1 (the index the guards around the lists hold) is NaN: its use shows in the result"""
    t = t.clone()
    t[:, -1] = float("nan")
    return t


@pytest.mark.parametrize("C,order,ld,off", sc.GATHER_VECTOR + sc.GATHER_ROW8 + sc.GATHER_SCALAR)
def test_group_gather_in_guards_bit_for_bit(A, C, order, ld, off):
    N, S, K = sc.GATHER_N, sc.GATHER_S, sc.GATHER_K
    for B in (1, sc.GATHER_B):
        gen = bc.gen_of(bc.seed_of(47, C, order, ld, B))
        xyz, ctr = torch.randn(B, N, 3, generator=gen), torch.randn(B, S, 3, generator=gen)
        feat = torch.randn(B, N, C, generator=gen) if C else None
        idx = sc.oob_index((B, S, K), N, gen)
        rows = B * S * K
        g = Bufs()
        xd, cd, ix = g.fin(poisoned_rows(xyz)), g.fin(ctr), g.iin(idx, N - 1)
        fd = g.fin(poisoned_rows(feat)) if C else None
        buf = g.fout((rows * ld + 4,))
        out = buf[off // 4:off // 4 + rows * ld].view(rows, ld)
        ok_rc(A, "prifit_group_gather", A.ptr(fd), A.ptr(xd), A.ptr(cd), A.ptr(ix), B, N, S, K, C, order, ld, A.ptr(out), A.cur_stream())
        finite(out)
        g.intact()
        assert bool((torch.cat([buf[:off // 4], buf[off // 4 + rows * ld:]]).view(I32) == poison_bits(SENTINEL)).all())
        want = sc.grouped_rows(xyz, ctr, feat, idx, order == 0, F32).reshape(rows, C + 3)
        assert same(out[:, :C + 3], want)
        assert not bool(out[:, C + 3:].any())
        bad = ((idx < 0) | (idx >= N)).reshape(-1)
        assert bool(bad.any()) and not bool(out.cpu()[bad].any())


def pad_matrix(g, t, col0, ld):
    """t [P, C] at column col0 of a NaN matrix with row stride ld, in NaN guards -> the [P, col0 + C] view"""
    P, C = t.shape
    full = torch.full((P, col0 + C), float("nan"))
    full[:, col0:] = t
    return g.fin(full, ld)


@pytest.mark.parametrize("C,col0,ld,hub", sc.SCATTER_CASES)
def test_group_scatter_add_in_guards_against_fp64(A, C, col0, ld, hub):
    rep = bc.Report()
    N, S, K = sc.GATHER_N, sc.GATHER_S, sc.GATHER_K
    for B in (1, 3):
        gen = bc.gen_of(bc.seed_of(48, C, col0, ld, hub, B))
        idx = sc.oob_index((B, S, K), N, gen)
        if hub:
            idx[:] = 5
        gout, d0 = torch.randn(B, S * K, C, generator=gen).to(F32), torch.randn(B, N, C, generator=gen).to(F32)
        g = Bufs()
        gd, ix = pad_matrix(g, gout.view(-1, C), col0, ld), g.iin(idx, N - 1)
        d1, d2 = g.fout((B, N, C), init=d0), g.fout((B, N, C), init=d0)
        for d in (d1, d2):
            ok_rc(A, "prifit_group_scatter_add", A.ptr(gd), ld, col0, A.ptr(ix), B, N, S, K, C, A.ptr(d), A.cur_stream())
        finite(d1)
        g.intact()
        flat = idx.reshape(B, -1)
        assert same(d1[:, N - 1], d0[:, N - 1])            # no list names point N - 1: nothing was added
        absum = sc.scatter_add_absum(gout, flat, d0)
        rep.red("scatter_dfeat", (C, col0, ld, hub, B), d1, sc.scatter_add(gout, flat, d0), sc.scatter_add(gout, flat, d0, F32), absum)
        print("RERUN scatter_dfeat %s %.3e" % ((C, col0, ld, hub, B), rerun_diff(d1, d2, absum)))
    rep.assert_bars()


def interp_inputs(B, N, S, C, gen):
    """idx3 in [0, S - 1) (row S - 1 of points2 is the poison row), positive weights that sum to one"""
    i3 = torch.randint(0, S - 1, (B, N, 3), generator=gen, dtype=I32)
    w = torch.rand(B, N, 3, generator=gen) + 0.05
    return torch.randn(B, S, C, generator=gen).to(F32), i3, (w / w.sum(-1, keepdim=True)).to(F32)


@pytest.mark.parametrize("C,col0,ld,hub", sc.SCATTER_CASES)
def test_three_interpolate_bwd_in_guards_against_fp64(A, C, col0, ld, hub):
    rep = bc.Report()
    N, S = sc.GATHER_N, sc.INTERP_S
    for B in (1, 3):
        gen = bc.gen_of(bc.seed_of(49, C, col0, ld, hub, B))
        _, i3, w = interp_inputs(B, N, S, C, gen)
        if hub:
            i3[:] = 2
        gout, d0 = torch.randn(B, N, C, generator=gen).to(F32), torch.randn(B, S, C, generator=gen).to(F32)
        g = Bufs()
        gd, ix, wd = pad_matrix(g, gout.view(-1, C), col0, ld), g.iin(i3, S - 1), g.fin(w)
        d1, d2 = g.fout((B, S, C), init=d0), g.fout((B, S, C), init=d0)
        for d in (d1, d2):
            ok_rc(A, "prifit_three_interpolate_bwd", A.ptr(gd), ld, col0, A.ptr(ix), A.ptr(wd), B, N, S, C, A.ptr(d), A.cur_stream())
        finite(d1)
        g.intact()
        assert same(d1[:, S - 1], d0[:, S - 1])
        absum = sc.interpolate_bwd_absum(gout, i3, w, d0)
        rep.red("interp_dp2", (C, col0, ld, hub, B), d1, sc.interpolate_bwd(gout, i3, w, d0), sc.interpolate_bwd(gout, i3, w, d0, F32), absum)
        print("RERUN interp_dp2 %s %.3e" % ((C, col0, ld, hub, B), rerun_diff(d1, d2, absum)))
    rep.assert_bars()


@pytest.mark.parametrize("C,N,col0,pad", sc.INTERP_CASES)
def test_three_interpolate_in_guards_against_fp64(A, C, N, col0, pad):
    rep = bc.Report()
    S = sc.INTERP_S
    for B in (1, 3):
        p2, i3, w = interp_inputs(B, N, S, C, bc.gen_of(bc.seed_of(54, C, N, col0, B)))
        g = Bufs()
        pd, ix, wd = g.fin(poisoned_rows(p2)), g.iin(i3, S - 1), g.fin(w)
        out = g.mout(B * N, C, col0 + C + pad, col0, col0 + C + pad)
        ok_rc(A, "prifit_three_interpolate", A.ptr(pd), A.ptr(ix), A.ptr(wd), B, N, S, C, out.stride(0), col0, A.ptr(out) - 4 * col0, A.cur_stream())
        finite(out)
        g.intact()
        rep.ew("interp_out", (C, N, col0, pad, B), out.reshape(B, N, C), sc.interpolate(p2, i3, w), sc.interpolate(p2, i3, w, F32))
    rep.assert_bars()


@pytest.mark.parametrize("D2,D1,pad,N", sc.FP_ROWS_CASES)
def test_fp_rows_in_guards_against_fp64(A, D2, D1, pad, N):
    rep = bc.Report()
    kp = D2 + D1 + pad
    for B in (1, 3):
        for S in (sc.INTERP_S, 1):
            gen = bc.gen_of(bc.seed_of(55, D2, D1, pad, N, B, S))
            p2, i3, w = interp_inputs(B, N, max(S, 3), D2, gen)
            p2 = p2[:, :S].contiguous() if S == 1 else p2
            p1 = torch.randn(B, N, D1, generator=gen).to(F32) if D1 else None
            g = Bufs()
            pd = g.fin(poisoned_rows(p2) if S > 1 else p2)
            ix, wd = (g.iin(i3, S - 1), g.fin(w)) if S > 1 else (None, None)
            p1d = g.fin(p1) if D1 else None
            out = g.fout((B * N, kp))
            ok_rc(A, "prifit_fp_rows", A.ptr(pd), A.ptr(ix), A.ptr(wd), A.ptr(p1d), B, N, S, D2, D1, kp, A.ptr(out), A.cur_stream())
            finite(out)
            g.intact()
            a3, aw = (i3, w) if S > 1 else (None, None)
            r64, r32 = sc.fp_rows(p2, a3, aw, p1, kp, N), sc.fp_rows(p2, a3, aw, p1, kp, N, F32)
            o = out.view(B, N, kp)
            assert not bool(o[:, :, D2 + D1:].any())
            assert same(o[:, :, D2:], r32[:, :, D2:])                      # points1 and the pad: moves
            if S == 1:
                assert same(o[:, :, :D2], p2.expand(B, N, D2))
            else:                                           # the left block equals prifit_three_interpolate bit for bit
                ti = g.fout((B * N, D2))
                ok_rc(A, "prifit_three_interpolate", A.ptr(pd), A.ptr(ix), A.ptr(wd), B, N, S, D2, D2, 0, A.ptr(ti), A.cur_stream())
                finite(ti)
                g.intact()
                assert same(o[:, :, :D2], ti.view(B, N, D2))
            rep.ew("fp_rows", (D2, D1, pad, N, B, S), o, r64, r32)
    rep.assert_bars()


def test_interpolation_rejects_unsupported_arguments(A):
    """every rejected call differs in one argument from a call that is accepted"""
    g = Bufs()
    p2, ix, w = g.fin(torch.zeros(1, 2, 4)), g.iin(torch.zeros(1, 5, 3, dtype=I32), 0), g.fin(torch.zeros(1, 5, 3))
    gin, out, acc = g.fin(torch.zeros(5, 8)), g.fout((5, 8)), g.fout((1, 5, 4), zero=True)
    st = A.cur_stream()

    def fp(idx=ix, wt=w, D1=0, kp=4):
        return rc_of(A, "prifit_fp_rows", A.ptr(p2), A.ptr(idx), A.ptr(wt), None, 1, 5, 2, 4, D1, kp, A.ptr(out), st)

    def ti(ld=8):
        return rc_of(A, "prifit_three_interpolate", A.ptr(p2), A.ptr(ix), A.ptr(w), 1, 5, 2, 4, ld, 2, A.ptr(out), st)

    def tib(ld=8):
        return rc_of(A, "prifit_three_interpolate_bwd", A.ptr(gin), ld, 2, A.ptr(ix), A.ptr(w), 1, 5, 2, 4, A.ptr(acc), st)

    def sca(ld=8):
        return rc_of(A, "prifit_group_scatter_add", A.ptr(gin), ld, 2, A.ptr(ix), 1, 5, 1, 3, 4, A.ptr(acc), st)

    def gat(ld=3):
        return rc_of(A, "prifit_group_gather", None, A.ptr(w), A.ptr(w), A.ptr(ix), 1, 5, 1, 3, 0, 0, ld, A.ptr(out), st)
    assert fp(idx=None) == EINVAL                           # idx == NULL with S = 2
    assert fp(wt=None) == EINVAL and fp(kp=3) == EINVAL and fp(D1=2, kp=8) == EINVAL
    assert ti(ld=5) == EINVAL and tib(ld=5) == EINVAL and sca(ld=5) == EINVAL and gat(ld=2) == EINVAL
    untouched(out)
    torch.cuda.synchronize()
    assert not bool(acc.any())
    assert fp() == 0 and fp(kp=8) == 0 and ti() == 0 and tib() == 0 and sca() == 0 and gat() == 0
    finite(acc)
    g.intact()


# ---------------------------------------------------------------------------------------------------------------------------
# column packers
# ---------------------------------------------------------------------------------------------------------------------------
def test_pack_and_unpack_cols_in_guards_exactly(A):
    gen = bc.gen_of(56)
    st = A.cur_stream()
    g = Bufs()
    jobs = []
    for (rows, scols), cmap in zip(sc.PACK_SHAPES, sc.PACK_MAPS):
        w, gr = torch.randn(rows, scols, generator=gen).to(F32), torch.randn(rows, len(cmap), generator=gen).to(F32)
        off, inv = sc.inverse_map(cmap, scols)
        m = torch.tensor(cmap)
        jobs.append(dict(rows=rows, scols=scols, dcols=len(cmap), w=g.fin(w), gr=g.fin(gr), map=g.iin(m, 0), off=g.iin(off, 0),
                         inv=g.iin(inv, 0), want=w.index_select(1, m.clamp(min=0)) * (m >= 0),
                         want_gw=torch.zeros(rows, scols).index_add_(1, m[m >= 0], gr[:, m >= 0])))
        assert torch.equal(jobs[-1]["want"], sc.pack_cols(w, cmap).to(F32))
    n = len(jobs)
    single = [(g.fout((j["rows"], j["dcols"])), g.fout((j["rows"], j["scols"]))) for j in jobs]
    multi = [(g.fout((j["rows"], j["dcols"])), g.fout((j["rows"], j["scols"]))) for j in jobs]
    for j, (o, gw) in zip(jobs, single):
        ok_rc(A, "prifit_pack_cols", A.ptr(j["w"]), j["rows"], j["scols"], A.ptr(j["map"]), j["dcols"], A.ptr(o), st)
        ok_rc(A, "prifit_unpack_cols", A.ptr(j["gr"]), j["rows"], j["dcols"], A.ptr(j["off"]), A.ptr(j["inv"]), j["scols"], A.ptr(gw), st)
    i32 = lambda key: (ctypes.c_int32 * n)(*[j[key] for j in jobs])
    ok_rc(A, "prifit_pack_cols_multi", n, ptrs([j["w"] for j in jobs]), i32("rows"), i32("scols"), ptrs([j["map"] for j in jobs]),
          i32("dcols"), ptrs([o for o, _ in multi]), st)
    ok_rc(A, "prifit_unpack_cols_multi", n, ptrs([j["gr"] for j in jobs]), i32("rows"), i32("dcols"), ptrs([j["off"] for j in jobs]),
          ptrs([j["inv"] for j in jobs]), i32("scols"), ptrs([gw for _, gw in multi]), st)
    finite(*[t for pair in single + multi for t in pair])
    g.intact()
    for j, (o, gw), (mo, mgw) in zip(jobs, single, multi):
        assert same(o, j["want"]) and same(mo, j["want"])
        assert same(gw, j["want_gw"]) and same(mgw, j["want_gw"])


def test_pack_cols_multi_takes_max_jobs_and_rejects_one_more(A):
    most = A.query("prifit_pack_cols_max_jobs")
    st = A.cur_stream()
    g = Bufs()
    w, m = g.fin(torch.arange(12.0).view(3, 4)), g.iin(torch.tensor([2, -1, 0]), 0)
    off, inv = (g.iin(t, 0) for t in sc.inverse_map((2, -1, 0), 4))
    gr = g.fin(torch.arange(9.0).view(3, 3))
    outs, gws = [g.fout((3, 3)) for _ in range(most + 1)], [g.fout((3, 4)) for _ in range(most + 1)]

    def run(n):
        c = lambda v: (ctypes.c_int32 * n)(*[v] * n)
        return (rc_of(A, "prifit_pack_cols_multi", n, ptrs([w] * n), c(3), c(4), ptrs([m] * n), c(3), ptrs(outs[:n]), st),
                rc_of(A, "prifit_unpack_cols_multi", n, ptrs([gr] * n), c(3), c(3), ptrs([off] * n), ptrs([inv] * n), c(4), ptrs(gws[:n]), st))
    assert run(most + 1) == (EINVAL, EINVAL) and run(0) == (EINVAL, EINVAL)
    untouched(*outs, *gws)
    assert run(most) == (0, 0)
    finite(*outs[:most], *gws[:most])
    g.intact()
    for o, gw in zip(outs[:most], gws[:most]):
        assert same(o, torch.tensor([[2.0, 0, 0], [6, 0, 4], [10, 0, 8]]))
        assert same(gw, torch.tensor([[2.0, 0, 0, 0], [5, 0, 3, 0], [8, 0, 6, 0]]))
    untouched(outs[most], gws[most])


# ---------------------------------------------------------------------------------------------------------------------------
# the front end's rows and slabs
# ---------------------------------------------------------------------------------------------------------------------------
def front_radii(n, rot):
    """n squared radii (lattice units), the largest at position rot % n"""
    base = [sc.R2_SMALL, sc.R2_MID, sc.R2_TINY][:n - 1]
    base.insert(rot % n if isinstance(rot, int) else 0, sc.R2_BIG)
    return base


def compare_front(rep, name, tag, A, B, S, ks, widths, Y, slab, Y64, Y32):
    q = A.query("prifit_sa_group_queries_per_slab", B, S)
    for r, (K, C) in enumerate(zip(ks, widths)):
        if Y[r] is not None:
            rep.ew(name + "_rows", tag + (C, K), Y[r].view(B, S, K, C), Y64[r], Y32[r])
        if slab[r] is not None:
            s64, s32, ab = sc.slab_stats(Y64[r], q), sc.slab_stats(Y32[r], q, F32), sc.slab_absum(Y64[r], q)
            ab[:, 1] = s64[:, 1]
            for h, nm in enumerate(("_slab_s", "_slab_q")):
                rep.red(name + nm, tag + (C, K), slab[r][:, h], s64[:, h], s32[:, h], ab[:, h])


@pytest.mark.parametrize("D,feat_first,B,S,N,rot", sc.SG_DIRECT)
def test_front_end_direct_mode_in_guards_against_fp64(A, D, feat_first, B, S, N, rot):
    rep = bc.Report()
    widths, ks = sc.sg_shape(rot)
    case = sc.sg_case(B, S, N, D, widths, 1)
    r2u = front_radii(4, rot)
    r2 = sc.r2_of(r2u)
    want = [sc.ball_query(case["xyz"], case["ctr"], r, K) for r, K in zip(r2, ks)]
    g = Bufs()
    xd, cd = g.fin(case["xyz"]), g.fin(case["ctr"])
    fd = g.fin(case["feat"]) if D else None
    W = [g.fin(w) for w in case["W"]]
    bias = [g.fin(b) if r % 2 == 0 else None for r, b in enumerate(case["bias"])]
    runs = [run_front(A, g, xd, cd, B, N, S, r2, ks, widths, 0, fd, D, feat_first, fx, W, bias=bias) for fx in ((0, 1) if D else (0,))]
    Y, slab, idx = runs[0]
    finite(*[t for run in runs for t in run[0] + run[1]])
    in_range(N, *[t for run in runs for t in run[2]])
    g.intact()
    for r in range(4):
        assert same(idx[r], want[r].int()), r
        for Y2, slab2, idx2 in runs[1:]:                    # features 0..2 taken from the LDS cloud: the same bits
            assert same(Y[r], Y2[r]) and same(slab[r], slab2[r]) and same(idx[r], idx2[r])
        if S > 1:                                           # the empty ball: its rows are the bias
            bv = case["bias"][r] if r % 2 == 0 else torch.zeros(widths[r])
            assert same(Y[r].view(B, S, ks[r], -1)[:, S - 1], bv.expand(B, ks[r], widths[r]))
    Ys = [[sc.first_layer(sc.grouped_rows(case["xyz"], case["ctr"], case["feat"], want[r], feat_first, dt), case["W"][r],
                          case["bias"][r] if r % 2 == 0 else None, dt) for r in range(4)] for dt in (F64, F32)]
    compare_front(rep, "direct", (D, feat_first, B, S, N), A, B, S, ks, widths, Y, slab, Ys[0], Ys[1])
    rep.assert_bars()


@pytest.mark.parametrize("null,B,S,N,rot", sc.SG_GATHER)
def test_front_end_gather_mode_in_guards_against_fp64(A, null, B, S, N, rot):
    rep = bc.Report()
    widths, ks = sc.sg_shape(rot)
    case = sc.sg_case(B, S, N, 0, widths, 2)
    r2 = sc.r2_of(front_radii(4, rot if isinstance(rot, int) else 3))
    want = [sc.ball_query(case["xyz"], case["ctr"], r, K) for r, K in zip(r2, ks)]
    g = Bufs()
    xd, cd = g.fin(case["xyz"]), g.fin(case["ctr"])
    U, Vc = [g.fin(u) for u in case["U"]], [g.fin(v) for v in case["Vc"]]
    bias = [None if null == "bias" else g.fin(b) for b in case["bias"]]
    Y, slab, idx = run_front(A, g, xd, cd, B, N, S, r2, ks, widths, 1, U=U, Vc=Vc, bias=bias, want_Y=null != "Y", want_slab=null != "slab")
    finite(*[t for t in Y + slab if t is not None])
    in_range(N, *idx)
    g.intact()
    for r in range(4):
        assert same(idx[r], want[r].int()), r
        if S > 1 and Y[r] is not None:                      # the empty ball: the bias alone, neither U nor Vc
            bv = torch.zeros(widths[r]) if null == "bias" else case["bias"][r]
            assert same(Y[r].view(B, S, ks[r], -1)[:, S - 1], bv.expand(B, ks[r], widths[r]))
    Ys = [[sc.gather_layer(case["U"][r], case["Vc"][r], None if null == "bias" else case["bias"][r], want[r], dt) for r in range(4)]
          for dt in (F64, F32)]
    compare_front(rep, "gather", (null, B, S, N), A, B, S, ks, widths, Y, slab, Ys[0], Ys[1])
    rep.assert_bars()


def test_front_end_eight_waves_with_idle_trailing_waves_against_fp64(A):
    rep = bc.Report()
    e = sc.SG_EIGHT_WAVE
    B, S, N, K, C = e["B"], e["S"], e["N"], e["K"], e["C"]
    assert A.query("prifit_sa_group_queries_per_slab", B, S) == 8
    case = sc.sg_case(B, S, N, 3, [C], 3)
    r2 = sc.r2_of([sc.R2_BIG])
    want = sc.ball_query(case["xyz"], case["ctr"], r2[0], K)
    g = Bufs()
    xd, cd, fd = g.fin(case["xyz"]), g.fin(case["ctr"]), g.fin(case["feat"])
    Y, slab, idx = run_front(A, g, xd, cd, B, N, S, r2, [K], [C], 0, fd, 3, 1, 0, [g.fin(case["W"][0])], bias=[g.fin(case["bias"][0])])
    assert slab[0].shape[0] == B * 128
    finite(Y[0], slab[0])
    in_range(N, idx[0])
    g.intact()
    assert same(idx[0], want.int())
    Ys = [[sc.first_layer(sc.grouped_rows(case["xyz"], case["ctr"], case["feat"], want, 1, dt), case["W"][0], case["bias"][0], dt)] for dt in (F64, F32)]
    compare_front(rep, "wave8", (B, S, N), A, B, S, [K], [C], Y, slab, Ys[0], Ys[1])
    rep.assert_bars()


def test_front_end_rejects_unsupported_arguments(A):
    B, S, N = sc.SG_REJECT_CASE[:3]
    case = sc.sg_case(*sc.SG_REJECT_CASE)
    g = Bufs()
    xd, cd, fd = g.fin(case["xyz"]), g.fin(case["ctr"]), g.fin(case["feat"])
    st = A.cur_stream()
    big = g.fout((B * S * 128 * 128 + 4,))
    slab, idx = g.fout((2, 128)), g.iout((B, S, 128))
    W, U, bias = g.fin(torch.ones(256, 6)), g.fin(torch.ones(B * N * 128 + 4)), g.fin(torch.ones(260))

    def rc(N=N, R=1, ks=(4,), widths=(16,), mode=0, Y=(big,), Ws=(W,), Us=(U,), Vcs=(U,), bs=(bias,), yoff=0, uoff=0, voff=0, boff=0):
        at = lambda ts, o: (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() + o for t in ts])
        n = len(ks)
        return rc_of(A, "prifit_sa_group_linear_fwd", A.ptr(xd), A.ptr(cd), B, N, S, R, floats([1.0] * n), ints(ks), ints(widths), mode,
                     A.ptr(fd), 3, 1, 0, at(Ws * n if len(Ws) == 1 else Ws, 0), at(Us * n if len(Us) == 1 else Us, uoff),
                     at(Vcs * n if len(Vcs) == 1 else Vcs, voff), at(bs * n if len(bs) == 1 else bs, boff),
                     at(Y * n if len(Y) == 1 else Y, yoff), ptrs([slab] * n), ptrs([idx] * n), st)
    for kw in ([dict(widths=(c,)) for c in (8, 24, 256)] + [dict(yoff=4), dict(boff=4), dict(mode=1, uoff=4), dict(mode=1, voff=4),
               dict(mode=1, yoff=8), dict(Y=(None,)), dict(N=2049), dict(R=4, ks=(64, 128, 96, 33), widths=(16, 128, 32, 64)), dict(ks=(0,)),
               dict(mode=2), dict(R=5, ks=(4,) * 5, widths=(16,) * 5)]):
        assert rc(**kw) == EINVAL, kw
    untouched(big, slab, idx)
    assert rc() == 0 and rc(mode=1) == 0                    # the call the rejected ones differ from in one argument
    finite(big[:B * S * 4 * 16])
    g.intact()


# ---------------------------------------------------------------------------------------------------------------------------
# the per-point / per-centre tables
# ---------------------------------------------------------------------------------------------------------------------------
def run_tables(A, g, xd, cd, fd, B, N, S, D, feat_first, widths, W, bias):
    U, Vc = [g.fout((B, N, C)) for C in widths], [g.fout((B, S, C)) for C in widths]
    ok_rc(A, "prifit_sa_point_tables", A.ptr(xd), A.ptr(cd), A.ptr(fd), B, N, S, D, feat_first, len(widths), ints(widths), ptrs(W), ptrs(bias),
          ptrs(U), ptrs(Vc), A.cur_stream())
    return U, Vc


@pytest.mark.parametrize("D,feat_first,widths,with_bias", sc.TABLES_CASES)
def test_point_tables_in_guards_against_fp64(A, D, feat_first, widths, with_bias):
    rep = bc.Report()
    N, S = sc.TABLES_N, sc.TABLES_S
    for B in (1, sc.TABLES_B):
        gen = bc.gen_of(bc.seed_of(57, D, feat_first, len(widths), B))
        xyz, ctr = torch.randn(B, N, 3, generator=gen).to(F32), torch.randn(B, S, 3, generator=gen).to(F32)
        feat = torch.randn(B, N, D, generator=gen).to(F32) if D else None
        Ws = [(0.5 * torch.randn(C, D + 3, generator=gen)).to(F32) for C in widths]
        bs = [torch.randn(C, generator=gen).to(F32) if with_bias else None for C in widths]
        g = Bufs()
        xd, cd, fd = g.fin(xyz), g.fin(ctr), (g.fin(feat) if D else None)
        U, Vc = run_tables(A, g, xd, cd, fd, B, N, S, D, feat_first, widths, [g.fin(w) for w in Ws], [None if b is None else g.fin(b) for b in bs])
        finite(*U, *Vc)
        g.intact()
        idx = torch.arange(N).expand(B, S, N)
        for r, C in enumerate(widths):
            tag = (D, feat_first, C, with_bias, B)
            (u64, v64), (u32, v32) = (sc.point_tables(xyz, ctr, feat, Ws[r], bs[r], feat_first, dt) for dt in (F64, F32))
            rep.ew("tables_U", tag, U[r], u64, u32)
            rep.ew("tables_Vc", tag, Vc[r], v64, v32)
            # U_j - Vc_s == conv1([feat_j | xyz_j - c_s]) + b: it cancels, so in units of the sum of the |terms|
            rows = sc.grouped_rows(xyz, ctr, feat, idx, feat_first)
            y64 = sc.first_layer(rows, Ws[r], bs[r])
            ab = sc.point_tables(xyz.abs(), ctr.abs(), None if feat is None else feat.abs(), Ws[r].abs(), None if bs[r] is None else bs[r].abs(), feat_first)
            absum = ab[0].unsqueeze(1) + ab[1].unsqueeze(2)
            got = U[r].cpu().to(F64).unsqueeze(1) - Vc[r].cpu().to(F64).unsqueeze(2)
            rep.red("tables_ident", tag, got, y64, u32.to(F64).unsqueeze(1) - v32.to(F64).unsqueeze(2), absum)
    rep.assert_bars()


def test_point_tables_rejects_unsupported_arguments(A):
    g = Bufs()
    x, W = g.fin(torch.zeros(1, 4, 3)), g.fin(torch.zeros(8, 3))
    U, Vc = g.fout((4 * 8 + 4,)), g.fout((4 * 8,))
    st = A.cur_stream()

    def rc(width=8, uoff=0, D=0, R=1, Wp=W):
        return rc_of(A, "prifit_sa_point_tables", A.ptr(x), A.ptr(x), None, 1, 4, 4, D, 1, R, ints([width]), ptrs([Wp]), ptrs([None]),
                     (ctypes.c_void_p * 1)(U.data_ptr() + uoff), ptrs([Vc]), st)
    for kw in (dict(width=6), dict(width=0), dict(uoff=4), dict(D=10), dict(D=3), dict(R=0), dict(Wp=None)):
        assert rc(**kw) == EINVAL, kw
    untouched(U, Vc)
    assert rc() == 0                                        # the call the rejected ones differ from in one argument
    finite(U[:32], Vc)
    g.intact()


# ---------------------------------------------------------------------------------------------------------------------------
# the weight gradient of the first layer, plain and with the BatchNorm backward formed on load
# ---------------------------------------------------------------------------------------------------------------------------
def run_dw(A, g, form, t, c, nblocks):
    """-> partial [nblocks, C, D + 3] in guards"""
    part = g.fout((nblocks, c["C"], c["D"] + 3))
    tail = (A.ptr(t["idx"]), A.ptr(t["xyz"]), A.ptr(t["ctr"]), A.ptr(t["feat"]), c["B"], c["N"], c["S"], c["K"], c["C"], c["D"], c["feat_first"],
            nblocks, A.ptr(part), A.cur_stream())
    tabs = tuple(A.ptr(t[n]) for n in ("scale", "shift", "ca", "cb", "cd"))
    if form == "dw":
        ok_rc(A, "prifit_sa_first_layer_dw", A.ptr(t["dY"]), *tail)
    elif form == "dw_bn":
        ok_rc(A, "prifit_sa_first_layer_dw_bn", A.ptr(t["G"]), A.ptr(t["Y1"]), *tabs, *tail)
    else:
        ok_rc(A, "prifit_sa_first_layer_dw_bn_gather", A.ptr(t["G"]), A.ptr(t["U"]), A.ptr(t["Vc"]), *tabs, *tail)
    return part


def blocks_with_rows(P, nblocks):
    """every block takes ceil(P / nblocks) rows rounded up to whole chunks of 256: the blocks behind the last row have none"""
    per = -(-(-(-P // nblocks)) // 256) * 256
    return -(-P // per)


@pytest.mark.parametrize("P", sorted(sc.DW_SHAPES))
def test_first_layer_dw_forms_in_guards_against_fp64(A, P):
    rep = bc.Report()
    for tup in [t for t in sc.DW_CASES if t[0] == P]:
        c = sc.dw_case(*tup)
        assert sc.dw_violations(c) == 0
        rows = [sc.grouped_rows(c["xyz"], c["ctr"], c["feat"], c["idx"], c["feat_first"], dt) for dt in (F64, F32)]
        dys = {"dw": [c["G"].to(F64), c["G"]]}
        dys["dw_bn"] = [sc.bn_dy(c["G"], c["Y1"], c["scale"], c["shift"], c["ca"], c["cb"], c["cd"], dt) for dt in (F64, F32)]
        dys["dw_bn_gather"] = dys["dw_bn"]
        g = Bufs()
        t = dict(dY=g.fin(c["G"]), G=g.fin(c["G"]), Y1=g.fin(c["Y1"]), U=g.fin(c["U"]), Vc=g.fin(c["Vc"]), idx=g.iin(c["idx"], c["N"] - 1),
                 xyz=g.fin(poisoned_rows(c["xyz"])), ctr=g.fin(c["ctr"]), feat=g.fin(poisoned_rows(c["feat"])) if c["D"] else None,
                 **{n: g.fin(c[n]) for n in ("scale", "shift", "ca", "cb", "cd")})
        for nblocks in sc.dw_nblocks(P):
            parts = {form: run_dw(A, g, form, t, c, nblocks) for form in ("dw", "dw_bn", "dw_bn_gather")}
            finite(*parts.values())
            g.intact()
            used = blocks_with_rows(P, nblocks)
            for form, part in parts.items():
                assert not bool(part[used:].any()), (form, "surplus blocks write zero partials")
                assert same(part, run_dw(A, g, form, t, c, nblocks))          # a fixed order: the same bits again
                rep.red(form, tup + (nblocks,), part.sum(0), sc.first_layer_dw(dys[form][0], rows[0]),
                        sc.first_layer_dw(dys[form][1], rows[1], F32), sc.first_layer_dw_absum(dys[form][0], rows[0]))
        g.intact()
    rep.assert_bars()


def test_first_layer_dw_rejects_unsupported_arguments(A):
    c = sc.dw_case(255, 16, 3, 1)
    g = Bufs()
    wide = g.fin(torch.zeros(255 * 32 + 4))
    t = dict(idx=g.iin(c["idx"], 0), xyz=g.fin(c["xyz"]), ctr=g.fin(c["ctr"]), feat=g.fin(c["feat"]),
             **{n: g.fin(torch.ones(32)) for n in ("scale", "shift", "ca", "cb", "cd")})
    part = g.fout((2, 32, 7))
    st = A.cur_stream()

    def rc(form, C=16, D=3, off=(0, 0, 0), nblocks=2):
        tail = (A.ptr(t["idx"]), A.ptr(t["xyz"]), A.ptr(t["ctr"]), A.ptr(t["feat"]), c["B"], c["N"], c["S"], c["K"], C, D, 1, nblocks, A.ptr(part), st)
        tabs = tuple(A.ptr(t[n]) for n in ("scale", "shift", "ca", "cb", "cd"))
        a = [A.ptr(wide) + o for o in off]
        if form == "dw":
            return rc_of(A, "prifit_sa_first_layer_dw", a[0], *tail)
        if form == "dw_bn":
            return rc_of(A, "prifit_sa_first_layer_dw_bn", a[0], a[1], *tabs, *tail)
        return rc_of(A, "prifit_sa_first_layer_dw_bn_gather", a[0], a[1], a[2], *tabs, *tail)
    for form in ("dw", "dw_bn", "dw_bn_gather"):
        for kw in (dict(C=24), dict(C=8), dict(C=256), dict(D=4), dict(off=(4, 0, 0)), dict(nblocks=0)):
            assert rc(form, **kw) == EINVAL, (form, kw)
    assert rc("dw_bn", off=(0, 4, 0)) == EINVAL                              # Y1
    assert rc("dw_bn_gather", off=(0, 4, 0)) == EINVAL and rc("dw_bn_gather", off=(0, 0, 8)) == EINVAL          # U, Vc
    untouched(part)
    for form in ("dw", "dw_bn", "dw_bn_gather"):            # the call the rejected ones differ from in one argument
        assert rc(form) == 0, form
        finite(part.view(-1)[:2 * 16 * 6])
    g.intact()


# ---------------------------------------------------------------------------------------------------------------------------
# tables -> front end (gather mode) -> fused-BatchNorm weight gradient, on the kernels' own outputs
# ---------------------------------------------------------------------------------------------------------------------------
def test_chain_tables_front_end_weight_gradient_against_fp64(A):
    rep = bc.Report()
    c = sc.chain_case()
    B, N, S, K, C, D = c["B"], c["N"], c["S"], c["K"], c["C"], c["D"]
    f64, f32 = sc.chain_forward(c), sc.chain_forward(c, F32)
    g = Bufs()
    xd, cd, fd = g.fin(c["xyz"]), g.fin(c["ctr"]), g.fin(c["feat"])
    U, Vc = run_tables(A, g, xd, cd, fd, B, N, S, D, c["feat_first"], [C], [g.fin(c["W"])], [g.fin(c["bias"])])
    Y, slab, idx = run_front(A, g, xd, cd, B, N, S, [c["r2u"] * sc.UNIT2], [K], [C], 1, U=U, Vc=Vc, bias=[None])
    t = dict(G=g.fin(c["G"]), U=U[0], Vc=Vc[0], idx=idx[0], xyz=xd, ctr=cd, feat=fd, **{n: g.fin(c[n]) for n in ("scale", "shift", "ca", "cb", "cd")})
    part = run_dw(A, g, "dw_bn_gather", t, c, 3)
    finite(U[0], Vc[0], Y[0], slab[0], part)
    in_range(N, idx[0])
    g.intact()
    assert same(idx[0], f64["idx"].int())
    rep.ew("chain_U", "chain", U[0], f64["U"], f32["U"])
    rep.ew("chain_Vc", "chain", Vc[0], f64["Vc"], f32["Vc"])
    compare_front(rep, "chain", ("chain",), A, B, S, [K], [C], Y, slab, [f64["Y"]], [f32["Y"]])
    (dw64, absum), (dw32, _) = sc.chain_dw(c, f64), sc.chain_dw(c, f32, F32)
    rep.red("chain_dW", "chain", part.sum(0), dw64, dw32, absum)
    rep.assert_bars()

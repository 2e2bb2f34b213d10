"""The DGCNN graph kernels (csrc/dgcnn.hip, csrc/edge_conv.hip, csrc/pool_alg.hip: neighbour search, edge features, the CSR of
the neighbour lists, the edge-convolution tables forward and backward, the winners' terms of the cloud-wide pool, slab sums)
through the C ABI at edge shapes, every tensor a kernel reads inside NaN guard bands (pad columns of matrices with ld > C
included; index inputs inside an in-range poison), every tensor it writes inside sentinel guards (tests/guard_common.py),
against the float64 restatements of tests/dgcnn_graph_common.py (pinned to torch by tests/test_dgcnn_graph_restatement.py).

Each kernel is fed the float64 reference's upstream results rounded to float32, so an error belongs to one kernel;
test_whole_block_* chains the kernels' own outputs.  Each case asserts, in this order: outputs finite, guards intact, the exact
properties, then the bars: error against float64 at most 4 x the error of the float32 restatement on the same inputs (floored
at 2^-24), element-wise outputs normalised by max |fp64|, reduced outputs element by element by the float64 sum of |terms|.

Path -> case that reaches it:
  knn_select_kernel<64>                      test_knn_topk (4096, 64)          knn_topk_kernel<64>      test_knn_topk (4096, 65)
  round-per-neighbour form, k > 64 / N < 64  test_knn_topk (1, 1), (63, 63), (130, 65), (130, 130)
  edge_csr_kernel, > 1 bin per thread        test_csr (1025, 3075), (8192, 16384: the LDS limit)
  edge_csr_kernel, E < one pass, E % 1024    test_csr (1, 1), (16, 160), (7, 1000), (256, 8193: more than one 8192-entry pass)
  edge_stats / edge_bwd_point, k > 64        test_edge_stats (64, 65 / 70 / 130, ..), (128 / 256, 70, ..); test_edge_bwd (.., 70, ..)
  edge_stats, k % 10 == 0 at C = 128, 256    test_edge_stats (128 / 256, 20 / 70, ..)
  edge_stats at N = 16 (a single slab)       test_edge_stats (.., 16, ..)
  every case of the tables at B = 1 and B = 3 (neighbour search at N > 2048: B = 1 alone); B = 1 is the graph of sample 0
  edge_bwd_gather, in-degree 0 / > 64 / every remainder of the 12-wide batches
                                             test_edge_bwd (.., 70, 16, ..), (.., 20 / 70, 48, ..): in-degrees 0, 1, 11, 12, 13, 63,
                                             64, 65, 76, 77, 130 in sample 0, a hub of N k in-edges in sample 2
  row strides other than C and 2 C           test_edge_stats / _pool / _bwd (pad 4), test_whole_block (2 C + 4)
  edge_gather_rows, ld / 4 not dividing 256  test_edge_gather (4, 3, 24)       ld = 1024   test_edge_gather (128, 5, 1024)
  scalar edge_gather_kernel                  test_edge_gather (3, 20, 8), (6, 7, 12), (5, 1, 11), (128, 2, 1028)
  edge_scatter_kernel (k < 4)                test_edge_scatter (.., 1 / 3, ..)
  global_pool_winners off the network shape  test_global_pool_winners, every case
  slab_sum, both loops                       test_slab_sum, nslab 1 .. 1000

Measured on an MI355X (per quantity the case with the largest ratio: kernel error, float32 restatement's error, their ratio
with the restatement's error floored at 2^-24, the case -- the last entry of a case tuple is B; the bar is a ratio of 4; the
block_* rows are the chained tests):

  quantity           kernel   fp32     ratio   case
  scatter_dx         1.2e-07  7.2e-08   1.62   (3, 1, 0, False, 3)
  stats_ysum         2.6e-07  2.1e-07   1.23   (64, 130, 48, 1, 4, 1)
  stats_slab_s       9.5e-08  7.9e-08   1.19   (64, 130, 48, 1, 4, 1)
  stats_slab_q       1.2e-07  1.3e-07   0.93   (64, 65, 16, 0, 4, 1)
  pool_out           4.7e-08  5.5e-08   0.79   (64, 5, 4, 0.0, 3)
  bwd_dVc            1.3e-07  1.7e-07   0.75   (128, 70, 16, 0, 0, 0, 1)
  bwd_dU             1.2e-07  1.7e-07   0.67   (64, 7, 48, 1, 0, 4, 1)
  block_scale        6.5e-08  6.5e-08   1.00   chain(64)
  block_shift        4.5e-08  4.0e-08   0.75   chain(64)
  block_mean         3.5e-08  3.5e-08   0.59   chain(64)
  block_invstd       3.8e-08  3.8e-08   0.64   chain(64)
  block_out          8.9e-08  8.9e-08   1.00   chain(64)
  block_cb           2.1e-07  1.5e-07   1.37   chain(256)
  block_cd           5.3e-08  1.1e-07   0.47   chain(128)
  block_dgamma       1.3e-07  1.5e-07   0.90   chain(256)
  block_dbeta        7.5e-08  9.0e-08   0.84   chain(128)
  block_dU           4.0e-07  6.2e-07   0.64   chain(64)
  block_dVb          6.0e-07  5.7e-07   1.06   chain(128)
  winners_dX         1.1e-07  9.6e-08   1.12   (1, 1, 64, 64, False, 'dX', 0, 4, 4, 0)
  winners_dW         8.9e-08  8.9e-08   1.00   (1, 1, 64, 64, False, 'dW', 4, 0, 0, 4)
  slab_sum           8.2e-08  5.8e-08   1.38   (57, 384)

Largest difference between two runs of the outputs that are not asserted to repeat, in the unit of the bars (edge_scatter adds
with float atomics in arrival order; edge_bwd sums dU over a CSR list, whose order is not fixed, in float64):

  quantity           largest   case
  scatter_dx         2.1e-07   (64, 3, 4, False, 3)
  bwd_dU             0.0e+00   (64, 7, 16, 0, 0, 0, 1)

Defects these tests found:
- edge_bwd_point_kernel looked up the winner's neighbour with `w < 64 ? __shfl(nl, w) : ix[w]`.  With k > 64 the lanes whose own
  winner sits at a position >= 64 are switched off while the shuffle runs, and a lane that reads one of them receives 0, an
  in-range index: a winner that is an out-of-range entry (a zero row, no gradient) then put its a T into dVc, and through the
  self term into dU.  Before: bwd_dVc 0.10 .. 8.5 and bwd_dU 0.08 .. 4.5 (in units of the sum of |terms|) at every k = 70 case.
  Now the shuffle runs outside the select: the ratios above.
- edge_stats_kernel added a point's k values of y in one chain and the squares of a wave's four points in one chain of 4 k.
  Before: stats_slab_q 9.1e-07 against 2.1e-07 (ratio 4.3) at k = 20, 3.9e-06 against 2.7e-07 (14) at k = 70 and 7.0e-06
  against 3.0e-07 (24) at k = 130; stats_ysum 2.0e-06 against 4.0e-07 (4.9) and stats_slab_s 9.7e-07 against 2.3e-07 (4.3) at
  k = 130.  Now a pairwise tree over the slots of a batch and one chain over a point's batches: the ratios above.
Nothing else was found: no guard word was touched, every index list, CSR and winner is exact, and every kernel that is
asserted to repeat its bits does.

What these tests cannot see: a stray read whose value is discarded (the clamped loads of dead unroll slots in edge_stats_kernel
and edge_bwd_gather_kernel read row 0 of the shape, in range), as in tests/test_gpu_norm_pool_guards.py.
"""
import ctypes

import pytest
import torch

import bn_common as bc
import dgcnn_graph_common as gc
from bn_common import F32, F64
from guard_common import SENTINEL, Bufs, poison_bits

pytestmark = pytest.mark.gpu

LL = ctypes.c_longlong
EINVAL = -1


@pytest.fixture(scope="module")
def A(hiplib):
    assert torch.cuda.is_available()
    from prifit_amd import _lib
    return _lib


def rc_of(A, name, *args):
    return getattr(A.dll(), name)(*args)


def finite(*ts):
    torch.cuda.synchronize()
    for t in ts:
        assert bool(torch.isfinite(t).all()), "non-finite output"


def same(a, b):
    return torch.equal(a.cpu(), b.cpu())


def rerun_diff(a, b, absum):
    """largest difference between two runs, in the unit of the red bars"""
    return bc.red_err(a, b.to("cpu", F64), absum)


# ---------------------------------------------------------------------------------------------------------------------------
# neighbour search
# ---------------------------------------------------------------------------------------------------------------------------
def _knn_expected(x, k):
    """float64 stable sort on the lattice (exact values: the device the sort runs on does not matter)"""
    G, xx = gc.gram(x.cuda() if x.shape[1] > 512 else x)
    return G, xx, gc.knn_ref(G, xx, k).cpu()


@pytest.mark.parametrize("N,k", gc.KNN_TOPK_CASES)
def test_knn_topk_in_guards_bit_for_bit(A, N, k):
    for B in gc.knn_Bs(N):
        for kind in gc.KNN_KINDS:
            x = gc.knn_cloud(kind, B, N, bc.gen_of(bc.seed_of(31, N, k, B)))
            G, xx, want = _knn_expected(x, k)
            g = Bufs()
            Gd, xd, out = g.fin(G), g.fin(xx), g.iout((B, N, k))
            A.call("prifit_knn_topk", A.ptr(Gd), A.ptr(xd), B, N, k, A.ptr(out), A.cur_stream())
            g.intact()
            assert same(out, want), (kind, N, k, B)
            if kind == "same":
                assert same(out, torch.arange(k, dtype=torch.int32).expand(B, N, k))


@pytest.mark.parametrize("N,k", gc.KNN3_CASES)
def test_knn3_topk_in_guards_bit_for_bit(A, N, k):
    for B in (1, 3):
        for kind in gc.KNN_KINDS:
            x = gc.knn_cloud(kind, B, N, bc.gen_of(bc.seed_of(31, N, k, B)))
            _, _, want = _knn_expected(x, k)
            g = Bufs()
            xd, out = g.fin(x), g.iout((B, N, k))
            A.call("prifit_knn3_topk", A.ptr(xd), B, N, k, A.ptr(out), A.cur_stream())
            g.intact()
            assert same(out, want), (kind, N, k, B)


def test_knn3_equals_the_product_route_on_a_ragged_cloud_off_the_lattice(A, monkeypatch):
    from prifit_amd.src import dgcnn as D
    B, N, k = 3, 997, 20
    x = torch.randn(B, N, 3, generator=bc.gen_of(32)).to(F32)
    g = Bufs()
    xd, out = g.fin(x), g.iout((B, N, k))
    A.call("prifit_knn3_topk", A.ptr(xd), B, N, k, A.ptr(out), A.cur_stream())
    g.intact()
    monkeypatch.setattr(D, "_KNN3_FUSED", False)
    assert same(out, D._knn_cl(x.cuda(), k))


def test_knn_rejects_unsupported_shapes(A):
    g = Bufs()
    G, xx, x, out = g.fin(torch.zeros(64, 64)), g.fin(torch.zeros(64)), g.fin(torch.zeros(64, 3)), g.iout((64, 64))
    st = A.cur_stream()
    assert rc_of(A, "prifit_knn_topk", A.ptr(G), A.ptr(xx), 1, 8, 9, A.ptr(out), st) == EINVAL          # k > N
    assert rc_of(A, "prifit_knn_topk", A.ptr(G), A.ptr(xx), 1, 4097, 4, A.ptr(out), st) == EINVAL       # N > 4096
    for N, k in ((63, 4), (2049, 4), (64, 65), (64, 0)):
        assert A.query("prifit_knn3_supported", N, k) == 0
        assert rc_of(A, "prifit_knn3_topk", A.ptr(x), 1, N, k, A.ptr(out), st) == EINVAL
    assert A.query("prifit_knn3_supported", 64, 64) == 1 and A.query("prifit_knn3_supported", 2048, 1) == 1
    g.intact()


# ---------------------------------------------------------------------------------------------------------------------------
# edge features
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,k,ld", gc.GATHER_VECTOR_CASES + gc.GATHER_SCALAR_CASES)
def test_edge_gather_in_guards_bit_for_bit(A, C, k, ld):
    for B in (1, 3):
        case = gc.gather_case(C, k, ld, B=B)
        N = gc.GATHER_N
        g = Bufs()
        x, idx, out = g.fin(case["x"]), g.iin(case["idx"], N - 1), g.fout((B * N * k, ld))
        A.call("prifit_edge_gather", A.ptr(x), A.ptr(idx), B, N, C, k, ld, A.ptr(out), A.cur_stream())
        finite(out)
        g.intact()
        want = gc.edge_feature(case["x"], case["idx"], ld, F32).view(B * N * k, ld)
        assert same(out, want)
        assert not bool(out[:, 2 * C:].any())


@pytest.mark.parametrize("C,k,pad,hub", gc.SCATTER_CASES)
def test_edge_scatter_in_guards_against_fp64(A, C, k, pad, hub):
    rep = bc.Report()
    for B in (1, 3):
        case = gc.scatter_case(C, k, pad, hub, B=B)
        N = gc.GATHER_N
        g = Bufs()
        gout = g.fin(case["gout"].view(B * N * k, 2 * C), 2 * C + pad)
        idx = g.iin(case["idx"], N - 1)
        dx, dx2 = g.fout((B, N, C), init=case["dx0"]), g.fout((B, N, C), init=case["dx0"])
        for d in (dx, dx2):
            A.call("prifit_edge_scatter", A.ptr(gout), gout.stride(0), A.ptr(idx), B, N, C, k, A.ptr(d), A.cur_stream())
        finite(dx)
        g.intact()
        absum = gc.edge_scatter_absum(case["gout"], case["idx"], case["dx0"], C)
        rep.red("scatter_dx", (C, k, pad, hub, B), dx, gc.edge_scatter(case["gout"], case["idx"], case["dx0"], C),
                gc.edge_scatter(case["gout"], case["idx"], case["dx0"], C, F32), absum)
        print("RERUN scatter_dx %s %.3e" % ((C, k, pad, hub, B), rerun_diff(dx, dx2, absum)))
    rep.assert_bars()


# ---------------------------------------------------------------------------------------------------------------------------
# CSR of the neighbour lists
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins,E", gc.CSR_CASES)
def test_csr_in_guards_exactly(A, nbins, E):
    for kind in gc.CSR_GRAPHS:
        for B in (1, 3):
            idx = gc.csr_graph(kind, B, nbins, E, bc.gen_of(bc.seed_of(33, nbins, E, B)))
            as_edges = E % nbins == 0 and kind != "hub"            # also through prifit_edge_csr (N = nbins, k = E / nbins)
            g = Bufs()
            ix = g.iin(idx, nbins // 2)
            offs, lst, pos, owner = g.iout((B, nbins + 1)), g.iout((B, E)), g.iout((B, E)), g.iout((B, E))
            A.call("prifit_list_csr", A.ptr(ix), B, nbins, E, A.ptr(offs), A.ptr(lst), A.ptr(pos), A.ptr(owner), A.cur_stream())
            outs = [(offs, lst, pos, owner)]
            if as_edges:
                o2, l2, p2 = g.iout((B, nbins + 1)), g.iout((B, E)), g.iout((B, E))
                A.call("prifit_edge_csr", A.ptr(ix), B, nbins, E // nbins, A.ptr(o2), A.ptr(l2), A.ptr(p2), A.cur_stream())
                outs.append((o2, l2, p2, None))
            torch.cuda.synchronize()
            g.intact()
            for o, l, p, w in outs:
                o, l, p = o.cpu().long(), l.cpu().long(), p.cpu().long()
                for b in range(B):
                    want = gc.csr_offsets(idx[b], nbins)
                    assert torch.equal(o[b], want)
                    total = int(want[-1])
                    ok = (idx[b] >= 0) & (idx[b] < nbins)
                    e = ok.nonzero().squeeze(1)
                    assert bool((p[b][~ok] == -1).all())
                    pe = p[b][e]
                    bins = idx[b][e].long()
                    assert bool((pe >= want[bins]).all()) and bool((pe < want[bins + 1]).all())
                    assert torch.equal(pe.sort().values, torch.arange(total))          # every list position taken once: sets
                    assert torch.equal(l[b][pe], e)
                    assert bool((l[b][total:] == poison_bits(SENTINEL)).all())
                    if w is not None:
                        wc = w.cpu().long()[b]
                        assert torch.equal(wc[pe], bins)
                        assert bool((wc[total:] == poison_bits(SENTINEL)).all())


def test_csr_rejects_more_bins_than_the_histogram_holds(A):
    g = Bufs()
    ix, out = g.iin(torch.zeros(1, 8193, dtype=torch.int32), 0), g.iout((4, 8194))
    st = A.cur_stream()
    assert rc_of(A, "prifit_list_csr", A.ptr(ix), 1, 8193, 8193, A.ptr(out[0]), A.ptr(out[1]), A.ptr(out[2]), None, st) == EINVAL
    assert rc_of(A, "prifit_edge_csr", A.ptr(ix), 1, 8193, 1, A.ptr(out[0]), A.ptr(out[1]), A.ptr(out[2]), st) == EINVAL
    g.intact()


# ---------------------------------------------------------------------------------------------------------------------------
# edge-convolution tables
# ---------------------------------------------------------------------------------------------------------------------------
def operands_in(g, case, pad):
    """U and the second operand in guards: the halves of one [B N, 2 C (+ pad)] matrix (selfterm) or two matrices of different
    row strides.  -> U, V2, ldu, ldv"""
    B, N, C = case["U"].shape
    if case["selfterm"]:
        UV = g.fin(torch.cat([case["U"], case["V2"]], 2).view(B * N, 2 * C), 2 * C + pad)
        return UV[:, :C], UV[:, C:], UV.stride(0), UV.stride(0)
    U, V2 = g.fin(case["U"].view(B * N, C), C + pad), g.fin(case["V2"].view(B * N, C), C + 4 - pad)
    return U, V2, U.stride(0), V2.stride(0)


def run_stats(A, g, case, U, V2, ldu, ldv, idx):
    B, N, C, k = case["B"], case["N"], case["C"], case["k"]
    o = dict(ymax=g.fout((B * N, C)), ymin=g.fout((B * N, C)), karg=g.iout((B * N, C)), ysum=g.fout((B * N, C)),
             vct=g.fout((B * N, C)), slab=g.fout((B * N // gc.EC_PTS, 2, C)))
    A.call("prifit_edge_stats", A.ptr(U), LL(ldu), A.ptr(V2), LL(ldv), case["selfterm"], A.ptr(idx), B, N, k, C, A.ptr(o["ymax"]),
           A.ptr(o["ymin"]), A.ptr(o["karg"]), A.ptr(o["ysum"]), A.ptr(o["vct"]), A.ptr(o["slab"]), A.cur_stream())
    return o


@pytest.mark.parametrize("C", sorted({c[0] for c in gc.STATS_CASES}))
def test_edge_stats_in_guards_against_fp64(A, C):
    assert A.query("prifit_edge_points_per_slab") == gc.EC_PTS
    rep = bc.Report()
    for c in [c + (B,) for c in gc.STATS_CASES if c[0] == C for B in gc.EDGE_BS]:
        _, k, N, selfterm, pad, B = c
        case = gc.edge_case(C, k, N, selfterm, B=B)
        g = Bufs()
        U, V2, ldu, ldv = operands_in(g, case, pad)
        idx = g.iin(case["idx"], 0)
        o, o2 = run_stats(A, g, case, U, V2, ldu, ldv, idx), run_stats(A, g, case, U, V2, ldu, ldv, idx)
        finite(o["ymax"], o["ymin"], o["ysum"], o["vct"], o["slab"])
        g.intact()
        r64, r32 = gc.edge_stats(case["U"], case["V2"], case["idx"], selfterm), gc.edge_stats(case["U"], case["V2"], case["idx"], selfterm, F32)
        for n in ("ymax", "ymin", "vct", "karg"):
            assert same(o[n].view(B, N, C), r32[n]), (n, c)
        if B > 1:                                            # the point without a valid neighbour: nothing was added at all
            assert bool(((case["idx"][1, 1] < 0) | (case["idx"][1, 1] >= N)).all())
            assert not bool(o["ysum"].view(B, N, C)[1, 1].any()) and not bool(o["ymax"].view(B, N, C)[1, 1].any())
        kg = o["karg"].cpu().view(B, N, C)
        assert torch.equal(kg & 1023, r64["kx"].int()) and torch.equal((kg >> 10) & 1023, r64["kn"].int())
        assert torch.equal(kg >> 20, r64["nv"].int())
        for n in o:
            assert same(o[n], o2[n]), n
        y = r64["y"]
        rep.red("stats_ysum", c, o["ysum"].view(B, N, C), r64["ysum"], r32["ysum"], y.abs().sum(2))
        ys = y.reshape(B * N // gc.EC_PTS, gc.EC_PTS * k, C)
        ab = torch.stack([ys.abs().sum(1), (ys * ys).sum(1)], 1)
        for h, name in enumerate(("stats_slab_s", "stats_slab_q")):
            rep.red(name, c, o["slab"][:, h], r64["slab"][:, h], r32["slab"][:, h], ab[:, h])
    rep.assert_bars()


@pytest.mark.parametrize("C,N,pad,slope", gc.POOL_CASES)
def test_edge_pool_in_guards_against_fp64(A, C, N, pad, slope):
    rep = bc.Report()
    for B in (1, 3):
        case = gc.pool_case(C, N, slope, B=B)
        g = Bufs()
        ymax, ymin = g.fin(case["ymax"].view(B * N, C)), g.fin(case["ymin"].view(B * N, C))
        sc, sh = g.fin(case["scale"]), g.fin(case["shift"])
        out, ystar = g.mout(B * N, C, C + pad, 0, C + pad), g.fout((B * N, C))
        A.call("prifit_edge_pool", A.ptr(ymax), A.ptr(ymin), A.ptr(sc), A.ptr(sh), B, N, C, slope, A.ptr(out), LL(out.stride(0)),
               A.ptr(ystar), A.cur_stream())
        finite(out, ystar)
        g.intact()
        o64, y64, _ = gc.edge_pool(case["ymax"], case["ymin"], case["scale"], case["shift"], slope)
        o32, y32, _ = gc.edge_pool(case["ymax"], case["ymin"], case["scale"], case["shift"], slope, F32)
        assert same(ystar.view(B, N, C), y32)
        neg = (case["scale"] < 0).unsqueeze(1).expand(B, N, C)
        ys = ystar.cpu().view(B, N, C)
        assert torch.equal(ys[neg], case["ymin"][neg]) and torch.equal(ys[~neg], case["ymax"][~neg])
        assert bool((case["scale"][:, 1] == 0).all()) and bool(torch.signbit(case["scale"][:, 2]).all()) and not bool(neg[:, :, 2].any())
        rep.ew("pool_out", (C, N, pad, slope, B), out.reshape(B, N, C), o64, o32)
    rep.assert_bars()


def test_edge_pool_rejects_misaligned_and_ragged_arguments(A):
    g = Bufs()
    t, out = g.fin(torch.zeros(8, 8)), g.fout((8, 16))
    st = A.cur_stream()

    def rc(C, ldo, o):
        return rc_of(A, "prifit_edge_pool", A.ptr(t), A.ptr(t), A.ptr(t), A.ptr(t), 1, 2, C, 0.0, o, LL(ldo), A.ptr(out[4:]), st)
    assert rc(4, 4, A.ptr(out) + 4) == EINVAL
    assert rc(6, 8, A.ptr(out)) == EINVAL
    assert rc(4, 6, A.ptr(out)) == EINVAL
    g.intact()


def random_csr(idx, N, gen):
    """offs [B, N + 1], lst, pos [B, N k] of the neighbour lists, every list in a random order"""
    B = idx.shape[0]
    E = idx[0].numel()
    offs, lst, pos = torch.zeros(B, N + 1, dtype=torch.int32), torch.zeros(B, E, dtype=torch.int32), torch.full((B, E), -1, dtype=torch.int32)
    for b in range(B):
        flat = idx[b].reshape(-1).long()
        ok = (flat >= 0) & (flat < N)
        offs[b] = gc.csr_offsets(flat, N).int()
        e = ok.nonzero().squeeze(1)
        order = e[torch.argsort(flat[e] * E + torch.randperm(e.numel(), generator=gen))]
        lst[b, :order.numel()] = order.int()
        pos[b, order] = torch.arange(order.numel(), dtype=torch.int32)
    return offs, lst, pos


def bwd_reference(case, dtype):
    st = gc.edge_stats(case["U"], case["V2"], case["idx"], case["selfterm"], dtype)
    _, ystar, _ = gc.edge_pool(st["ymax"], st["ymin"], case["scale"], case["shift"], case["slope"], dtype)
    T = gc.edge_T(case["gp"], ystar, case["scale"], case["shift"], case["slope"], dtype)
    win = gc.winners(st["kx"], st["kn"], case["scale"])
    dU, dV = gc.edge_bwd(case["U"], case["V2"], case["idx"], case["selfterm"], win, T, case["ca"], case["cb"], case["cd"], dtype)
    return dict(st=st, ystar=ystar, T=T, win=win, dU=dU, dV=dV)


def run_bwd(A, g, case, tabs, ldd_pad):
    """-> dU, dV (the kernel's second output: dVc, or dVb with selfterm), both [B N, C] views"""
    B, N, C, k = case["B"], case["N"], case["C"], case["k"]
    P = B * N
    if case["selfterm"]:
        both = g.mout(P, 2 * C, 2 * C + ldd_pad, 0, 2 * C + ldd_pad)
        dU, dV = both[:, :C], both[:, C:]
    else:
        dU, dV = g.mout(P, C, C + ldd_pad, 0, C + ldd_pad), g.mout(P, C, C + ldd_pad, 0, C + ldd_pad)
    ws = g.fout((A.query("prifit_edge_bwd_workspace", B, N, k, C) // 4,))
    A.call("prifit_edge_bwd", A.ptr(tabs["gp"]), LL(tabs["gp"].stride(0)), A.ptr(tabs["ystar"]), A.ptr(tabs["ysum"]), A.ptr(tabs["karg"]),
           A.ptr(tabs["scale"]), A.ptr(tabs["shift"]), A.ptr(tabs["ca"]), A.ptr(tabs["cb"]), A.ptr(tabs["cd"]), A.ptr(tabs["U"]),
           LL(tabs["U"].stride(0)), A.ptr(tabs["vct"]), case["selfterm"], A.ptr(tabs["idx"]), A.ptr(tabs["offs"]), A.ptr(tabs["lst"]),
           A.ptr(tabs["pos"]), B, N, k, C, case["slope"], A.ptr(dU), A.ptr(dV), LL(dU.stride(0)), A.ptr(ws), A.cur_stream())
    return dU, dV


@pytest.mark.parametrize("C", sorted({c[0] for c in gc.BWD_CASES}))
def test_edge_bwd_in_guards_against_fp64(A, C):
    rep = bc.Report()
    for c in [c + (B,) for c in gc.BWD_CASES if c[0] == C for B in gc.EDGE_BS]:
        _, k, N, selfterm, ldd_pad, ldgp_pad, B = c
        case = gc.edge_case(C, k, N, selfterm, B=B, degrees=True)
        P = B * N
        r64, r32 = bwd_reference(case, F64), bwd_reference(case, F32)
        st = r64["st"]
        offs, lst, pos = random_csr(case["idx"], N, bc.gen_of(bc.seed_of(34, C, k, N, B)))
        g = Bufs()
        tabs = dict(gp=g.fin(case["gp"].view(P, C), C + ldgp_pad), ystar=g.fin(r64["ystar"].view(P, C)), ysum=g.fin(st["ysum"].view(P, C)),
                    karg=g.iin(st["karg"].view(P, C), 0), vct=g.fin(st["vct"].view(P, C)), U=g.fin(case["U"].view(P, C), C + 4),
                    idx=g.iin(case["idx"], 0), offs=g.iin(offs, 0), lst=g.iin(lst, 0), pos=g.iin(pos, 0),
                    **{n: g.fin(case[n]) for n in ("scale", "shift", "ca", "cb", "cd")})
        (dU, dV), (dU2, dV2) = run_bwd(A, g, case, tabs, ldd_pad), run_bwd(A, g, case, tabs, ldd_pad)
        finite(dU, dV)
        g.intact()
        deg0 = (gc.in_degrees(case["idx"], N) == 0).view(P)
        assert bool(deg0.any()) or N * k < sum(gc.DEGREES)
        du, dv = dU.cpu(), dV.cpu()
        if selfterm:
            assert torch.equal(du[deg0], -dv[deg0])           # the point's own dVc = -dVb and nothing else
        else:
            assert not bool(du[deg0].any())
        assert same(dV, dV2)
        absU, absV = gc.edge_bwd_absum(case["U"], case["V2"], case["idx"], selfterm, r64["win"], r64["T"], case["ca"], case["cb"], case["cd"])
        rep.red("bwd_dVc", c, dV.reshape(B, N, C), r64["dV"], r32["dV"], absV)
        rep.red("bwd_dU", c, dU.reshape(B, N, C), r64["dU"], r32["dU"], absU)
        print("RERUN bwd_dU %s %.3e" % (c, rerun_diff(dU.reshape(B, N, C), dU2.reshape(B, N, C), absU)))
    rep.assert_bars()


@pytest.mark.parametrize("C", gc.CHAIN_C)
def test_whole_block_on_the_kernels_own_outputs_against_fp64(A, C):
    """stats -> prifit_gn_finalize -> pool -> (prifit_bn_relu_bwd_reduce over the winners' table) -> prifit_gn_bwd_finalize ->
    CSR -> bwd, stacked operands with row stride 2 C + 4, against the torch-anchored float64 chain"""
    rep = bc.Report()
    case = gc.chain_case(C)
    B, N, k, groups, slope = case["B"], case["N"], case["k"], case["groups"], case["slope"]
    P, E = B * N, N * k
    count = float(N * k * (C // groups))
    st_ = A.cur_stream()
    g = Bufs()
    U, V2, ldu, ldv = operands_in(g, case, 4)
    idx = g.iin(case["idx"], 0)
    gamma, beta, gout = g.fin(case["gamma"]), g.fin(case["beta"]), g.fin(case["gout"].view(P, C), C + 4)
    o = run_stats(A, g, case, U, V2, ldu, ldv, idx)
    sc, sh, mu, isd = (g.fout((B, C)) for _ in range(4))
    A.call("prifit_gn_finalize", A.ptr(o["slab"]), B, N // gc.EC_PTS, C, groups, count, A.ptr(gamma), A.ptr(beta), gc.GN_EPS, A.ptr(sc),
           A.ptr(sh), A.ptr(mu), A.ptr(isd), None, st_)
    out, ystar = g.fout((P, C)), g.fout((P, C))
    A.call("prifit_edge_pool", A.ptr(o["ymax"]), A.ptr(o["ymin"]), A.ptr(sc), A.ptr(sh), B, N, C, slope, A.ptr(out), LL(C), A.ptr(ystar), st_)
    assert N == bc.RED_ROWS                                  # one backward slab per sample
    bslab = g.fout((B, 2, C))
    A.call("prifit_bn_relu_bwd_reduce", A.ptr(gout), LL(gout.stride(0)), A.ptr(ystar), LL(C), A.ptr(sc), A.ptr(sh), A.ptr(mu), A.ptr(isd),
           P, C, N, slope, A.ptr(bslab), st_)
    cb, cd, S = g.fout((B, C)), g.fout((B, C)), g.dout((B, 2, C))
    A.call("prifit_gn_bwd_finalize", A.ptr(bslab), B, 1, C, groups, count, A.ptr(gamma), A.ptr(mu), A.ptr(isd), A.ptr(cb), A.ptr(cd),
           A.ptr(S), None, float(N), None, st_)
    offs, lst, pos = g.iout((B, N + 1)), g.iout((B, E)), g.iout((B, E))
    A.call("prifit_edge_csr", A.ptr(idx), B, N, k, A.ptr(offs), A.ptr(lst), A.ptr(pos), st_)
    tabs = dict(gp=gout, ystar=ystar, ysum=o["ysum"], karg=o["karg"], vct=o["vct"], U=U, idx=idx, offs=offs, lst=lst, pos=pos,
                scale=sc, shift=sh, ca=sc, cb=cb, cd=cd)
    dU, dV = run_bwd(A, g, case, tabs, 4)
    finite(out, ystar, sc, sh, mu, isd, cb, cd, S, dU, dV)
    g.intact()
    f64, f32 = gc.chain_forward(case), gc.chain_forward(case, F32)
    g64, g32 = gc.chain_backward(case, f64), gc.chain_backward(case, f32, F32)
    assert same(o["karg"].view(B, N, C), f64["st"]["karg"]) and same(ystar.view(B, N, C), f64["ystar"].to(F32))
    tag = "chain(%d)" % C
    for n, t in (("scale", sc), ("shift", sh), ("mean", mu), ("invstd", isd)):
        rep.ew("block_" + n, tag, t, f64["fin"][n], f32["fin"][n])
    rep.ew("block_out", tag, out.view(B, N, C), f64["out"], f32["out"])
    rep.ew("block_cb", tag, cb, g64["cb"], g32["cb"])
    rep.ew("block_cd", tag, cd, g64["cd"], g32["cd"])
    Sc = S.cpu()
    rep.ew("block_dgamma", tag, Sc[:, 1].sum(0), g64["dgamma"], g32["dgamma"])
    rep.ew("block_dbeta", tag, Sc[:, 0].sum(0), g64["dbeta"], g32["dbeta"])
    absU, absV = gc.edge_bwd_absum(case["U"], case["V2"], case["idx"], 1, f64["win"], g64["T"], f64["fin"]["scale"], g64["cb"], g64["cd"])
    rep.red("block_dU", tag, dU.reshape(B, N, C), g64["dU"], g32["dU"], absU)
    rep.red("block_dVb", tag, dV.reshape(B, N, C), g64["dV"], g32["dV"], absV)
    rep.assert_bars()


# ---------------------------------------------------------------------------------------------------------------------------
# the winners' terms of the cloud-wide pool, slab sums
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bs,K,Cout,Cin,one_row", [c + (False,) for c in gc.WINNERS_CASES] + [(3, 65, 128, 256, True)])
def test_global_pool_winners_in_guards_against_fp64(A, Bs, K, Cout, Cin, one_row):
    rep = bc.Report()
    case = gc.winners_case(Bs, K, Cout, Cin, one_row)
    assert A.query("prifit_global_pool_winners_supported", Cout, Cin) == 1
    if one_row:
        assert bool((case["arg"][0] == K // 2).all()) and bool((case["T"][0] != 0).all())
    r64, r32 = (gc.winners_terms(case["arg"], case["T"], case["W"], case["X"], K, dt) for dt in (F64, F32))
    S = gc.winners_S(case["arg"], case["T"], K).abs()
    absX = case["dX0"].to(F64).abs() + (S @ case["W"].to(F64).abs()).view(Bs * K, Cin)
    absW = case["dW0"].to(F64).abs() + torch.einsum("bkc,bki->ci", S, case["X"].to(F64).abs().view(Bs, K, Cin))
    won = (S.sum(2) > 0).view(Bs * K)
    assert bool((case["T"] == 0).any()) and bool(((case["arg"] < 0) | (case["arg"] >= K)).any())
    for mode, (pw, px, pdx, pdw) in (("dX", (0, 4, 4, 0)), ("dW", (4, 0, 0, 4)), ("both", (4, 4, 0, 0)), ("both", (0, 0, 4, 4))):
        g = Bufs()
        arg, T = g.iin(case["arg"], K // 2), g.fin(case["T"])
        W, X = g.fin(case["W"], Cin + pw), g.fin(case["X"], Cin + px)
        runs = []
        for _ in range(2):
            dX = dW = None
            if mode != "dW":
                dX = g.mout(Bs * K, Cin, Cin + pdx, 0, Cin + pdx)
                dX.copy_(case["dX0"])
            if mode != "dX":
                dW = g.mout(Cout, Cin, Cin + pdw, 0, Cin + pdw)
                dW.copy_(case["dW0"])
            A.call("prifit_global_pool_winners_f32", Bs, K, Cout, Cin, A.ptr(arg), A.ptr(T), A.ptr(W), LL(W.stride(0)), A.ptr(X),
                   LL(X.stride(0)), A.ptr(dX), LL(Cin + pdx), A.ptr(dW), LL(Cin + pdw), A.cur_stream())
            runs.append((dX, dW))
        (dX, dW), (dX2, dW2) = runs
        finite(*[t for t in (dX, dW) if t is not None])
        g.intact()
        tag = (Bs, K, Cout, Cin, one_row, mode, pw, px, pdx, pdw)
        if dX is not None:
            assert same(dX, dX2)
            assert torch.equal(dX.cpu()[~won], case["dX0"][~won])
            rep.red("winners_dX", tag, dX, case["dX0"].to(F64) + r64[0], case["dX0"] + r32[0], absX)
        if dW is not None:
            assert same(dW, dW2)
            rep.red("winners_dW", tag, dW, case["dW0"].to(F64) + r64[1], case["dW0"] + r32[1], absW)
    rep.assert_bars()


@pytest.mark.parametrize("n", gc.SLAB_SUM_N)
def test_slab_sum_in_guards_against_fp64(A, n):
    rep = bc.Report()
    gen = bc.gen_of(35 + n)
    for nslab in gc.SLAB_SUM_NSLAB + (-57,):
        part = torch.randn(abs(nslab), n, generator=gen).to(F32)
        if nslab < 0:                                         # all slabs equal
            nslab = -nslab
            part = part[:1].expand(nslab, n).contiguous()
        g = Bufs()
        pd, out, out2 = g.fin(part), g.fout((n,)), g.fout((n,))
        for o in (out, out2):
            A.call("prifit_slab_sum", A.ptr(pd), nslab, LL(n), A.ptr(o), A.cur_stream())
        finite(out)
        g.intact()
        assert same(out, out2)
        rep.red("slab_sum", (nslab, n), out, gc.slab_sum(part), gc.slab_sum(part, F32), part.to(F64).abs().sum(0))
    rep.assert_bars()

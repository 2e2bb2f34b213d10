"""The point-set Chamfer op (csrc/chamfer.hip, fit_ops.ChamferNNFn, src/utils.py chamfer_distance*) on the GPU.

Kernel level: d2, idx, ga and gb are compared BIT FOR BIT with the numpy restatement of tests/chamfer_common.py (fp32, the
documented operation order, first minimum, gb summed in ascending query order), on ragged batches whose sizes cross every
edge the kernels have: the 256-query block, the 256-target LDS tile, the split of the target range over workgroups (taken
from NB >= 1024 at these batch sizes: (257, 1031) runs 4 ranges of 258, (300, 5003) 16 ranges of 313), the 64-index ballot
step and the 1024-row LDS tile of the backward (NA = 1000 is below it, the (1100, 70) case above).

Public functions: against the fp64 matrix form and against values recorded from the reference itself
(tests/golden/chamfer_pointsets.npz, tools/make_golden_chamfer.py), within the derived rounding bound
(n + 8) * 2^-24 * m of chamfer_common.mean_bound / grad_bound -- nothing here is a measured tolerance."""

import numpy as np
import pytest
import torch

import chamfer_common as cc
from guard_common import SENTINEL, assert_guards_intact, guarded, guarded_like, x_tail

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 257), (63, 3), (65, 255), (257, 1031), (1000, 64), (300, 5003), (1100, 70)]
FAMILIES = ("normal", "lattice")
_cache = {}


def case(family, NA, NB):
    """inputs + restatement of one case, computed once: B = 4 ragged shapes, one without queries, one without targets"""
    key = (family, NA, NB)
    if key not in _cache:
        rng = np.random.default_rng(1000 * NA + NB + (7 if family == "lattice" else 0))
        B = 4
        if family == "normal":
            a = rng.standard_normal((B, NA, 3)).astype(np.float32)
            b = rng.standard_normal((B, NB, 3)).astype(np.float32)
        else:
            a, b = cc.lattice(rng, (B, NA, 3)), cc.lattice(rng, (B, NB, 3))
        g = rng.standard_normal((B, NA)).astype(np.float32)
        na = np.array([NA, NA // 2 + 1, 0, NA], np.int32)
        nb = np.array([NB, 1, NB, 0], np.int32)
        d2, idx, ties = cc.nn_ref(a, b, na, nb)
        ga, gb = cc.bwd_ref(a, b, na, nb, idx, g)
        for arr in (a, b, g, na, nb, d2, idx, ties, ga, gb):
            arr.setflags(write=False)
        _cache[key] = dict(a=a, b=b, g=g, na=na, nb=nb, d2=d2, idx=idx, ties=ties, ga=ga, gb=gb)
    return _cache[key]


@pytest.fixture(scope="module")
def L(hiplib):
    assert torch.cuda.is_available()
    from prifit_amd import _lib
    return _lib


def run_fwd(L, a, b, na, nb):
    Bt, NA, NB = a.shape[0], a.shape[1], b.shape[1]
    d2 = torch.full((Bt, NA), 7.0, dtype=torch.float32, device="cuda")
    idx = torch.full((Bt, NA), 7, dtype=torch.int32, device="cuda")
    nws = L.query("prifit_chamfer_nn_workspace_floats", Bt, NA, NB)
    ws = torch.full((max(nws, 1),), float("nan"), dtype=torch.float32, device="cuda")
    L.call("prifit_chamfer_nn_fwd", L.ptr(a), L.ptr(b), L.ptr(na), L.ptr(nb), Bt, NA, NB, L.ptr(d2), L.ptr(idx), L.ptr(ws),
           L.cur_stream())
    return d2, idx


def run_bwd(L, a, b, na, nb, idx, g, ga=None, gb=None, accumulate=0):
    Bt, NA, NB = a.shape[0], a.shape[1], b.shape[1]
    ga = torch.full((Bt, NA, 3), 7.0, dtype=torch.float32, device="cuda") if ga is None else ga
    gb = torch.full((Bt, NB, 3), 7.0, dtype=torch.float32, device="cuda") if gb is None else gb
    L.call("prifit_chamfer_nn_bwd", L.ptr(a), L.ptr(b), L.ptr(na), L.ptr(nb), Bt, NA, NB, L.ptr(idx), L.ptr(g), L.ptr(ga),
           L.ptr(gb), accumulate, L.cur_stream())
    return ga, gb


def dev(c, *names):
    return [torch.from_numpy(np.array(c[n])).cuda() for n in names]


def assert_bits(got, want, what):
    got = got.cpu().numpy()
    same = cc.bits(got) == cc.bits(want)
    assert same.all(), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        what, (~same).sum(), same.size, np.argwhere(~same)[0], got[~same][0], want[~same][0])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("NA,NB", SHAPES)
def test_kernels_bit_exact(L, family, NA, NB):
    c = case(family, NA, NB)
    a, b, na, nb, g = dev(c, "a", "b", "na", "nb", "g")
    d2, idx = run_fwd(L, a, b, na, nb)
    assert_bits(idx, c["idx"], "idx")
    assert_bits(d2, c["d2"], "d2")
    ga, gb = run_bwd(L, a, b, na, nb, idx, g)
    assert_bits(ga, c["ga"], "ga")
    assert_bits(gb, c["gb"], "gb")


def test_full_counts_are_null_pointers(L):
    """na = nb = NULL means every row is live"""
    c = case("normal", 65, 255)
    a, b, g = dev(c, "a", "b", "g")
    d2r, idxr, _ = cc.nn_ref(c["a"], c["b"])
    gar, gbr = cc.bwd_ref(c["a"], c["b"], None, None, idxr, c["g"])
    d2, idx = run_fwd(L, a, b, None, None)
    ga, gb = run_bwd(L, a, b, None, None, idx, g)
    for got, want, what in ((idx, idxr, "idx"), (d2, d2r, "d2"), (ga, gar, "ga"), (gb, gbr, "gb")):
        assert_bits(got, want, what)


def test_lattice_inputs_contain_ties():
    """the lowest-index rule is exercised: on the lattice family more than one target attains the minimum for at least 5 %
    of the live rows (runs on the restatement alone)"""
    tied = rows = 0
    for NA, NB in SHAPES:
        c = case("lattice", NA, NB)
        for s in range(4):
            n = int(c["na"][s]) if c["nb"][s] > 0 else 0
            tied += int(c["ties"][s, :n].sum())
            rows += n
    print("lattice family: %d of %d live rows tied (%.1f %%)" % (tied, rows, 100.0 * tied / rows))
    assert tied >= 0.05 * rows


@pytest.mark.parametrize("NA,NB", [(65, 255), (257, 1031), (300, 5003)])
def test_rows_past_the_counts_are_never_read(L, NA, NB):
    """padded rows hold NaN, both clouds end where a NaN guard begins, the float outputs sit in sentinel guards"""
    c = case("normal", NA, NB)
    a_h, b_h = np.array(c["a"]), np.array(c["b"])
    for s in range(4):
        a_h[s, c["na"][s]:] = np.nan
        b_h[s, c["nb"][s]:] = np.nan
    a, a_base = guarded_like(torch.from_numpy(a_h).cuda(), 64, x_tail(3))
    b, b_base = guarded_like(torch.from_numpy(b_h).cuda(), 64, x_tail(3))
    na, nb, g = dev(c, "na", "nb", "g")
    g[torch.from_numpy(np.arange(NA)[None, :] >= c["na"][:, None]).cuda()] = float("nan")   # dead rows of g are not read either
    d2, idx = run_fwd(L, a, b, na, nb)
    ga, ga_base = guarded((4, NA, 3), 64, 4096, SENTINEL)
    gb, gb_base = guarded((4, NB, 3), 64, 4096, SENTINEL)
    run_bwd(L, a, b, na, nb, idx, g, ga, gb)
    for t in (d2, ga, gb):
        assert torch.isfinite(t).all()
    assert_guards_intact(ga_base, ga)
    assert_guards_intact(gb_base, gb)
    assert torch.isnan(a_base).sum() == a_base.numel() - sum(int(v) for v in c["na"]) * 3   # inputs not written
    for got, want, what in ((idx, c["idx"], "idx"), (d2, c["d2"], "d2"), (ga, c["ga"], "ga"), (gb, c["gb"], "gb")):
        assert_bits(got, want, what)


def test_same_bits_from_run_to_run_and_accumulate(L):
    c = case("normal", 257, 1031)
    a, b, na, nb, g = dev(c, "a", "b", "na", "nb", "g")
    runs = []
    for _ in range(2):
        d2, idx = run_fwd(L, a, b, na, nb)
        ga, gb = run_bwd(L, a, b, na, nb, idx, g)
        runs.append((d2, idx, ga, gb))
    for x, y in zip(*runs):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    pre = np.random.default_rng(5).standard_normal((4, 1031, 3)).astype(np.float32)
    _, want = cc.bwd_ref(c["a"], c["b"], c["na"], c["nb"], c["idx"], c["g"], gb0=pre)
    _, gb = run_bwd(L, a, b, na, nb, runs[0][1], g, gb=torch.from_numpy(pre).cuda(), accumulate=1)
    assert_bits(gb, want, "gb (accumulate_b)")


def test_bad_arguments_are_refused(L):
    a = torch.zeros(1, 4, 3, device="cuda")
    o = torch.zeros(1, 4, device="cuda")
    i = torch.zeros(1, 4, dtype=torch.int32, device="cuda")
    f = L.dll().prifit_chamfer_nn_fwd
    w = L.dll().prifit_chamfer_nn_bwd
    p = L.ptr
    assert f(None, p(a), None, None, 1, 4, 4, p(o), p(i), None, None) == -1
    assert f(p(a), p(a), None, None, 0, 4, 4, p(o), p(i), None, None) == -1
    assert f(p(a), p(a), None, None, 1, -1, 4, p(o), p(i), None, None) == -1
    assert f(p(a), p(a), None, None, 1, 4, -1, p(o), p(i), None, None) == -1
    assert f(p(a), p(a), None, None, 60000, 20000, 4, p(o), p(i), None, None) == -1      # B * NA * 3 past int32
    assert f(p(a), p(a), None, None, 1, 4, 1 << 30, p(o), p(i), None, None) == -1
    assert w(p(a), p(a), None, None, 1, 4, 4, p(i), p(o), None, p(a), 0, None) == -1
    assert w(p(a), p(a), None, None, 1, 4, 4, p(i), p(o), p(a), p(a), 0, None) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# public functions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def U(hiplib):
    from prifit_amd.src import utils
    return utils


def clouds(N, M, seed=11, B=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, N, 3)).astype(np.float32), rng.standard_normal((B, M, 3)).astype(np.float32)


def args_of(name, pred, gt):
    return (pred[0], gt[0]) if name == "chamfer_distance_single_shape" else (pred, gt)


def raises_upstream(name, kw, N, M):
    return name == "chamfer_distance_single_shape" and not kw["one_side"] and not kw["reduce"] and N != M


def check_value(U, name, kw, pred, gt):
    p, q = args_of(name, pred, gt)
    got = getattr(U, name)(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda(), **kw).double().cpu().numpy()
    P, Q = torch.from_numpy(p).double(), torch.from_numpy(q).double()
    want = cc.public64(name, P, Q, **kw).numpy()
    pg, gp, _, _ = cc.minima64(*((P[None], Q[None]) if P.dim() == 2 else (P, Q)))
    if kw.get("sqrt", False):
        pg, gp = cc.guard_sqrt64(pg), cc.guard_sqrt64(gp)
    bound = cc.value_bound(name, pg.numpy(), gp.numpy(), **kw)
    err = np.abs(got - want)
    print("%s %r: max err %.3e, largest err / bound %.3f" % (name, kw, err.max(), np.max(err / bound)))
    assert got.shape == want.shape
    assert (err <= bound).all()


@pytest.mark.parametrize("name,kw", cc.PUBLIC_CASES)
def test_public_values_against_fp64(U, name, kw):
    pred, gt = clouds(130, 97)
    if raises_upstream(name, kw, 130, 97):
        with pytest.raises(ValueError):
            getattr(U, name)(torch.from_numpy(pred[0]).cuda(), torch.from_numpy(gt[0]).cuda(), **kw)
    else:
        check_value(U, name, kw, pred, gt)
    if name == "chamfer_distance_single_shape" and not kw["reduce"]:
        check_value(U, name, kw, *clouds(65, 65, seed=12))


@pytest.mark.parametrize("name,kw", cc.PUBLIC_CASES)
def test_public_gradients_against_fp64(U, name, kw):
    N, M = (65, 65) if raises_upstream(name, kw, 130, 97) else (130, 97)
    pred, gt = clouds(N, M, seed=13)
    p, q = args_of(name, pred, gt)
    # the comparison presumes that fp32 and fp64 agree on every nearest neighbour (no near-ties in these seeded clouds)
    _, i32, _ = cc.nn_ref(pred, gt)
    _, j32, _ = cc.nn_ref(gt, pred)
    _, _, i64, j64 = cc.minima64(torch.from_numpy(pred).double(), torch.from_numpy(gt).double())
    assert (i32 == i64.numpy()).all() and (j32 == j64.numpy()).all()
    _, (gp64, cnt_p, abs_p), (gq64, cnt_q, abs_q) = cc.grad64(name, torch.from_numpy(p).double(), torch.from_numpy(q).double(), **kw)
    P = torch.from_numpy(p).cuda().requires_grad_(True)
    Q = torch.from_numpy(q).cuda().requires_grad_(True)
    getattr(U, name)(P, Q, **kw).sum().backward()
    for got, want, cnt, sabs, what in ((P.grad, gp64, cnt_p, abs_p, "pred"), (Q.grad, gq64, cnt_q, abs_q, "gt")):
        got = torch.zeros_like(want) if got is None else got.double().cpu()
        err, bound = (got - want).abs(), cc.grad_bound(cnt, sabs)
        print("%s %r d/d%s: max err %.3e, max bound %.3e" % (name, kw, what, err.max(), bound.max()))
        assert (err <= bound).all(), (what, float((err - bound).max()))
    assert P.grad is not None or Q.grad is not None


def test_values_recorded_from_the_reference(U, golden):
    z = golden("chamfer_pointsets")
    pred, gt = z["pred"], z["gt"]
    assert pred.shape == (2, 130, 3) and gt.shape == (2, 97, 3)
    P, Q = torch.from_numpy(pred).double(), torch.from_numpy(gt).double()
    seen = 0
    for name, kw in cc.PUBLIC_CASES:
        key = name + "".join("|%s=%s" % (k, int(v)) for k, v in sorted(kw.items()))
        if raises_upstream(name, kw, 130, 97):
            assert key not in z.files
            continue
        p, q = args_of(name, pred, gt)
        got = getattr(U, name)(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda(), **kw).double().cpu().numpy()
        pg, gp, _, _ = cc.minima64(*((P[:1], Q[:1]) if p.ndim == 2 else (P, Q)))
        if kw.get("sqrt", False):
            pg, gp = cc.guard_sqrt64(pg), cc.guard_sqrt64(gp)
        # both sides are fp32 computations of the same fp64 quantity: each is within the bound of it
        bound = 2.0 * cc.value_bound(name, pg.numpy(), gp.numpy(), **kw)
        assert got.shape == z[key].shape and (np.abs(got - z[key].astype(np.float64)) <= bound).all(), key
        seen += 1
    assert seen == 10
    # chamfer_distance_kdtree(source, target): per shape (mean_t + mean_s) / 2, plain sqrt
    for sq in (False, True):
        got = float(U.chamfer_distance_kdtree(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), sqrt=sq))
        pg, gp, _, _ = cc.minima64(P, Q)
        if sq:
            pg, gp = pg.sqrt(), gp.sqrt()
        bound = 2.0 * cc.value_bound("chamfer_distance", pg.numpy(), gp.numpy())
        assert abs(got - float(z["chamfer_distance_kdtree|sqrt=%d" % sq])) <= bound


def test_numpy_in_host_tensors_refused_unequal_sizes_refused(U):
    pred, gt = clouds(33, 20, seed=14)
    want = float(cc.public64("chamfer_distance", torch.from_numpy(pred).double(), torch.from_numpy(gt).double()))
    got = U.chamfer_distance(pred, gt)                      # numpy in, device tensor out
    assert got.is_cuda and abs(float(got) - want) <= 1e-5 * want
    assert U.chamfer_distance_one_side(pred.astype(np.float64), gt, side=0).is_cuda
    assert U.chamfer_distance_single_shape(pred[0], gt[0]).is_cuda
    for fn, args in ((U.chamfer_distance, (pred, gt)), (U.chamfer_distance_one_side, (pred, gt)),
                     (U.chamfer_distance_single_shape, (pred[0], gt[0]))):
        with pytest.raises(RuntimeError, match="need device tensors"):
            fn(*[torch.from_numpy(x) for x in args])
    with pytest.raises(ValueError):
        U.chamfer_distance_single_shape(pred[0], gt[0], reduce=False)
    with pytest.raises(ValueError):
        U.chamfer_distance_one_side(pred, gt, side=2)
    from prifit_amd import fit_ops
    d2, idx = fit_ops.ChamferNNFn.apply(torch.from_numpy(pred).cuda().requires_grad_(True), torch.from_numpy(gt).cuda())
    assert d2.requires_grad and not idx.requires_grad and idx.dtype == torch.int32


def test_ragged_callers_match_the_per_shape_form(U):
    """Loss.loss and the list form's source half pack ragged sample lists with counts: same value as shape by shape"""
    from prifit_amd.src.sample_ellipsoid import Loss
    rng = np.random.default_rng(15)
    gt = torch.from_numpy(rng.standard_normal((3, 50, 3)).astype(np.float32)).cuda()
    samples = [torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).cuda().requires_grad_(True) for n in (70, 31)]
    lists = [samples[0], None, samples[1]]
    loss = Loss().loss(gt, lists)
    loss.backward()
    per = [cc.public64("chamfer_distance", samples[k].detach().cpu().double()[None], gt[b].cpu().double()[None])
           for k, b in ((0, 0), (1, 2))]
    want = float(torch.stack(per).mean())
    assert abs(float(loss) - want) <= 1e-5 * want
    assert all(torch.isfinite(s.grad).all() and s.grad.abs().sum() > 0 for s in samples)

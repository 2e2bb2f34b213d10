"""CPU: the float64 restatements of tests/fit_common.py, so that tests/test_gpu_fit_guards.py stands on something checked.

- against the committed reference fixtures (fit_ellipsoid, fit_kat, fit_chamfer, fit_cuboid) at the tolerances
  tests/test_gpu_fit.py holds the kernels to against the same fixtures;
- fit64's gradient against central differences in float64;
- the stated conditions (validity, sign and extreme-row margins, both flip branches, budget rounding, SDF argmin clearance,
  duplicated targets that are somebody's nearest) on every input family of the GPU tests;
- sensitivity: float32 restatements with one formula wrong each are rejected by the very comparison functions, at the very
  bars, the GPU tests use."""
import numpy as np
import pytest
import torch

import fit_common as fc
from fit_common import F32, F64
from tests_helpers import fit_inputs


def _t(a):
    return torch.from_numpy(np.asarray(a))


def fixture_params(ge):
    r, V, c = (torch.stack([_t(ge["%s_%d" % (n, b)]) for b in range(2)]) for n in ("r", "V", "c"))
    return r, V, c, torch.ones(2, r.shape[1], dtype=torch.int32)


def test_fit64_against_the_reference_fixture(golden):
    g = golden("fit_ellipsoid")
    pts, _, _ = fit_inputs(2, 2048, 128, int(g["seed"]))
    K = g["r_0"].shape[0]
    W = torch.stack([_t(g["W_0"]), _t(g["W_1"])]).double().requires_grad_(True)
    out = fc.fit64(pts, W, [K, K], _t(g["R"]), True)
    gr = _t(g["grad_seed_table"])[:K].double()
    seeds = (gr[:, 0:3].expand(2, K, 3), gr[:, 3:12].reshape(K, 3, 3).expand(2, K, 3, 3), gr[:, 12:15].expand(2, K, 3))
    fc.fit_loss(out, *seeds).backward()
    assert bool(out["valid"].all())
    for b in range(2):
        torch.testing.assert_close(out["r"][b].detach().float(), _t(g[f"r_{b}"]), rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(out["V"][b].detach().float(), _t(g[f"V_{b}"]), rtol=1e-3, atol=1e-4)
        torch.testing.assert_close(out["c"][b].detach().float(), _t(g[f"c_{b}"]), rtol=1e-4, atol=1e-5)
        ref = _t(g[f"dW_{b}"])
        torch.testing.assert_close(W.grad[b].float(), ref, rtol=2e-3, atol=1e-4 * ref.abs().max().item())


def test_fit64_known_answer_fixture(golden):
    g = golden("fit_kat")
    out = fc.fit64(_t(g["points"]), _t(g["W"]).unsqueeze(0), [3], _t(g["R"]), False)
    assert bool(out["valid"].all())
    torch.testing.assert_close(out["r"][0].float(), _t(g["r_ref"]), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out["c"][0].float(), _t(g["c_ref"]), rtol=1e-4, atol=1e-4)
    assert bool((torch.linalg.det(out["V"][0]) > 0).all())


def test_svd_backward_is_the_oracles():
    """fit_common.Svd3 (batched) against oracle Svd3 (one matrix) on double inputs: the same gradient."""
    import prifit_oracle as orc
    gen = torch.Generator().manual_seed(3)
    M = torch.randn(4, 3, 3, generator=gen, dtype=F64)
    G = torch.randn(4, 3, 3, generator=gen, dtype=F64)
    Ma = M.clone().requires_grad_(True)
    (fc.Svd3.apply(Ma)[2] * G).sum().backward()
    for i in range(4):
        Mb = M[i].clone().requires_grad_(True)
        (orc.Svd3.apply(Mb)[2] * G[i]).sum().backward()
        torch.testing.assert_close(Ma.grad[i], Mb.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("kind,name", [("ellipsoid", "fit_chamfer"), ("cuboid", "fit_cuboid")])
def test_sdf_budget_samples_combine_against_the_reference_fixtures(golden, kind, name):
    ge, gc = golden("fit_ellipsoid"), golden(name)
    _, cham, _ = fit_inputs(2, 2048, 128, int(ge["seed"]))
    r, V, c, valid = fixture_params(ge)
    K = r.shape[1]
    torch.testing.assert_close(fc.sdf64(kind, cham[:, :256], r, V, c).float(), _t(gc["sdf_head"]), rtol=1e-4, atol=1e-6)
    loss, pd, ps, _, aux = fc.chamfer_chain(kind, r, V, c, valid, cham, 13312)
    assert aux["total"].tolist() == list(gc["nsamples"])
    torch.testing.assert_close(ps.float(), _t(gc["sdf_ts"]), rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(pd.float(), _t(gc["dist_st"]), rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(loss.float(), _t(gc["loss"]), rtol=1e-4, atol=1e-8)
    if kind == "cuboid":
        torch.testing.assert_close(aux["pts"][:, :64].float(), _t(gc["samples_head"]), rtol=1e-5, atol=1e-6)


def test_fit64_gradient_against_central_differences():
    """N = 40, three live slots of four, well separated singular values (the 1e-6 clamp inactive): 1e-6 of the largest entry."""
    case = fc.fit_case("n40_soft")
    out, dW = fc.fit_reference(case)
    S = out["S"][out["live"]]
    assert float((S[:, :2] - S[:, 1:]).min()) > 1e-5
    W0 = case["W"].double()
    f = lambda W: float(fc.fit_loss(fc.fit64(case["points"], W, case["count"], case["rnd"], case["canonical"]),
                                    case["g_r"], case["g_V"], case["g_c"]))
    h, worst = 1e-6, 0.0
    gen = torch.Generator().manual_seed(0)
    for i in torch.randperm(40, generator=gen)[:12].tolist():
        for k in range(3):
            Wp, Wm = W0.clone(), W0.clone()
            Wp[0, i, k] += h
            Wm[0, i, k] -= h
            worst = max(worst, abs((f(Wp) - f(Wm)) / (2 * h) - float(dW[0, i, k])))
    assert worst <= 1e-6 * float(dW.abs().max()), worst / float(dW.abs().max())
    assert float(dW[0, :, 3].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# conditions on the input families
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in fc.FIT_CASES])
def test_fit_families_meet_the_conditions(name):
    case = fc.fit_case(name)
    out = fc.fit64(case["points"], case["W"], case["count"], case["rnd"], case["canonical"])
    fc.fit_conditions(out, case["canonical"])
    out32 = fc.fit64(case["points"], case["W"], case["count"], case["rnd"], case["canonical"], F32)
    assert torch.equal(out32["valid"], out["valid"])
    if case["family"] == "special":
        b = len(case["count"]) - 1
        assert not bool(out["valid"][b, fc.PLANE_SLOT]) and int(out["valid"][b].sum()) == 31      # live slots behind it
        S = out["S"][b, fc.ISO_SLOT]
        gaps = (S[:2] - S[1:]) / S[0]
        assert 1e-4 < float(gaps.min()) and float(gaps.max()) < 1e-2, gaps
    if case["family"] == "hard":
        assert int((case["W"] == 0).sum()) > 0


@pytest.mark.parametrize("kind", ["ellipsoid", "cuboid"])
@pytest.mark.parametrize("M,KM", fc.SDF_CASES)
def test_sdf_families_meet_the_conditions(kind, M, KM):
    case = fc.sdf_case(kind, M, KM)
    red, _, _ = fc.sdf_reference(case)
    unclear = ~red["clear"]
    unclear[0, :case["placed"]] = False
    assert int(unclear.sum()) <= 0.01 * 2 * M, int(unclear.sum())
    assert bool((red["arg"][1] == -1).all()) and float(red["sum_sq"][1]) == 0.0
    if case["placed"]:
        if kind == "ellipsoid":
            assert float(red["fval"][0, 0]) == 0.0 and int(red["arg"][0, 0]) == 0     # the centre: k0 = 0 exactly
        else:
            assert float(red["fval"][0, 1:4].abs().max()) == 0.0           # face, edge, vertex: exactly on the box
        assert float(red["fval"][0, 5]) > 1.0                              # far outside


@pytest.mark.parametrize("kind", ["ellipsoid", "cuboid"])
@pytest.mark.parametrize("M,KM,cap", [(M, 32, 600) for M in fc.NN_M] + [(1000, 32, 13312), (1000, 64, 16640)])
def test_search_families_meet_the_conditions(kind, M, KM, cap):
    case = fc.nn_case(kind, M, KM, cap)
    fc.budget_conditions(case["frac"], case["valid"])
    ref = fc.nn_reference(case)
    if KM == 32:
        assert int(ref["n"][1, 0]) == 100 and float(case["frac"][1, 0]) < 0.49   # the tiny slot: its share rounds to 0 -> 100
        if cap == 600:
            assert ref["total"].tolist() == [600, 600, 0, 600]
            assert int((ref["n"][3] == 0).sum()) >= 29                     # n = cap - off, and n = 0 behind the clip
    hits = fc.check_neighbours("nn", ref["idx"], ref, ref["d2"], case["targets"], case["pairs"], {})
    shapes_with_samples = int((ref["total"] > 0).sum())
    assert hits >= len(case["pairs"]) * shapes_with_samples
    chunk = -(-M // 8)
    if M == 8200:
        assert chunk == 1025 and (chunk + 1023, chunk + 1024) in case["pairs"] and (chunk - 1, chunk) in case["pairs"]   # tiles, ranges
    if M == 1030:
        assert chunk == 129 and (128, 129) in case["pairs"]


# ---------------------------------------------------------------------------------------------------------------------------
# sensitivity: one wrong formula each, in float32, through the comparison functions of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation,quantity", [("unweighted_centre", "r"), ("no_flip", "V"), ("svd_k", "dW")])
def test_bars_reject_a_wrong_fit(mutation, quantity):
    case = fc.fit_case("n256_soft64")
    o64, dW64 = fc.fit_reference(case)
    o32, dW32 = fc.fit_reference(case, F32)
    om, dWm = fc.fit_reference(case, F32, mutate=(mutation,))
    pick = lambda o, dW: dW if quantity == "dW" else o[quantity] * o64["valid"].view(*o64["valid"].shape, *([1] * (o[quantity].dim() - 2)))
    good, bad = {}, {}
    fc.check(quantity, pick(o32, dW32), pick(o64, dW64), pick(o32, dW32), good)
    fc.assert_bars(good)
    fc.check(quantity, pick(om, dWm), pick(o64, dW64), pick(o32, dW32), bad)
    with pytest.raises(AssertionError):
        fc.assert_bars(bad)


def test_bars_reject_a_cuboid_gradient_without_the_inside_term():
    case = fc.sdf_case("cuboid", 257, 32)
    _, _, gb64 = fc.sdf_reference(case)
    _, _, gb32 = fc.sdf_reference(case, F32)
    _, _, gbm = fc.sdf_reference(case, F32, mutate=("no_plus_one",))
    for i, name in enumerate(("g_r", "g_V", "g_c")):
        bad = {}
        fc.check(name, gbm[i], gb64[i], gb32[i], bad)
        with pytest.raises(AssertionError):
            fc.assert_bars(bad)


def test_exact_comparison_rejects_a_budget_without_the_hundred():
    case = fc.nn_case("ellipsoid", 1000, 32, 13312)
    n64, off64, _ = fc.budget64("ellipsoid", case["r"], case["valid"], 13312)
    n32, off32, _ = fc.budget64("ellipsoid", case["r"], case["valid"], 13312, F32)
    fc.assert_exact("n", n32, n64)
    fc.assert_exact("off", off32, off64)
    nm, offm, _ = fc.budget64("ellipsoid", case["r"], case["valid"], 13312, F32, mutate=("no_hundred",))
    with pytest.raises(AssertionError):
        fc.assert_exact("n", nm, n64)
    with pytest.raises(AssertionError):
        fc.assert_exact("off", offm, off64)


@pytest.mark.parametrize("M", [8, 1030])
def test_neighbour_check_rejects_the_last_of_duplicated_targets(M):
    case = fc.nn_case("ellipsoid", M, 32, 600)
    ref = fc.nn_reference(case)
    r32 = fc.nn_reference(case, F32)
    good = {}
    fc.check_neighbours("nn", r32["idx"], ref, r32["d2"], case["targets"], case["pairs"], good)
    fc.assert_bars(good)
    rm = fc.nn_reference(case, F32, last=True)
    with pytest.raises(AssertionError):
        fc.check_neighbours("nn", rm["idx"], ref, r32["d2"], case["targets"], case["pairs"], {})


def test_bars_reject_a_sample_given_to_the_slot_before_an_empty_one():
    case = fc.nn_case("ellipsoid", 1000, 32, 13312)
    ref = fc.nn_reference(case)
    r32 = fc.nn_reference(case, F32)
    rm = fc.nn_reference(case, F32, mutate=("slot_before_empty",))
    good, bad = {}, {}
    fc.check("sum_d2", r32["sum_d2"], ref["sum_d2"], r32["sum_d2"], good)
    fc.assert_bars(good)
    fc.check("sum_d2", rm["sum_d2"], ref["sum_d2"], r32["sum_d2"], bad)
    with pytest.raises(AssertionError):
        fc.assert_bars(bad)


def test_combine64_and_the_small_statements():
    valid = torch.tensor([[1, 0], [0, 0], [0, 1]], dtype=torch.int32)
    d2, tot, sdf = torch.tensor([2.0, 5.0, 0.0]), torch.tensor([4, 7, 0]), torch.tensor([1.0, 3.0, 6.0])
    loss, pd, ps = fc.combine64(d2, tot, sdf, valid, 2)
    assert abs(float(loss) - ((0.5 + 0.5) / 2 + (0.0 + 3.0) / 2) / 2) < 1e-15
    assert float(fc.combine64(d2, tot, sdf, torch.zeros_like(valid), 2)[0]) == 0.0
    assert fc.verdict(torch.tensor([3, 70]), torch.tensor([[1, 1, 0, 0], [1, 1, 1, 1]]), 4, 25, 32) == ([2, 70], 1)
    assert abs(float(fc.bandwidth64(torch.tensor([[4.0, 1e-9]]))[0]) - (2.0 + 1e-3) / 2) < 1e-12

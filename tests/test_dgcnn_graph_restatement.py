"""The float64 restatements of tests/dgcnn_graph_common.py pinned against torch itself (F.group_norm + F.leaky_relu + max over the
k neighbours on the explicit [B, N, k, C] tensor, with autograd), the stacked form against the unstacked one, the
precision-independence of every discrete decision on every case of the tables, the exactness of the lattice distances, and
three mutations the bars must reject -- all on the CPU."""
import pytest
import torch
import torch.nn.functional as Fn

import bn_common as bc
import dgcnn_graph_common as gc
from bn_common import F32, F64


def close(a, b, tol=1e-11):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
    assert err <= tol, err


@pytest.mark.parametrize("stacked", [False, True])
def test_block_equals_group_norm_leaky_relu_max_with_autograd_in_float64(stacked):
    """The CPU version of test_gpu_dgcnn.py::test_edge_tables_forward_and_backward_against_torch: tables, pooled output and every
    gradient of the restated block against torch on the explicit tensor."""
    case = gc.chain_case(64, N=32, k=9, B=2)
    U, Vb, idx = case["U"].to(F64), case["V2"].to(F64), case["idx"]
    if not stacked:
        case = dict(case, selfterm=0, V2=(U - Vb).to(F32))       # exact on the grid: the same centre term
        assert torch.equal(case["V2"].to(F64), U - Vb)
    f = gc.chain_forward(case)
    g = gc.chain_backward(case, f)
    B, N, C, k, slope = case["B"], case["N"], case["C"], case["k"], case["slope"]
    assert bool((idx[1] < 0).any()) and bool((idx[1] >= N).any())

    first = (torch.cat([U, Vb], 2) if stacked else U).clone().requires_grad_(True)
    second = case["V2"].to(F64).clone().requires_grad_(True)
    gamma, beta = case["gamma"].to(F64).requires_grad_(True), case["beta"].to(F64).requires_grad_(True)
    Ur = first[:, :, :C]
    centre = Ur - first[:, :, C:] if stacked else second
    ok = ((idx >= 0) & (idx < N)).unsqueeze(-1)
    rows = torch.gather(Ur.unsqueeze(1).expand(B, N, N, C), 2, idx.clamp(0, N - 1).long().unsqueeze(-1).expand(B, N, k, C))
    y = torch.where(ok, rows - centre.unsqueeze(2), torch.zeros((), dtype=F64))
    z = Fn.leaky_relu(Fn.group_norm(y.permute(0, 3, 1, 2), case["groups"], gamma, beta, gc.GN_EPS), slope)      # [B, C, N, k]
    top = z.amax(3).permute(0, 2, 1)
    # amax spreads a tie's gradient evenly where the block gives it to the FIRST winner: the graph goes through a gather at the
    # restatement's winners, after checking that each attains torch's maximum and is the first to do so
    zz = z.permute(0, 2, 3, 1)                                                                                   # [B, N, k, C]
    firstpos = torch.where(zz.detach() == top.detach().unsqueeze(2), torch.arange(k).view(1, 1, k, 1), k).min(2).values
    zero_scale = (f["fin"]["scale"] == 0).unsqueeze(1).expand_as(firstpos)
    assert torch.equal(firstpos[~zero_scale], f["win"][~zero_scale])
    out = torch.gather(zz, 2, f["win"].unsqueeze(2)).squeeze(2)
    assert torch.equal(out.detach(), top.detach())
    close(f["out"], out)
    (out * case["gout"].to(F64)).sum().backward()
    if stacked:
        close(g["dU"], first.grad[:, :, :C])
        close(g["dV"], first.grad[:, :, C:])
    else:
        close(g["dU"], first.grad)
        close(g["dV"], second.grad)
    close(g["dgamma"], gamma.grad)
    close(g["dbeta"], beta.grad)


def test_stacked_form_equals_the_unstacked_one():
    case = gc.edge_case(64, 20, 48, 1, degrees=True)
    U, Vb = case["U"].to(F64), case["V2"].to(F64)
    Vc = (U - Vb).to(F32)
    assert torch.equal(Vc.to(F64), U - Vb)
    s1, s0 = gc.edge_stats(case["U"], case["V2"], case["idx"], 1), gc.edge_stats(case["U"], Vc, case["idx"], 0)
    for n in ("ymax", "ymin", "karg", "ysum", "vct", "slab"):
        assert torch.equal(s1[n], s0[n]), n
    _, ystar, _ = gc.edge_pool(s1["ymax"], s1["ymin"], case["scale"], case["shift"], case["slope"])
    T = gc.edge_T(case["gp"], ystar, case["scale"], case["shift"], case["slope"])
    win = gc.winners(s1["kx"], s1["kn"], case["scale"])
    tabs = (win, T, case["ca"], case["cb"], case["cd"])
    dU1, dVb = gc.edge_bwd(case["U"], case["V2"], case["idx"], 1, *tabs)
    dU0, dVc = gc.edge_bwd(case["U"], Vc, case["idx"], 0, *tabs)
    close(dVb, -dVc)                    # Vb enters the centre term with a minus sign
    close(dU1, dU0 + dVc)               # and the point's own row of U with a plus sign
    # the case does hold what it is built for: the prescribed in-degrees, and a zero row that wins
    deg = gc.in_degrees(case["idx"], case["N"])
    assert deg[0, :len(gc.DEGREES)].tolist() == list(gc.DEGREES)
    n_w = torch.gather(case["idx"][1].long(), 1, s1["kx"][1, :, 8:16].clamp(max=case["k"] - 1))
    assert bool(((n_w[2:5] < 0) | (n_w[2:5] >= case["N"])).any()) and bool((s1["ymax"][1, 2, 8:16] == 0).all())


def test_point_without_a_valid_neighbour_and_first_position_of_a_tie():
    case = gc.edge_case(64, 7, 16, 0)
    st = gc.edge_stats(case["U"], case["V2"], case["idx"], 0)
    assert int(st["nv"][1, 1, 0]) == 0
    for n in ("ymax", "ymin", "ysum", "kx", "kn"):
        assert not bool(st[n][1, 1].any()), n
    k = case["k"]
    assert bool((case["idx"][0, :, k - 1] == case["idx"][0, :, (k - 1) // 2]).all())
    assert not bool((st["kx"][0] == k - 1).any()) and not bool((st["kn"][0] == k - 1).any())


def test_a_winner_sits_behind_position_64_in_the_long_lists():
    for c in gc.BWD_CASES:
        if c[1] > 64:
            case = gc.edge_case(*c[:4], degrees=True)
            st = gc.edge_stats(case["U"], case["V2"], case["idx"], case["selfterm"])
            win = gc.winners(st["kx"], st["kn"], case["scale"])
            assert bool((win >= 64).any()) and bool(((case["scale"] < 0).unsqueeze(1) & (win == st["kn"])).any())


_CASES = gc.all_cases()


@pytest.mark.parametrize("label", [c[0] for c in _CASES])
def test_decisions_do_not_depend_on_the_precision(label):
    case = dict(_CASES)[label]()
    for d32, d64 in zip(gc.decisions(case, F32), gc.decisions(case, F64)):
        assert int((d32 != d64).sum()) == 0
    if case["kind"] == "edge":           # and y itself is exact in float32
        y32 = gc.edge_y(case["U"], case["V2"], case["idx"], case["selfterm"])[0]
        y64 = gc.edge_y(case["U"].to(F64), case["V2"].to(F64), case["idx"], case["selfterm"])[0]
        assert torch.equal(y32.to(F64), y64)


@pytest.mark.parametrize("N,k", sorted(set(gc.KNN_TOPK_CASES + gc.KNN3_CASES)))
def test_lattice_distances_are_exact_in_float32_so_the_order_is_the_same(N, k):
    """Equal values give equal stable sorts: the float64 sort is the expected answer of a float32 kernel in any fma order."""
    for kind in gc.KNN_KINDS:
        x = gc.knn_cloud(kind, 1, N, bc.gen_of(bc.seed_of(31, N, k)))
        G64, xx64 = gc.gram(x)
        G32, xx32 = gc.gram(x, F32)
        assert torch.equal(G32.to(F64), G64) and torch.equal(xx32.to(F64), xx64)
        v32, v64 = gc.knn_values(G32, xx32, F32), gc.knn_values(G64, xx64)
        assert torch.equal(v32.to(F64), v64)
        if N <= 130:
            i64 = gc.knn_ref(G64, xx64, k)
            assert torch.equal(gc.knn_ref(G32, xx32, k, F32), i64)
            if kind == "same":
                assert torch.equal(i64[0], torch.arange(k, dtype=torch.int32).expand(N, k))
            else:
                ties = v64[0].gather(1, i64[0].long())
                assert kind != "doubled" or k < 2 or bool((ties[:, 1:] == ties[:, :-1]).any())


def test_csr_offsets_and_feature_restatements_on_a_hand_case():
    idx = torch.tensor([2, 0, 2, -1, 3, 2, 4], dtype=torch.int32)
    assert gc.csr_offsets(idx, 4).tolist() == [0, 1, 1, 4, 5]
    x = torch.tensor([[[1.0, 2.0], [3.0, 5.0], [7.0, 11.0]]], dtype=F64)
    f = gc.edge_feature(x, torch.tensor([[[1], [2], [0]]], dtype=torch.int32), 5)
    assert f[0, :, 0].tolist() == [[2.0, 3.0, 1.0, 2.0, 0.0], [4.0, 6.0, 3.0, 5.0, 0.0], [-6.0, -9.0, 7.0, 11.0, 0.0]]
    w = gc.winners_case(3, 5, 64, 64)
    dX, dW = gc.winners_terms(w["arg"], w["T"], w["W"], w["X"], 5)
    ref_dX, ref_dW = torch.zeros(15, 64, dtype=F64), torch.zeros(64, 64, dtype=F64)
    for b in range(3):
        for c in range(64):
            if w["T"][b, c] != 0:
                r = b * 5 + int(w["arg"][b, c])
                ref_dX[r] += w["T"][b, c].double() * w["W"][c].double()
                ref_dW[c] += w["T"][b, c].double() * w["X"][r].double()
    close(dX, ref_dX)
    close(dW, ref_dW)


def test_bars_reject_a_dropped_in_edge_a_moved_winner_and_a_one_ulp_bias():
    case = gc.edge_case(64, 20, 48, 0, degrees=True)
    idx, N, k = case["idx"], case["N"], case["k"]
    ref = {}
    for dt in (F64, F32):
        st = gc.edge_stats(case["U"], case["V2"], idx, 0, dt)
        _, ystar, _ = gc.edge_pool(st["ymax"], st["ymin"], case["scale"], case["shift"], case["slope"], dt)
        T = gc.edge_T(case["gp"], ystar, case["scale"], case["shift"], case["slope"], dt)
        win = gc.winners(st["kx"], st["kn"], case["scale"])
        ref[dt] = dict(st=st, T=T, win=win, g=gc.edge_bwd(case["U"], case["V2"], idx, 0, win, T, case["ca"], case["cb"], case["cd"], dt))
    absU, absV = gc.edge_bwd_absum(case["U"], case["V2"], idx, 0, ref[F64]["win"], ref[F64]["T"], case["ca"], case["cb"], case["cd"])
    rep = bc.Report()
    rep.red("dU", "ok", ref[F32]["g"][0], ref[F64]["g"][0], ref[F32]["g"][0], absU)
    rep.red("dVc", "ok", ref[F32]["g"][1], ref[F64]["g"][1], ref[F32]["g"][1], absV)
    rep.assert_bars()

    # (1) one in-edge dropped from one dU row: the degree-130 point loses the edge of one list position
    hub = 10
    assert gc.DEGREES[hub] == 130
    i, j = (idx[0] == hub).nonzero()[0].tolist()
    dropped = idx.clone()
    dropped[0, i, j] = -1
    dU_drop = gc.edge_bwd(case["U"], case["V2"], dropped, 0, ref[F32]["win"], ref[F32]["T"], case["ca"], case["cb"], case["cd"], F32)[0]
    full = ref[F32]["g"][0].clone()
    full[0, hub] = dU_drop[0, hub]
    rep = bc.Report()
    rep.red("dU", "dropped", full, ref[F64]["g"][0], ref[F32]["g"][0], absU)
    with pytest.raises(AssertionError):
        rep.assert_bars()

    # (2) a winner moved to the second of two tied positions: every list of sample 0 repeats an entry ... of a random graph
    tied = gc.edge_case(64, 7, 16, 0)
    st = gc.edge_stats(tied["U"], tied["V2"], tied["idx"], 0)
    kk = tied["k"]
    at = (st["kx"][0] == (kk - 1) // 2).nonzero()
    assert at.numel() > 0                                   # the tie's first position does win somewhere
    moved = st["kx"].clone()
    p, c = at[0].tolist()
    assert st["y"][0, p, kk - 1, c] == st["y"][0, p, (kk - 1) // 2, c]
    moved[0, p, c] = kk - 1
    assert not torch.equal((moved | (st["kn"] << 10) | (st["nv"] << 20)).to(torch.int32), st["karg"])
    _, ystar, _ = gc.edge_pool(st["ymax"], st["ymin"], tied["scale"], tied["shift"], tied["slope"])
    T = gc.edge_T(tied["gp"], ystar, tied["scale"], tied["shift"], tied["slope"])
    w_ok, w_mv = gc.winners(st["kx"], st["kn"], tied["scale"]), gc.winners(moved, st["kn"], tied["scale"])
    if bool((tied["scale"][0, c] >= 0)):
        g_ok = gc.edge_bwd(tied["U"], tied["V2"], tied["idx"], 0, w_ok, T, tied["ca"], tied["cb"], tied["cd"])
        g_mv = gc.edge_bwd(tied["U"], tied["V2"], tied["idx"], 0, w_mv, T, tied["ca"], tied["cb"], tied["cd"])
        close(g_ok[0], g_mv[0])          # the same neighbour: the gradients cannot tell, only the exact comparison of karg can

    # (3) a one-ulp bias on ysum.  One ulp of the RESULT is at most 2^-23 of the sum of |terms|, half the floor of the bar
    # (MARGIN x 2^-24): the measure registers it and no bar of this convention can reject it.  What the bar does reject is the
    # bias as a summation defect produces it -- every addition of the chain rounded one ulp the same way -- at k = 130
    long = gc.edge_case(64, 130, 48, 1)
    y32 = gc.edge_stats(long["U"], long["V2"], long["idx"], 1, F32)["y"]
    st64 = gc.edge_stats(long["U"], long["V2"], long["idx"], 1)
    s64, s32, absum = st64["ysum"], y32.sum(2), st64["y"].abs().sum(2)
    inf = torch.full_like(s32, float("inf"))
    rep = bc.Report()
    rep.red("ysum", "ok", s32, s64, s32, absum)
    rep.red("ysum", "one ulp", torch.nextafter(s32, inf), s64, s32, absum)
    rep.assert_bars()
    assert rep.rows[1][2] > rep.rows[0][2]
    chain = torch.zeros_like(s32)
    for j in range(long["k"]):
        chain = torch.nextafter(chain + y32[:, :, j], inf)
    rep.red("ysum", "one ulp per addition", chain, s64, s32, absum)
    with pytest.raises(AssertionError):
        rep.assert_bars()

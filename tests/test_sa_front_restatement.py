"""tests/sa_front_common.py on the CPU: every restatement against an independent statement (the oracle's Python functions,
torch conv1d / matmul / autograd / index_select / index_add_), the exactness of the lattice distances in float32, that every case
list of tests/test_gpu_sa_front_guards.py reaches the path it is named for (pure arithmetic on the case tuples, restating the
launchers' selections), and that the decision-margin builder leaves no violation."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_common as bc
import prifit_oracle as orc
import sa_front_common as sc
from bn_common import F32, F64
from prifit_amd import synth


def _t(a):
    return torch.from_numpy(np.asarray(a))


# ---------------------------------------------------------------------------------------------------------------------------
# restatements against independent statements, in float64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cube", "lattice"])
def test_index_restatements_equal_the_oracles(kind):
    B, N, S = 3, 130, 9
    if kind == "cube":
        xyz = _t(synth.cloud("cube", B, N, 3)).to(F64)
        ctr = xyz[:, :S].clone()
    else:
        xyz, ctr = (t.to(F64) for t in sc.ball_case(N, S, (sc.R2_SMALL, sc.R2_BIG), B))
    start = torch.tensor([0, N - 1, N // 2])
    assert torch.equal(sc.fps(xyz, N, start), orc.farthest_point_sample(xyz, N, start))
    d = sc.sqdist_expanded(ctr, xyz)
    assert torch.equal(d, orc.square_distance(ctr, xyz))
    for radius, K in ((0.125, 4), (0.5, 16), (3.5, 200)):
        r2 = float(np.float32(radius ** 2))
        want = orc.query_ball_point(float(np.sqrt(np.float64(r2))), min(K, N), xyz, ctr) if kind == "cube" else None
        got = sc.ball_query(xyz, ctr, r2, K)
        if want is None:                                     # on the lattice the threshold itself decides: state it directly
            ids = torch.where(d > r2, N, torch.arange(N).expand(B, S, N)).sort(-1).values
            ids = torch.cat([ids, torch.full((B, S, max(0, K - N)), N)], -1)[:, :, :K]
            want = torch.where(ids == N, ids[:, :, :1].expand(-1, -1, K), ids)
        elif K > N:
            want = torch.cat([want, want[:, :, :1].expand(-1, -1, K - N)], -1)
        assert torch.equal(got, want), (kind, radius)
    d3, i3 = sc.three_nn(xyz, ctr)
    od, oi = orc.three_nn(xyz, ctr)
    assert torch.equal(d3, od)
    assert torch.equal(torch.gather(sc.sqdist_expanded(xyz, ctr), 2, i3), od)      # (an unstable sort may swap equal ones)
    if kind == "cube":
        assert torch.equal(i3, oi)
    p2 = torch.randn(B, S, 24, dtype=F64)
    w = sc.nn_weights(d3)
    torch.testing.assert_close(sc.interpolate(p2, i3, w), orc.three_interpolate(p2, d3, i3), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(w.sum(-1), torch.ones(B, N, dtype=F64), rtol=1e-12, atol=0)


def test_lattice_distance_ties_go_to_the_lowest_index():
    xyz = torch.tensor([[[0.0, 0, 0], [0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [0.5, 0, 0]]])
    assert sc.fps(xyz, 3, torch.tensor([0])).tolist() == [[0, 1, 2]]
    assert sc.three_nn(xyz[:, :1], xyz[:, 1:])[1].tolist() == [[[0, 1, 2]]]
    assert sc.ball_query(xyz, xyz[:, :1], 0.25, 3).tolist() == [[[0, 1, 2]]]          # ON the radius counts as inside
    assert sc.ball_query(xyz, torch.full((1, 1, 3), sc.FAR), 0.25, 3).tolist() == [[[5, 5, 5]]]
    assert sc.ball_query(xyz, xyz[:, 1:2], 0.0, 4).tolist() == [[[1, 4, 1, 1]]]


@pytest.mark.parametrize("D,feat_first", [(0, 0), (3, 1), (6, 0), (9, 1)])
def test_rows_layer_tables_and_weight_gradient_equal_torch(D, feat_first):
    B, N, S, K, C = 3, 21, 5, 7, 16
    gen = bc.gen_of(50 + D)
    xyz, ctr = torch.randn(B, N, 3, generator=gen, dtype=F64), torch.randn(B, S, 3, generator=gen, dtype=F64)
    feat = torch.randn(B, N, D, generator=gen, dtype=F64) if D else None
    idx = sc.oob_index((B, S, K), N, gen)
    W = torch.randn(C, D + 3, generator=gen, dtype=F64).requires_grad_(True)
    b = torch.randn(C, generator=gen, dtype=F64)
    rows = sc.grouped_rows(xyz, ctr, feat, idx, feat_first)
    ok = (idx >= 0) & (idx < N)
    assert bool((~ok).any()) and not bool(rows[~ok].any())
    want = torch.zeros(B, S, K, D + 3, dtype=F64)
    for bb, s, k in ok.nonzero().tolist():
        rel, f = xyz[bb, idx[bb, s, k]] - ctr[bb, s], (feat[bb, idx[bb, s, k]] if D else xyz.new_zeros(0))
        want[bb, s, k] = torch.cat([f, rel] if feat_first else [rel, f])
    assert torch.equal(rows, want)
    Y = sc.first_layer(rows, W, b)
    conv = F.conv1d(rows.reshape(1, -1, D + 3).transpose(1, 2), W.unsqueeze(-1), b).transpose(1, 2).reshape(B, S, K, C)
    torch.testing.assert_close(Y, conv, rtol=1e-13, atol=1e-13)
    dY = torch.randn(B * S * K, C, generator=gen, dtype=F64)
    (conv.reshape(-1, C) * dY).sum().backward()
    torch.testing.assert_close(sc.first_layer_dw(dY, rows), W.grad, rtol=1e-12, atol=1e-12)
    assert bool((sc.first_layer_dw_absum(dY, rows) >= sc.first_layer_dw(dY, rows).abs() - 1e-12).all())
    # the tables: U_j - Vc_s == conv1([feat_j | xyz_j - c_s]) + b, and the layer by linearity
    U, Vc = sc.point_tables(xyz, ctr, feat, W.detach(), b, feat_first)
    torch.testing.assert_close(sc.gather_layer(U, Vc, None, idx)[ok], Y.detach()[ok], rtol=1e-12, atol=1e-12)
    assert torch.equal(sc.gather_layer(U, Vc, b, idx)[~ok], b.expand(int((~ok).sum()), C))
    # statistics slabs
    for q in (4, 8):
        sl = sc.slab_stats(Y.detach(), q)
        assert sl.shape == (B * -(-S // q), 2, C)
        torch.testing.assert_close(sl[:, 0].sum(0), Y.detach().reshape(-1, C).sum(0), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(sl[-1, 1], (Y.detach()[B - 1, (S - 1) // q * q:] ** 2).reshape(-1, C).sum(0), rtol=1e-12, atol=1e-12)


def test_batchnorm_form_of_dy_equals_autograd_of_the_layer():
    """dY of relu(bn(Y1)) in training mode is ca * mask * g + cb * y + cd with the coefficients of bn_common.bn_bwd_finalize"""
    P, C = 40, 8
    gen = bc.gen_of(51)
    Y1 = torch.randn(P, C, generator=gen, dtype=F64).requires_grad_(True)
    gamma, beta = bc.signed(C, 0.5, 1.5, gen).to(F64), bc.signed(C, 0.1, 1.0, gen).to(F64)
    G = torch.randn(P, C, generator=gen, dtype=F64)
    (F.relu(F.batch_norm(Y1, None, None, gamma, beta, True, 0.0, 1e-5)) * G).sum().backward()
    y = Y1.detach()
    fin = bc.bn_finalize(y.sum(0), (y * y).sum(0), float(P), gamma, beta, 1e-5)
    Gm = bc.masked_grad(G, y, fin["scale"], fin["shift"], 0, 0.0)
    t0, t1 = bc.bwd_terms(Gm, y, fin["mean"], fin["invstd"], 0)
    co = bc.bn_bwd_finalize(t0.sum(0), t1.sum(0), float(P), 1, fin["scale"], fin["mean"], fin["invstd"])
    torch.testing.assert_close(sc.bn_dy(G, y, fin["scale"], fin["shift"], co["a"], co["b"], co["d"]), Y1.grad, rtol=1e-10, atol=1e-10)


def test_scatter_interpolation_and_fp_rows_equal_torch():
    B, N, S, K, C = 3, 13, 4, 5, 3
    gen = bc.gen_of(52)
    idx = sc.oob_index((B, S, K), N, gen, share=4)
    g, d0 = torch.randn(B, S * K, C, generator=gen, dtype=F64), torch.randn(B, N, C, generator=gen, dtype=F64)
    feat = torch.zeros(B, N, C, dtype=F64, requires_grad=True)
    (sc.take_rows(feat, idx)[0].reshape(B, S * K, C) * g).sum().backward()
    torch.testing.assert_close(sc.scatter_add(g, idx.reshape(B, -1), d0), d0 + feat.grad, rtol=1e-13, atol=1e-13)
    p2 = torch.randn(B, S, C, generator=gen, dtype=F64).requires_grad_(True)
    i3 = torch.randint(0, S, (B, N, 3), generator=gen)
    w = torch.rand(B, N, 3, generator=gen, dtype=F64)
    out = sc.interpolate(p2, i3, w)
    want = (orc.gather_rows(p2, i3) * w.unsqueeze(-1)).sum(2)
    torch.testing.assert_close(out, want, rtol=1e-13, atol=1e-13)
    go = torch.randn(B, N, C, generator=gen, dtype=F64)
    (want * go).sum().backward()
    dp0 = torch.randn(B, S, C, generator=gen, dtype=F64)
    torch.testing.assert_close(sc.interpolate_bwd(go, i3, w, dp0), dp0 + p2.grad, rtol=1e-13, atol=1e-13)
    p1 = torch.randn(B, N, 6, generator=gen, dtype=F64)
    rows = sc.fp_rows(p2.detach(), i3, w, p1, 12, N)
    assert torch.equal(rows, torch.cat([out.detach(), p1, torch.zeros(B, N, 3, dtype=F64)], -1))
    one = sc.fp_rows(p2.detach()[:, :1], None, None, None, 4, N)
    assert torch.equal(one, torch.cat([p2.detach()[:, :1].expand(B, N, C), torch.zeros(B, N, 1, dtype=F64)], -1))


def test_column_packers_equal_index_select_and_index_add():
    gen = bc.gen_of(53)
    for (rows, scols), cmap in zip(sc.PACK_SHAPES, sc.PACK_MAPS):
        w = torch.randn(rows, scols, generator=gen, dtype=F64)
        m = torch.tensor(cmap)
        want = w.index_select(1, m.clamp(min=0)) * (m >= 0)
        assert torch.equal(sc.pack_cols(w, cmap), want)
        g = torch.randn(rows, len(cmap), generator=gen, dtype=F64)
        gw = torch.zeros(rows, scols, dtype=F64).index_add_(1, m[m >= 0], g[:, m >= 0])
        torch.testing.assert_close(sc.unpack_cols(g, cmap, scols), gw, rtol=1e-14, atol=1e-14)
        off, inv = sc.inverse_map(cmap, scols)
        assert off.tolist()[-1] == int((m >= 0).sum()) and max(off.diff().tolist()) <= 2      # two terms: any order, same bits
        for s in range(scols):
            assert [cmap[j] for j in inv[off[s]:off[s + 1]].tolist()] == [s] * int(off[s + 1] - off[s])


# ---------------------------------------------------------------------------------------------------------------------------
# lattice exactness
# ---------------------------------------------------------------------------------------------------------------------------
def test_lattice_distances_are_exact_in_float32():
    cases = sc.lattice_cases()
    assert len(cases) > 100
    for label, src, dst in cases:
        e64 = sc.sqdist_expanded(src, dst)
        assert torch.equal(sc.sqdist_expanded(src, dst, F32).to(F64), e64), label
        assert torch.equal(sc.sqdist_direct(src, dst, F32).to(F64), e64), label
        assert torch.equal(sc.sqdist_direct(src, dst), e64), label
    # FPS takes the DIRECT distances between the points of its own clouds
    for N in sc.FPS_N:
        for B in sc.fps_Bs(N):
            for kind in ("lattice", "same"):
                x = sc.fps_cloud(kind, B, N)
                for q0 in range(0, N, 512):
                    q = x[:, q0:q0 + 512]
                    assert torch.equal(sc.sqdist_direct(q, x, F32).to(F64), sc.sqdist_direct(q, x)), (kind, N, B)


# ---------------------------------------------------------------------------------------------------------------------------
# path coverage: arithmetic on the case tuples
# ---------------------------------------------------------------------------------------------------------------------------
def test_fps_sizes_reach_every_instantiation_with_a_ragged_last_slot():
    for N in sc.FPS_N:
        assert sc.fps_ppt(N) == sc.FPS_PPT[N]
    for ppt in (1, 2, 4, 8, 16):
        assert any(sc.fps_ppt(N) == ppt and N % 256 for N in sc.FPS_N), ppt          # a last slot that some threads lack
        assert any(sc.fps_ppt(N) == ppt and N < 256 * ppt for N in sc.FPS_N), ppt
    assert {4096, 256} <= set(sc.FPS_N)                                               # and the full sizes


def test_ball_cases_reach_their_paths():
    where = {(len(r2u), r2u.index(max(r2u))) for r2u, _ in sc.BALL_RK}
    assert (2, 0) in where and (3, 1) in where and (4, 3) in where                   # the largest first, in the middle, last
    assert {len(r2u) for r2u, _ in sc.BALL_RK} == {1, 2, 3, 4}
    assert {k for _, ks in sc.BALL_RK for k in ks} >= {1, 16, 63, 64, 65, 128}
    assert all(sum(ks) <= 320 for _, ks in sc.BALL_RK)                                # the front end takes every one of them
    assert any(N < 2048 for N in sc.BALL_N) and 2048 in sc.BALL_N and all(N > 2048 for N in sc.BALL_N_QUERY_ONLY)
    assert -(-sc.BALL_N_QUERY_ONLY[0] // 2048) == 2 and -(-sc.BALL_N_QUERY_ONLY[1] // 2048) == 3
    assert any(S % 4 for S in sc.BALL_S) and any(S % 4 == 0 for S in sc.BALL_S) and max(sc.BALL_S) > 8
    # points exactly on every planted radius, an empty ball, a full ball beside one that never fills
    for N in (65, 2048):
        for r2u, ks in sc.BALL_RK:
            xyz, ctr = sc.ball_case(N, 5, r2u, 3)
            d = sc.sqdist_expanded(ctr, xyz)
            for u, K in zip(r2u, ks):
                n_in = (~(d > u * sc.UNIT2)).sum(-1)
                if u in sc.OFFSETS:
                    assert bool((d[:, :2] == u * sc.UNIT2).any(-1).all()), (N, u)
                assert bool((n_in[:, -1] == 0).all())
                if u == sc.R2_ALL:
                    assert bool((n_in[:, :-1] == N).all())
            if r2u[0] == sc.R2_ALL:                         # the sibling never fills: every candidate passes through the ring
                n_tiny = (~(d > r2u[1] * sc.UNIT2)).sum(-1)
                assert int(n_tiny.max()) < ks[1]
    xyz, ctr = sc.ball_case(*sc.EXACT_K_CASE)
    assert int((~(sc.sqdist_expanded(ctr, xyz) > 0.0)).sum(-1)[0, 0]) == sc.EXACT_K


def test_gather_cases_reach_the_three_kernels():
    for c in sc.GATHER_VECTOR:
        assert sc.gather_path(*c) == "vector" and c[2] == c[0] + 4
        for B in (1, sc.GATHER_B):                          # the last step of the unrolled loop is ragged at both batch sizes
            assert B * sc.GATHER_S * sc.GATHER_K * (c[2] // 4) % 1024
    assert {c[0] for c in sc.GATHER_VECTOR} == {4, 64, 320}
    for c in sc.GATHER_ROW8:
        assert sc.gather_path(*c) == "row8"
    assert {c[0] for c in sc.GATHER_ROW8} == {0, 1, 3, 5}
    for c in sc.GATHER_SCALAR:
        assert sc.gather_path(*c) == "scalar"
    assert (7, 1, 12, 0) in sc.GATHER_SCALAR and any(c[1] == 0 and c[2] == c[0] + 3 and c[2] % 4 for c in sc.GATHER_SCALAR)
    assert any(c[3] % 16 for c in sc.GATHER_SCALAR)


def test_scatter_interpolation_and_fp_rows_cases_cover_what_they_name():
    assert {c[0] for c in sc.SCATTER_CASES} == {1, 3, 64} and {c[3] for c in sc.SCATTER_CASES} == {False, True}
    for C, col0, ld, _ in sc.SCATTER_CASES:
        assert col0 > 0 and ld > col0 + C
    assert {c[0] for c in sc.INTERP_CASES} == {1, 3, 24, 130} and 1 in {c[1] for c in sc.INTERP_CASES}
    assert any(c[2] > 0 and c[3] > 0 for c in sc.INTERP_CASES)
    assert set(sc.FP_ROWS_CASES) == {(D2, D1, pad, N) for D2 in (1, 3, 24, 130) for D1, pad in ((0, 0), (6, 0), (6, 3), (0, 5))
                                     for N in (1, 37)}
    for D2 in (1, 3, 24, 130):                              # every width with D1 0 and 6, kp == D1 + D2 and larger, N = 1
        mine = [c for c in sc.FP_ROWS_CASES if c[0] == D2]
        assert {c[1] for c in mine} == {0, 6} and {c[3] for c in mine} == {1, 37}
        assert {(c[1], c[2] > 0) for c in mine} == {(0, False), (0, True), (6, False), (6, True)}


def test_front_end_cases_reach_their_paths():
    for C in sc.SG_WIDTHS:
        assert sc.row_block(C) == 64 // (C // 4) * 4
        for K in sc.SG_PARTIAL_K:
            assert K % sc.row_block(C) != 0
    seen = set()
    for case in sc.SG_DIRECT + sc.SG_GATHER:
        widths, ks = sc.sg_shape(case[-1])
        assert sum(ks) <= 320
        seen |= {(C, K) for C, K in zip(widths, ks)}
        B, S = (case[2], case[3]) if len(case) == 6 else (case[1], case[2])
        assert sc.waves_per_group(B, S) == 4
    assert seen >= {(C, K) for C in sc.SG_WIDTHS for K in sc.SG_PARTIAL_K}          # every width with every partial K
    widths, ks = sc.SG_FULL
    assert sum(ks) == 320 and all(K % sc.row_block(C) == 0 for C, K in zip(widths, ks))
    assert {c[0] for c in sc.SG_DIRECT} == {0, 3, 6} and {c[1] for c in sc.SG_DIRECT} == {0, 1}
    assert {c[0] for c in sc.SG_GATHER} == {"none", "Y", "slab", "bias"}
    shapes = [c[2:5] for c in sc.SG_DIRECT] + [c[1:4] for c in sc.SG_GATHER]
    assert {s[0] for s in shapes} == {1, 3, 9} and {s[1] for s in shapes} == {1, 5, 9} and {s[2] for s in shapes} == {1, 65, 2048}
    e = sc.SG_EIGHT_WAVE
    assert e["B"] * -(-e["S"] // 8) >= 1024 and sc.waves_per_group(e["B"], e["S"]) == 8
    assert 8 - e["S"] % 8 == 3                                                        # three idle waves in every last workgroup
    assert e["K"] % sc.row_block(e["C"]) != 0


def test_tables_and_weight_gradient_cases_reach_their_paths():
    assert {c[0] for c in sc.TABLES_CASES} == {0, 3, 6, 9} and {c[1] for c in sc.TABLES_CASES} == {0, 1}
    assert {c[3] for c in sc.TABLES_CASES} == {False, True} and {c[2] for c in sc.TABLES_CASES} == {(4, 128), (12, 64, 16)}
    for _, _, widths, _ in sc.TABLES_CASES:
        assert len(set(widths)) > 1                        # threads past a narrower radius' own row count
        for C in widths:
            for B in (1, sc.TABLES_B):
                assert B * (sc.TABLES_N + sc.TABLES_S) * C // 4 % 256
    assert sorted(sc.DW_SHAPES) == [1, 255, 256, 257, 1000]
    for P, (B, S, K) in sc.DW_SHAPES.items():
        assert B * S * K == P and B in (1, 3)
        nb = sc.dw_nblocks(P)
        assert nb[0] == 1 and nb[1] == 3 and nb[2] > -(-P // 256)
    assert {(c[1], c[2]) for c in sc.DW_CASES} == {(C, D) for C in sc.SG_WIDTHS for D in (0, 3, 6)}
    assert {(c[0], c[1]) for c in sc.DW_CASES} == {(P, C) for P in sc.DW_SHAPES for C in sc.SG_WIDTHS}
    assert {c[3] for c in sc.DW_CASES} == {0, 1}


# ---------------------------------------------------------------------------------------------------------------------------
# decision margins
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", sorted(sc.DW_SHAPES))
def test_weight_gradient_cases_keep_the_decision_margin_in_both_precisions(P):
    for c in [c for c in sc.DW_CASES if c[0] == P]:
        case = sc.dw_case(*c)
        assert sc.dw_violations(case) == 0
        u, ok = sc.take_rows(case["U"], case["idx"])
        valid = ok.reshape(-1)
        assert bool((~valid).any()) or P == 1
        assert torch.equal(case["Y1"][valid], (u - case["Vc"].unsqueeze(2)).reshape(P, -1)[valid])      # exact on the grid
        assert torch.equal(case["Y1"].to(F64), (torch.where(ok.unsqueeze(-1), u.to(F64), case["U"][:, :1].unsqueeze(1).to(F64))
                                                - case["Vc"].to(F64).unsqueeze(2)).reshape(P, -1))
        z32 = case["Y1"] * case["scale"] + case["shift"]
        z64 = case["Y1"].to(F64) * case["scale"].to(F64) + case["shift"].to(F64)
        assert torch.equal(z32 > 0, z64 > 0)


def test_chain_case_keeps_the_decision_margin_in_both_precisions():
    c = sc.chain_case()
    f64, f32 = sc.chain_forward(c), sc.chain_forward(c, F32)
    y64, y32 = sc.chain_y1(c, f64).reshape(-1, c["C"]), sc.chain_y1(c, f32).reshape(-1, c["C"])
    assert not bool(bc.act_violations(y64, c["scale"], c["shift"], 0).any())
    assert torch.equal(y32 * c["scale"] + c["shift"] > 0, y64 * c["scale"].to(F64) + c["shift"].to(F64) > 0)
    assert bool((f64["idx"] == c["N"]).all(-1)[:, -1].all()) and int((f64["idx"] < c["N"]).sum()) > 0

"""The float64 restatements of tests/stream_common.py pinned against torch itself: the forward against F.linear behind F.relu,
the backward forms (dA with the (m1, m2) sums, dW, the fused pair; middle layer, max-pooled last layer, by-linearity rows)
against autograd of two conv1x1 + train-mode F.batch_norm + F.relu layers (+ amax), at toy sizes on the CPU -- a wrong
reference cannot then bless a wrong kernel.  Also the slab ownership, the candidates' first-occurrence rule and the
precision-independence of the masks of the GPU cases."""
import pytest
import torch
import torch.nn.functional as Fn

import bn_common as bc
import stream_common as sc
from bn_common import F32, F64

EPS = 1e-5


def close(a, b, tol=1e-11):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
    assert err <= tol, err


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("aff,bias", [(True, True), (False, True), (True, False), (False, False)])
def test_forward_is_linear_behind_relu(layout, aff, bias):
    c = sc.fwd_case(70, 12, 8, layout, aff, bias)
    C, ab = sc.gemm_fwd(c["A"], c["B"], layout, c["scale"], c["shift"], c["bias"])
    x = c["A"].to(F64)
    if aff:
        x = Fn.relu(x * c["scale"].to(F64) + c["shift"].to(F64))
    w = c["B"].to(F64) if layout == 0 else c["B"].to(F64).t()
    close(C, Fn.linear(x, w, None if c["bias"] is None else c["bias"].to(F64)))
    assert bool((ab >= C.abs() * (1 - 1e-12)).all())
    terms = (x.unsqueeze(1) * w.unsqueeze(0)).abs().sum(-1) + (0 if c["bias"] is None else c["bias"].to(F64).abs())
    close(ab, terms)
    if aff:
        assert float(c["scale"][1]) == 0.0 and bool((c["scale"] > 0).any()) and bool((c["scale"] < 0).any())
    assert sc.decision_violations(c) == 0


def test_candidates_are_first_occurrences():
    gen = bc.gen_of(3)
    C = torch.randn(96, 5, generator=gen).to(F32)
    C[40:64] = C[40]                                        # ties inside the second block
    C[70, 2] = C[66, 2] = 9.0
    C[80, 3] = C[95, 3] = -9.0
    vmax, amax, vmin, amin = sc.cand_of(C)
    for blk in range(3):
        for col in range(5):
            v = C[32 * blk:32 * blk + 32, col].tolist()
            assert float(vmax[blk, col]) == max(v) and int(amax[blk, col]) == v.index(max(v))
            assert float(vmin[blk, col]) == min(v) and int(amin[blk, col]) == v.index(min(v))
    assert int(amax[2, 2]) == 2 and int(amin[2, 3]) == 16


def test_gather_rows_is_the_by_linearity_layer_and_an_outside_index_reads_point_zero():
    c = sc.gather_fwd_case(50, 3, 64, 2, 32)
    n, S, rpc, Bs = c["n_points"], c["n_centres"], c["rpc"], c["Bs"]
    assert int((c["idx"] == -1).sum()) == 1 and int((c["idx"] == n).sum()) == 1 and not bool((c["idx"] == n - 1).any())
    y = sc.gather_rows(c["U"], c["Vc"], c["idx"], n, S, rpc)
    idx0 = torch.where((c["idx"] < 0) | (c["idx"] >= n), 0, c["idx"]).view(Bs, S, rpc)
    close(y, bc.gather_linear(c["U"].to(F64), c["Vc"].to(F64), None, idx0).view(-1, 64))
    r = sc.DUP1 + 3                                         # the row whose index is -1: sample 0, centre 1
    close(y[r], c["U"][0, 0].to(F64) - c["Vc"][0, 1].to(F64))


def test_slab_ownership():
    gen = bc.gen_of(4)
    T0, T1 = torch.randn(64 * 5 + 7, 3, generator=gen, dtype=F64), torch.randn(64 * 5 + 7, 3, generator=gen, dtype=F64)
    s = sc.wg_slabs(T0, T1, 4, 6)
    assert s.shape == (6, 2, 3) and not bool(s[4:].any())
    close(s.sum(0), torch.stack([T0.sum(0), T1.sum(0)]))
    close(s[1, 0], T0[64:128].sum(0) + T0[320:].sum(0))      # tiles 1 and 5 (the tail) belong to workgroup 1
    close(s[0, 1], T1[:64].sum(0) + T1[256:320].sum(0))
    assert sc.stream_grid(32768, 128) == 512 and sc.stream_grid(32769, 128) == 512 and sc.stream_grid(32769, 96) == 513
    assert sc.launched_grid(32769, 96, True) == 512 and sc.launched_grid(32769, 96, False) == 513
    assert sc.launched_grid(32769, 64, True) == 513


def _bn_relu(y, gamma, beta):
    return Fn.relu(Fn.batch_norm(y, None, None, gamma, beta, training=True, eps=EPS))


def _finalize(Y, gamma, beta):
    t0, t1 = sc.stats_terms(Y.to(F64))
    tot = sc.wg_slabs(t0, t1, 2, 3).sum(0)
    return bc.bn_finalize(tot[0], tot[1], float(Y.shape[0]), gamma, beta, EPS)


@pytest.mark.parametrize("form", ["middle", "pooled", "gather"])
def test_backward_forms_equal_torch_autograd_in_float64(form):
    gen = bc.gen_of(bc.seed_of(31, len(form)))
    P, Cin, Cout, K = 192, (64 if form == "gather" else 6), 5, 64
    if form == "gather":
        n, S, Bs = 40, 3, 1
        idx = torch.randint(0, n, (P,), generator=gen).to(torch.int32)
        idx[5], idx[P - 1] = -1, n
        U = torch.randn(Bs, n, Cin, generator=gen, dtype=F64).requires_grad_(True)
        Vc = torch.randn(Bs, S, Cin, generator=gen, dtype=F64)
        leaf = U
        i0 = torch.where((idx < 0) | (idx >= n), 0, idx).long()
        yp = U[0, i0] - Vc[0, (torch.arange(P) // K) % S]
        yp.retain_grad()
        Yp = sc.gather_rows(U.detach(), Vc, idx, n, S, K)
        close(Yp, yp.detach(), 0.0)
    else:
        yp = torch.randn(P, Cin, generator=gen, dtype=F64).requires_grad_(True)
        Yp = yp.detach()
    W = (torch.randn(Cout, Cin, generator=gen, dtype=F64) / Cin ** 0.5).requires_grad_(True)
    gam_p, bet_p = bc.signed(Cin, 0.5, 1.5, gen).to(F64), bc.signed(Cin, 0.1, 1.0, gen).to(F64)
    gam, bet = bc.signed(Cout, 0.5, 1.5, gen).to(F64), bc.signed(Cout, 0.1, 1.0, gen).to(F64)

    # torch: two layers and the loss
    y = Fn.linear(_bn_relu(yp, gam_p, bet_p), W)
    z = _bn_relu(y, gam, bet)
    if form == "pooled":
        z = z.view(P // K, K, Cout).amax(1)
    gout = torch.randn(z.shape, generator=gen, dtype=F64)
    (z * gout).sum().backward()

    # restatement: forward tables, then the backward of the upper layer in the kernels' terms
    fp = _finalize(Yp, gam_p, bet_p)
    Y, _ = sc.gemm_fwd(Yp, W.detach(), 0, fp["scale"], fp["shift"])
    close(Y, y.detach())
    f = _finalize(Y, gam, bet)
    if form == "pooled":
        G = P // K
        out, arg = bc.pool_fwd(Y, f["scale"], f["shift"], G, K, 0, 0.0)
        close(out, z.detach())
        Gm = bc.pooled_grad(gout, Y, arg, f["scale"], f["shift"], G, K, 0, 0.0)
    else:
        Gm = bc.masked_grad(gout, Y, f["scale"], f["shift"], 0, 0.0)
    t0, t1 = bc.bwd_terms(Gm, Y, f["mean"], f["invstd"], 0)
    co = bc.bn_bwd_finalize(t0.sum(0), t1.sum(0), float(P), 1, f["scale"], f["mean"], f["invstd"])
    if form == "pooled":
        T = bc.pool_bwd_table(gout, Y, arg, f["scale"], f["shift"], co["a"], G, K, 0.0)
        dY, mag = sc.dy_pooled(Y, arg, T, co["b"], co["d"], K)
        dY0, mag0 = sc.dy_pooled(Y, arg, T, co["b"], co["d"], K, with_d=False)
    else:
        dY, mag = sc.dy_middle(gout, Y, f["scale"], f["shift"], co["a"], co["b"], co["d"])
    assert bool((mag >= dY.abs() * (1 - 1e-12)).all())
    (Gp, gab), (dW, wab) = sc.fused_bwd(dY, mag, W.detach(), Yp, fp["scale"], fp["shift"])
    close(dW, W.grad)
    assert bool((gab >= Gp.abs() * (1 - 1e-12)).all()) and bool((wab >= dW.abs() * (1 - 1e-12)).all())
    # the separate products state the same thing
    close(sc.dgrad(dY, mag, W.detach())[0], Gp, 0.0)
    if form == "pooled":                                    # d folded into the bias by the caller
        close(sc.dgrad(dY0, mag0, W.detach(), bias=co["d"] @ W.detach())[0], Gp)
    out0 = torch.randn(Cout, Cin, generator=gen, dtype=F64)
    close(sc.wgrad(dY, mag, Yp, fp["scale"], fp["shift"], out0)[0], out0 + W.grad)
    # the layer below: (m1, m2) from the slabs of Gp, then its own BatchNorm backward
    r0, r1 = sc.red_terms(Gp, Yp, fp["scale"], fp["shift"], fp["mean"], fp["invstd"])
    tot = sc.wg_slabs(r0, r1, 2, 2).sum(0)
    cp = bc.bn_bwd_finalize(tot[0], tot[1], float(P), 1, fp["scale"], fp["mean"], fp["invstd"])
    dYp = bc.apply_bwd(bc.masked_grad(Gp, Yp, fp["scale"], fp["shift"], 0, 0.0), Yp, cp["a"], cp["b"], cp["d"], 0)
    close(dYp, yp.grad)
    if form == "gather":
        assert leaf.grad is not None


@pytest.mark.parametrize("N,K", sc.SWEEP_PAIRS)
def test_masks_of_the_gpu_cases_do_not_depend_on_the_precision(N, K):
    M = sc.STREAM_MIN + max(sc.T_SWEEP)
    c = sc.fwd_case(M, N, K, 0)
    assert sc.decision_violations(c) == 0
    assert torch.equal(sc.prologue(c["A"], c["scale"], c["shift"], F32) > 0, sc.prologue(c["A"], c["scale"], c["shift"]) > 0)
    assert torch.equal(c["A"][sc.DUP0 + 1], c["A"][sc.DUP1 - 1])      # the duplicated rows survive the nudge
    b = sc.bwd_case(168, 128, N if N != 128 else 64, 0)
    assert sc.decision_violations(b) == 0
    m32 = bc.pre_act(b["Y"], b["scale"], b["shift"], 0, F32) > 0
    assert torch.equal(m32, bc.pre_act(b["Y"], b["scale"], b["shift"], 0) > 0)

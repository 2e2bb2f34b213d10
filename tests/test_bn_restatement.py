"""The float64 restatements of tests/bn_common.py pinned against torch itself (F.batch_norm / F.group_norm + F.leaky_relu + amax
with autograd, float64), the by-linearity forward against the convolution it replaces, and the precision-independence of every
discrete decision on every case of the tables -- all on the CPU."""
import pytest
import torch
import torch.nn.functional as Fn

import bn_common as bc
from bn_common import F32, F64


def close(a, b, tol=1e-11):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
    assert err <= tol, err


@pytest.mark.parametrize("name", [c[0] for c in bc.CHAIN_CASES])
def test_chain_equals_torch_autograd_in_float64(name):
    case = bc.chain_case(name)
    C, P, slope, rps = case["C"], case["P"], case["slope"], case["rps"]
    fin, out, arg = bc.chain_forward(case, case["Y"])
    dY, dgamma, dbeta, doff = bc.chain_backward(case, case["Y"], fin, arg, case["gout"])

    y = case["Y"].to(F64).requires_grad_(True)
    gamma, beta = case["gamma"].to(F64).requires_grad_(True), case["beta"].to(F64).requires_grad_(True)
    off = None
    if case["norm"] == "bn":
        rm, rv = case["rmean"].to(F64).clone(), case["rvar"].to(F64).clone()
        z = Fn.batch_norm(y, rm, rv, gamma, beta, training=True, momentum=bc.BN_MOMENTUM, eps=bc.BN_EPS)
        close(fin["rmean"], rm)
        close(fin["rvar"], rv)
    else:
        x = y.view(case["samples"], rps, C)
        if case["offset"] is not None:
            off = case["offset"].to(F64).requires_grad_(True)
            x = x + off.unsqueeze(1)
        z = Fn.group_norm(x.transpose(1, 2), case["groups"], gamma, beta, bc.GN_EPS).transpose(1, 2).reshape(P, C)
    z = Fn.leaky_relu(z, slope)
    if case["pool"]:
        # amax for the value; its gradient spreads a tie evenly where the layer gives it to the FIRST maximum, so the graph goes
        # through a gather at the restatement's winners, after checking against torch's values that each is a first maximum
        G, K = case["pool"]
        zz = z.view(G, K, C)
        top = zz.amax(1)
        ks = torch.arange(K).view(1, K, 1)
        first = torch.where(zz.detach() == top.detach().unsqueeze(1), ks, K).min(1).values
        live = (top.detach() != 0) | (slope != 0)     # ReLU: a group whose maximum is <= 0 is all zeros and carries no gradient
        assert torch.equal(first[live], arg[live])
        z = torch.gather(zz, 1, arg.unsqueeze(1)).squeeze(1)
        assert torch.equal(z.detach(), top.detach())
        yv = case["Y"].view(G, K, C)
        assert bool((yv.unsqueeze(1) == yv.unsqueeze(2)).all(-1).sum((1, 2)).gt(K).any())     # the case does hold duplicated rows
    close(out, z)
    (z * case["gout"].to(F64)).sum().backward()
    close(dY, y.grad)
    close(dgamma, gamma.grad)
    close(dbeta, beta.grad)
    if off is not None:
        close(doff, off.grad)


def test_bn_eval_mode_backward_is_scale_times_masked_gradient():
    gen = bc.gen_of(11)
    t = bc.rand_tables(1, 8, gen)
    co = bc.bn_bwd_finalize(torch.randn(8, generator=gen), torch.randn(8, generator=gen), 40.0, 0, t["scale"][0], t["mean"][0],
                            t["invstd"][0])
    assert torch.equal(co["a"], t["scale"][0].to(F64)) and not bool(co["b"].any()) and not bool(co["d"].any())


@pytest.mark.parametrize("N,S,K", bc.GATHER_SHAPES[:3])
def test_gather_linear_equals_the_convolution_it_replaces(N, S, K):
    gen = bc.gen_of(N + S + K)
    B, D, C = bc.GATHER_B, 5, 12
    feat, xyz = torch.randn(B, N, D, generator=gen, dtype=F64), torch.randn(B, N, 3, generator=gen, dtype=F64)
    cen = torch.randn(B, S, 3, generator=gen, dtype=F64)
    W, bias = torch.randn(C, D + 3, generator=gen, dtype=F64), torch.randn(C, generator=gen, dtype=F64)
    idx = bc.gather_index(N, S, K, gen)
    ii = idx.long().view(B, S * K, 1)
    grouped = torch.cat([torch.gather(feat, 1, ii.expand(-1, -1, D)).view(B, S, K, D),
                         torch.gather(xyz, 1, ii.expand(-1, -1, 3)).view(B, S, K, 3) - cen.unsqueeze(2)], -1)
    conv = grouped @ W.t() + bias                                   # conv1x1([feat_j | xyz_j - c_g])
    U = torch.cat([feat, xyz], -1) @ W.t()
    Vc = cen @ W[:, D:].t()
    close(bc.gather_linear(U, Vc, bias, idx), conv)
    close(bc.gather_linear(U, Vc, None, idx), conv - bias)


def test_gather_linear_out_of_range_row_is_the_bias_and_has_no_gradient():
    gen = bc.gen_of(5)
    case = bc.gather_case(130, 9, 3, 12, bias=True, oob=True)
    idx, N = case["idx"], case["N"]
    oob = (idx < 0) | (idx >= N)
    assert bool((idx == N).any()) and bool((idx == -1).any())
    y = bc.gather_linear(case["U"].to(F64), case["Vc"].to(F64), case["bias"], idx)
    assert bool((y[oob] == case["bias"].to(F64)).all())
    dY = torch.randn(case["P"], case["C"], generator=gen, dtype=F64)
    dU, dVc = bc.gather_linear_grads(case["U"], case["Vc"], case["bias"], idx, dY)
    dv = dY.view(2, 9, 3, 12) * (~oob).unsqueeze(-1)
    close(dVc, -dv.sum(2))
    ref = torch.zeros(2, N, 12, dtype=F64)
    ref.index_put_((torch.arange(2).view(2, 1, 1).expand(2, 9, 3)[~oob], idx.long()[~oob]), dv[~oob], accumulate=True)
    close(dU, ref)


_CASES = bc.all_cases()


@pytest.mark.parametrize("label", [c[0] for c in _CASES])
def test_decisions_do_not_depend_on_the_precision(label):
    case = dict(_CASES)[label]()
    assert bc.margin_violations(case) == 0
    for d32, d64 in zip(bc.decisions(case, F32), bc.decisions(case, F64)):
        assert int((d32 != d64).sum()) == 0


def test_bars_reject_a_dropped_row_and_a_one_ulp_bias():
    """The two error measures see what the workloads' bars cannot: one row missing from a 300-row column sum, and every element
    one float32 ulp off."""
    gen = bc.gen_of(9)
    Y = torch.randn(300, 12, generator=gen).to(F32)
    r64, r32 = Y.to(F64).sum(0), Y.sum(0)
    absum = Y.to(F64).abs().sum(0)
    rep = bc.Report()
    rep.red("ok", "", r32, r64, r32, absum)
    rep.assert_bars()
    rep.red("dropped", "", Y[:-1].sum(0), r64, r32, absum)
    with pytest.raises(AssertionError):
        rep.assert_bars()
    rep = bc.Report()
    e64 = bc.affine_act(Y, torch.ones(1, 12), torch.zeros(1, 12), 0, 0.2)
    e32 = bc.affine_act(Y, torch.ones(1, 12), torch.zeros(1, 12), 0, 0.2, F32)
    rep.ew("ulp", "", torch.nextafter(torch.nextafter(e32, e32 * 2), e32 * 2), e64, e32)
    assert rep.rows[0][2] > 0
    rep.ew("big", "", e32 * (1 + 2.0 ** -20), e64, e32)
    with pytest.raises(AssertionError):
        rep.assert_bars()

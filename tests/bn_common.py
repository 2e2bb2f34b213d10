"""Restatements of the normalisation / activation / max-pool / by-linearity kernels of csrc/bn.hip (and of the gather form of
csrc/sa_gather_bwd.hip) in plain torch, float64 by default and float32 through `dtype`, the case tables of
tests/test_gpu_norm_pool_guards.py and the comparison helpers.  Written from the definitions in include/prifit_hip.h -- whole
tensor algebra, torch reductions, autograd for the by-linearity backward -- not from the kernels' loops.

Bars (fit_common's convention): a kernel passes when its error against float64 is at most MARGIN x the error of the float32
restatement on the same inputs, the latter floored at 2^-24.  Element-wise outputs are normalised by max |fp64|, reduced
outputs element by element by the float64 sum of the |terms| of that element.

Inputs are built so that float32 and float64 take the same discrete decisions: every activation argument scale y + shift keeps
a relative distance DECISION_MARGIN from 0, and in every pooled (group, channel) the maximum is either ahead of every other
value by that margin or shared by bit-identical values (duplicated rows, a zero scale), where the first one wins in any
precision.  tests/test_bn_restatement.py asserts this on every case of every table."""
import math

import torch

from fit_common import EPS32, F32, F64, MARGIN, bar_of

DECISION_MARGIN = 1e-3
RED_ROWS = 128          # rows per slab of the column reductions (prifit_reduce_rows_per_slab)
POOL_RED_ROWS = 16      # groups per slab of the pooled reduction (prifit_pool_reduce_groups_per_slab)
CS_ROWS = 512           # rows per partial of the column sums


# ---------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------
def _c64(t):
    return torch.as_tensor(t).detach().to("cpu", F64)


def ew_err(a, ref):
    """max |a - ref| / max |ref|"""
    a, ref = _c64(a), _c64(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    d = (a - ref).abs().max().item()
    if not math.isfinite(d):
        return float("inf")
    s = ref.abs().max().item()
    return d / s if s > 0 else d


def red_err(a, ref, absum):
    """max over the elements of |a - ref| / (float64 sum of the |terms| of that element); absolute where that sum is 0"""
    a, ref, absum = _c64(a), _c64(ref), _c64(absum)
    assert a.shape == ref.shape == absum.shape, (a.shape, ref.shape, absum.shape)
    d = (a - ref).abs()
    if not bool(torch.isfinite(d).all()):
        return float("inf")
    return torch.where(absum > 0, d / absum.clamp(min=1e-300), d).max().item()


class Report:
    """(kernel error, float32 restatement's error) per quantity and case; every line is printed before anything is asserted."""

    def __init__(self):
        self.rows = []

    def _add(self, name, case, ek, e32):
        self.rows.append((name, case, ek, e32))
        print("BAR %-14s %-34s kernel %.3e  fp32 %.3e  ratio %7.3f" % (name, case, ek, e32, ek / max(e32, EPS32)))

    def ew(self, name, case, got, r64, r32):
        self._add(name, str(case), ew_err(got, r64), ew_err(r32, r64))

    def red(self, name, case, got, r64, r32, absum):
        self._add(name, str(case), red_err(got, r64, absum), red_err(r32, r64, absum))

    def assert_bars(self):
        bad = [r for r in self.rows if not r[2] <= bar_of(r[3])]
        assert not bad, "above %g x the fp32 restatement's error: %s" % (MARGIN, bad)


# ---------------------------------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------------------------------
def tab(t, P, rps):
    """[P, C]: the table row of every matrix row (rps == 0: one row for all; else row r uses table row r // rps)"""
    t = t.reshape(-1, t.shape[-1])
    if rps == 0:
        return t[:1].expand(P, -1)
    return t.repeat_interleave(rps, 0)[:P]


def act(v, slope):
    return torch.where(v > 0, v, v * slope)


def slab_sums(T0, T1, rows, dtype=F64):
    """[ceil(P / rows)][2][C]: the column sums of the two term matrices over each block of `rows` rows"""
    T0, T1 = T0.to(dtype), T1.to(dtype)
    return torch.stack([torch.stack([T0[r:r + rows].sum(0), T1[r:r + rows].sum(0)]) for r in range(0, T0.shape[0], rows)])


def col_stats(Y, rows=RED_ROWS, dtype=F64):
    """slabs of (sum, sum of squares)"""
    y = Y.to(dtype)
    return slab_sums(y, y * y, rows, dtype)


def bn_finalize(s, q, count, gamma, beta, eps, momentum=0.0, rmean=None, rvar=None, dtype=F64):
    """Column totals -> scale, shift, mean, invstd (biased variance, clamped at 0) and the running statistics (unbiased variance;
    count == 1 has none: the biased one is kept, as the kernel does)."""
    s, q, gamma, beta = (t.to(dtype) for t in (s, q, gamma, beta))
    mean = s / count
    var = (q / count - mean * mean).clamp(min=0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    o = dict(scale=scale, shift=beta - mean * scale, mean=mean, invstd=invstd, var=var)
    if rmean is not None:
        unb = var * count / (count - 1.0) if count > 1 else var
        o["rmean"] = (1.0 - momentum) * rmean.to(dtype) + momentum * mean
        o["rvar"] = (1.0 - momentum) * rvar.to(dtype) + momentum * unb
    return o


def gn_finalize(s, q, groups, count, gamma, beta, eps, offset=None, rows=0.0, dtype=F64):
    """Per-sample column totals s, q [Bs, C] of Y -> per-sample tables of GroupNorm(Y + offset) RELATIVE TO Y (mean' = mean -
    offset, shift' = beta - mean' scale); chsum = the column sums of Y alone."""
    s, q, gamma, beta = (t.to(dtype) for t in (s, q, gamma, beta))
    Bs, C = s.shape
    cpg = C // groups
    off = torch.zeros_like(s) if offset is None else offset.to(dtype)
    q1 = q + 2.0 * off * s + rows * off * off
    s1 = s + rows * off
    gm = s1.view(Bs, groups, cpg).sum(-1) / count
    g2 = q1.view(Bs, groups, cpg).sum(-1) / count
    var = (g2 - gm * gm).clamp(min=0)
    invstd = (1.0 / torch.sqrt(var + eps)).repeat_interleave(cpg, 1)
    mean = gm.repeat_interleave(cpg, 1) - off
    scale = gamma * invstd
    return dict(scale=scale, shift=beta - mean * scale, mean=mean, invstd=invstd, chsum=s)


def affine_act(Y, scale, shift, rps, slope, dtype=F64):
    y = Y.to(dtype)
    return act(y * tab(scale.to(dtype), y.shape[0], rps) + tab(shift.to(dtype), y.shape[0], rps), slope)


def pre_act(Y, scale, shift, rps, dtype=F64):
    y = Y.to(dtype)
    return y * tab(scale.to(dtype), y.shape[0], rps) + tab(shift.to(dtype), y.shape[0], rps)


def pool_fwd(Y, scale, shift, G, K, rps, slope, dtype=F64):
    """-> out [G, C] = max over the K rows of each group of act(scale y + shift), arg [G, C] = the FIRST row that attains it"""
    v = pre_act(Y, scale, shift, rps, dtype).view(G, K, -1)
    vmax = v.max(1).values
    ks = torch.arange(K).view(1, K, 1)
    arg = torch.where(v == vmax.unsqueeze(1), ks, K).min(1).values
    return act(vmax, slope), arg


def masked_grad(G, Y, scale, shift, rps, slope, dtype=F64):
    """Gm = act'(scale y + shift) G"""
    g = G.to(dtype)
    return torch.where(pre_act(Y, scale, shift, rps, dtype) > 0, g, g * slope)


def pooled_grad(gp, Y, arg, scale, shift, G, K, rps, slope, dtype=F64):
    """Gm [G K, C]: the pooled gradient gp [G, C] at the winning row of every (group, channel), through the activation"""
    v = pre_act(Y, scale, shift, rps, dtype).view(G, K, -1)
    a = arg.long().unsqueeze(1)
    gpd = gp.to(dtype).unsqueeze(1)
    gw = torch.where(torch.gather(v, 1, a) > 0, gpd, gpd * slope)
    return torch.zeros_like(v).scatter(1, a, gw).view(G * K, -1)


def bwd_terms(Gm, Y, mean, invstd, rps, dtype=F64):
    """(Gm, Gm yhat), yhat = (Y - mean) invstd: the terms of m1 and m2"""
    y = Y.to(dtype)
    P = y.shape[0]
    return Gm, Gm * ((y - tab(mean.to(dtype), P, rps)) * tab(invstd.to(dtype), P, rps))


def bn_bwd_finalize(m1, m2, count, training, scale, mean, invstd, dtype=F64):
    """dY = a Gm + b Y + d.  train: dY = gamma invstd (Gm - m1 / n - yhat m2 / n); eval: dY = gamma invstd Gm"""
    m1, m2, a, mean, invstd = (t.to(dtype) for t in (m1, m2, scale, mean, invstd))
    if training:
        b = -a * invstd * m2 / count
        d = a * (mean * invstd * m2 / count - m1 / count)
    else:
        b, d = torch.zeros_like(a), torch.zeros_like(a)
    return dict(dgamma=m2, dbeta=m1, a=a, b=b, d=d)


def gn_bwd_finalize(t0, t1, groups, count, gamma, mean, invstd, chsum=None, rows=0.0, dtype=F64):
    """Per-sample totals t0 = sum Gm, t1 = sum Gm yhat [Bs, C] -> cb, cd [Bs, C], S [Bs][2][C], dsum = column sums of dY"""
    t0, t1, gamma, mean, invstd = (t.to(dtype) for t in (t0, t1, gamma, mean, invstd))
    Bs, C = t0.shape
    cpg = C // groups
    m1 = ((gamma * t0).view(Bs, groups, cpg).sum(-1) / count).repeat_interleave(cpg, 1)
    m2 = ((gamma * t1).view(Bs, groups, cpg).sum(-1) / count).repeat_interleave(cpg, 1)
    cb = -(invstd * invstd) * m2
    cd = -invstd * m1 + mean * invstd * invstd * m2
    o = dict(cb=cb, cd=cd, S=torch.stack([t0, t1], 1))
    if chsum is not None:
        o["dsum"] = gamma * invstd * t0 + cb * chsum.to(dtype) + cd * rows
    return o


def param_grads(S, dsum=None, dtype=F64):
    S = S.to(dtype)
    return dict(dbeta=S[:, 0].sum(0), dgamma=S[:, 1].sum(0), db=None if dsum is None else dsum.to(dtype).sum(0))


def apply_bwd(Gm, Y, a, b, d, rps, dtype=F64):
    y = Y.to(dtype)
    P = y.shape[0]
    return tab(a.to(dtype), P, rps) * Gm.to(dtype) + tab(b.to(dtype), P, rps) * y + tab(d.to(dtype), P, rps)


def pool_bwd_table(gp, Y, arg, scale, shift, ca, G, K, slope, dtype=F64):
    """T [G, C] = a act'(v at the winner) gp"""
    v = pre_act(Y, scale, shift, 0, dtype).view(G, K, -1)
    vw = torch.gather(v, 1, arg.long().unsqueeze(1)).squeeze(1)
    g = gp.to(dtype)
    return ca.to(dtype) * torch.where(vw > 0, g, g * slope)


def col_sum(Y, dtype=F64):
    return Y.to(dtype).sum(0)


def col_sum_samples(Y, rps, dtype=F64):
    y = Y.to(dtype)
    return y.view(-1, rps, y.shape[1]).sum(1)


def gather_linear(U, Vc, bias, idx, dtype=F64):
    """Y [B, S, K, C] = U[b, idx[b,s,k]] - Vc[b,s] + bias; an index outside [0, N) gives a row that is the bias alone (neither U
    nor Vc enters it).  Differentiable in U and Vc: the backward arms are tested against autograd of THIS."""
    B, N, C = U.shape
    S, K = idx.shape[1:]
    ok = (idx >= 0) & (idx < N)
    rows = torch.gather(U, 1, torch.where(ok, idx, 0).long().view(B, S * K, 1).expand(-1, -1, C)).view(B, S, K, C)
    y = torch.where(ok.unsqueeze(-1), rows - Vc.unsqueeze(2), torch.zeros((), dtype=U.dtype))
    return y if bias is None else y + bias.to(U.dtype)


def gather_linear_grads(U, Vc, bias, idx, dY, dtype=F64):
    """(dU, dVc) of sum(Y dY) by autograd of gather_linear"""
    u = U.detach().to(dtype).requires_grad_(True)
    v = Vc.detach().to(dtype).requires_grad_(True)
    y = gather_linear(u, v, None if bias is None else bias.to(dtype), idx, dtype)
    (y * dY.detach().to(dtype).view_as(y)).sum().backward()
    return u.grad, v.grad


# ---------------------------------------------------------------------------------------------------------------------------
# inputs whose decisions do not depend on the precision
# ---------------------------------------------------------------------------------------------------------------------------
def gen_of(seed):
    return torch.Generator().manual_seed(seed)


def signed(n, lo, hi, gen):
    """[n] float32 with |x| in [lo, hi) and a random sign"""
    return ((lo + (hi - lo) * torch.rand(n, generator=gen)) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)).to(F32)


def rand_tables(nt, C, gen, zero_scale=None):
    """float32 tables [nt, C]: scale, shift, mean, invstd, a, b, d (a = scale)"""
    t = dict(scale=signed(nt * C, 0.5, 1.5, gen).view(nt, C), shift=signed(nt * C, 0.1, 1.0, gen).view(nt, C),
             mean=(0.5 * torch.randn(nt, C, generator=gen)).to(F32), invstd=(0.5 + 1.5 * torch.rand(nt, C, generator=gen)).to(F32),
             b=(0.1 * torch.randn(nt, C, generator=gen)).to(F32), d=(0.1 * torch.randn(nt, C, generator=gen)).to(F32))
    if zero_scale is not None:
        t["scale"][:, zero_scale] = 0.0
    t["a"] = t["scale"].clone()
    return t


def act_violations(Y, scale, shift, rps, dtype=F64):
    """bool [P, C]: |scale y + shift| is closer to 0 than DECISION_MARGIN (|scale y| + |shift|)"""
    y = Y.to(dtype)
    P = y.shape[0]
    sy, t = y * tab(scale.to(dtype), P, rps), tab(shift.to(dtype), P, rps)
    return (sy + t).abs() < DECISION_MARGIN * (sy.abs() + t.abs())


def nudge_act(Y, scale, shift, rps):
    """float32 Y moved away from the activation's zero crossing wherever it is inside the margin"""
    Y = Y.to(F32).clone()
    for _ in range(20):
        bad = act_violations(Y, scale, shift, rps)
        if not bool(bad.any()):
            return Y
        P = Y.shape[0]
        s, t = tab(scale.to(F64), P, rps), tab(shift.to(F64), P, rps)
        y = Y.to(F64)
        step = 8.0 * DECISION_MARGIN * ((s * y).abs() + t.abs()) / s.abs().clamp(min=1e-30)
        side = torch.where(s * y + t >= 0, 1.0, -1.0) * torch.sign(s)
        Y = torch.where(bad, y + side * step, y).to(F32)
    raise AssertionError("nudge_act did not converge")


def pool_state(Y, scale, shift, G, K, rps, dtype=F64):
    """-> v [G,K,C], vmax, tied [G,K,C] (rows whose Y is bit-identical to the winner's, or scale == 0), the best value outside
    the tied set (-inf if none)"""
    v = pre_act(Y, scale, shift, rps, dtype).view(G, K, -1)
    yv = Y.view(G, K, -1)
    vmax, a = v.max(1)
    ywin = torch.gather(yv, 1, a.unsqueeze(1))
    s0 = tab(scale, G * K, rps).view(G, K, -1) == 0
    tied = (yv == ywin) | s0
    rival = torch.where(tied, torch.full_like(v, -math.inf), v).max(1).values
    return v, vmax, tied, rival


def pool_violations(Y, scale, shift, G, K, rps, dtype=F64):
    """bool [G, C]: the best value outside the winner's tied set is within the margin of the maximum, or the winner's activation
    argument is within the margin of 0"""
    v, vmax, tied, rival = pool_state(Y, scale, shift, G, K, rps, dtype)
    close = vmax - rival < DECISION_MARGIN * (vmax.abs() + rival.abs())
    close &= torch.isfinite(rival)
    sy = (Y.to(dtype) * tab(scale.to(dtype), G * K, rps)).view(G, K, -1)
    t = tab(shift.to(dtype), G * K, rps).view(G, K, -1)
    mag = torch.where(v == vmax.unsqueeze(1), sy.abs() + t.abs(), torch.zeros_like(v)).max(1).values
    return close | (vmax.abs() < DECISION_MARGIN * mag)


def nudge_pool(Y, scale, shift, G, K, rps):
    """float32 Y [G K, C] with the winner's tied set of every violating (group, channel) raised (in activation) until it is ahead
    of the rest and away from 0.  Equal values move together, so duplicated rows stay bit-identical."""
    Y = Y.to(F32).clone()
    C = Y.shape[1]
    for _ in range(40):
        bad = pool_violations(Y, scale, shift, G, K, rps)
        if not bool(bad.any()):
            return Y
        v, vmax, tied, rival = pool_state(Y, scale, shift, G, K, rps)
        s = tab(scale.to(F64), G * K, rps).view(G, K, C)
        rv = torch.where(torch.isfinite(rival), rival.abs(), torch.zeros_like(rival))
        lift = 0.05 * (vmax.abs() + rv + 0.1).unsqueeze(1)
        move = tied & bad.unsqueeze(1) & (s != 0)
        y = Y.to(F64).view(G, K, C)
        Y = torch.where(move, y + lift / s.where(s != 0, torch.ones_like(s)), y).view(G * K, C).to(F32)
    raise AssertionError("nudge_pool did not converge")


def duplicate_rows(Y, G, K, gen, share=0.5):
    """In about `share` of the groups (K >= 2) one row is copied over another: an exact tie wherever that row wins"""
    if K < 2:
        return Y
    yv = Y.view(G, K, -1)
    for g in range(G):
        if float(torch.rand((), generator=gen)) < share:
            i, j = sorted(torch.randperm(K, generator=gen)[:2].tolist())
            yv[g, j] = yv[g, i]
    return Y


# ---------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------
# prifit_col_stats / prifit_bn_relu_bwd_reduce: (P, C, rps, slope)
REDUCE_CASES = ([(P, C, 0, 0.0 if (i + j) % 2 else 0.2) for i, P in enumerate((1, 127, 128, 129, 300))
                 for j, C in enumerate((4, 12, 64, 132, 1024, 1028))]
                + [(3 * r, C, r, sl) for r in (128, 256) for C, sl in ((12, 0.2), (64, 0.0), (1028, 0.2))])
# prifit_affine_relu / prifit_bn_relu_bwd_apply: (P, C, rps, slope)
ELEMENT_CASES = [(P, C, rps, 0.2 if (i + j + k) % 2 else 0.0) for i, P in enumerate((1, 5, 257))
                 for j, C in enumerate((4, 12, 132, 1028)) for k, rps in enumerate((0, 1, 64))]
# prifit_pool_bwd_reduce: (G, K, C, per_sample, slope); per_sample: rows_per_sample = 16 K, two samples (G = 32)
POOL_REDUCE_CASES = ([(G, K, C, False, 0.2 if (i + j) % 2 else 0.0) for i, G in enumerate((1, 15, 16, 17, 33)) for K in (1, 7, 16)
                      for j, C in enumerate((4, 12, 64, 1028))]
                     + [(32, K, C, True, 0.2) for K in (1, 7, 16) for C in (4, 12, 64, 1028)])
# prifit_pool_fwd / _bwd_apply / _bwd_table: (G, K, C, rps in units of K, slope)
POOL_CASES = ([(G, K, C, m, 0.2 if (i + j) % 2 else 0.0) for i, K in enumerate((1, 7, 8, 9, 16)) for j, C in enumerate((4, 12, 64, 1028))
               for G in (1, 3, 40) for m in (0, 1, 4)]
              + [(G, 257, C, m, 0.0) for C in (4, 12) for G, m in ((1, 0), (3, 1), (8, 4))]
              + [(40, 257, 64, 1, 0.2), (3, 300, 64, 1, 0.2), (3, 300, 12, 1, 0.0), (2, 300, 1028, 0, 0.0)])
# prifit_col_sum: (P, C); _samples: rows_per_sample = 512, three samples
COLSUM_CASES = [(P, C) for P in (1, 2, 511, 512, 513, 1025) for C in (4, 12, 1028)]
# finalize kernels: (nslab, C)
FINALIZE_CASES = [(n, C) for n in (1, 3, 256, 257, 1000) for C in (1, 4, 100)]
# GroupNorm finalize kernels: (C, groups, slabs_per_sample, Bs)
GN_CASES = [(C, g, sps, Bs) for C, g in ((4, 4), (12, 3), (64, 2), (256, 1), (1024, 4)) for sps in (1, 3, 9) for Bs in (1, 5)]
# by-linearity layer: (N, S, K), B = 2
GATHER_SHAPES = [(5, 1, 1), (130, 9, 3), (130, 17, 65), (300, 33, 200), (128, 8, 64)]
GATHER_C_GENERIC = (4, 12, 132)
GATHER_C_STAGED = (4, 6, 126, 128)
GATHER_B = 2


def seed_of(*key):
    h = 1469598103
    for k in key:
        h = (h * 1000003 + int(round(float(k) * 10)) + 7) % (1 << 31)
    return h


def element_case(P, C, rps, slope, pad=0):
    """Inputs of the plain (unpooled) kernels: Y, G [P, C], tables [nt, C]; Y nudged against the tables' zero crossings"""
    gen = gen_of(seed_of(1, P, C, rps, slope))
    nt = 1 if rps == 0 else -(-P // rps)
    t = rand_tables(nt, C, gen)
    Y = nudge_act(torch.randn(P, C, generator=gen), t["scale"], t["shift"], rps)
    return dict(kind="plain", P=P, C=C, rps=rps, slope=slope, Y=Y, G=torch.randn(P, C, generator=gen).to(F32), **t)


def pool_case(G, K, C, rps, slope, seed=2):
    """Inputs of the pooled kernels: Y [G K, C], gp [G, C], tables; duplicated rows in half the groups, scale = 0 in channel 1"""
    gen = gen_of(seed_of(seed, G, K, C, rps, slope))
    nt = 1 if rps == 0 else -(-G * K // rps)
    t = rand_tables(nt, C, gen, zero_scale=1)
    Y = duplicate_rows(torch.randn(G * K, C, generator=gen).to(F32), G, K, gen)
    Y = nudge_pool(Y, t["scale"], t["shift"], G, K, rps)
    return dict(kind="pool", G=G, K=K, P=G * K, C=C, rps=rps, slope=slope, Y=Y, gp=torch.randn(G, C, generator=gen).to(F32), **t)


def gather_index(N, S, K, gen, oob=False):
    """[B, S, K] int32: random indices with repeats; every third group is a ball with few points (its first index in most
    slots); oob: entries N and -1 in some slots.  No list names point N - 1: the GPU tests fill the guards around idx with that
    index and its row of U with NaN, so an index read from outside the lists shows in Y, or in a dU row that must stay 0."""
    B = GATHER_B
    idx = torch.randint(0, N - 1, (B, S, K), generator=gen)
    for b in range(B):
        for s in range(0, S, 3):
            keep = max(1, K // 8)
            idx[b, s, keep:] = idx[b, s, 0]
    if K >= 2:
        idx[:, :, K - 1] = idx[:, :, K // 2]        # a duplicate in every group
    if oob:
        flat = idx.view(-1)
        pick = torch.randperm(flat.numel(), generator=gen)[:max(2, flat.numel() // 7)]
        flat[pick[0::2]] = N
        flat[pick[1::2]] = -1
    return idx.to(torch.int32)


def gather_case(N, S, K, C, bias=True, oob=False, slope=0.0):
    """Inputs of the by-linearity layer and its backward arms.  U, Vc, bias, idx; per-channel tables of the BatchNorm behind it
    and G [P, C]; per-sample tables (rps = S K) and gp, arg of the pooled arm.  Vc is resampled until every activation argument
    of the layer's rows keeps the margin."""
    B = GATHER_B
    gen = gen_of(seed_of(3, N, S, K, C, bias, oob))
    idx = gather_index(N, S, K, gen, oob)
    U = torch.randn(B, N, C, generator=gen).to(F32)
    bv = (0.3 * torch.randn(C, generator=gen)).to(F32) if bias else None
    t1, tb = rand_tables(1, C, gen), rand_tables(B, C, gen)
    Vc = torch.randn(B, S, C, generator=gen).to(F32)
    P = B * S * K
    for _ in range(200):
        Y = gather_linear(U.to(F64), Vc.to(F64), bv, idx).view(P, C).to(F32)
        bad = act_violations(Y, t1["scale"], t1["shift"], 0) | act_violations(Y, tb["scale"], tb["shift"], S * K)
        bad = bad.view(B, S, K, C)
        if not bool(bad.any()):
            break
        if bv is not None:      # an out-of-range row is the bias alone
            lone = (bad & ((idx < 0) | (idx >= N)).unsqueeze(-1)).any(0).any(0).any(0)
            bv = torch.where(lone, (0.3 * torch.randn(C, generator=gen)).to(F32), bv)
        bad = bad.any(2)
        Vc = torch.where(bad, torch.randn(B, S, C, generator=gen).to(F32), Vc)
    else:
        raise AssertionError("gather_case did not converge")
    _, arg = pool_fwd(Y, tb["scale"], tb["shift"], B * S, K, S * K, slope)
    return dict(kind="gather", N=N, S=S, K=K, C=C, B=B, P=P, slope=slope, idx=idx, U=U, Vc=Vc, bias=bv, Y=Y, bn=t1, gn=tb,
                arg=arg.to(torch.int32), G=torch.randn(P, C, generator=gen).to(F32),
                gp=torch.randn(B * S, C, generator=gen).to(F32))


# ---------------------------------------------------------------------------------------------------------------------------
# whole layers (the chained tests and their torch anchor)
# ---------------------------------------------------------------------------------------------------------------------------
# (name, norm, P or (G, K), C, groups, samples, slope, offset)
CHAIN_CASES = [
    ("bn", "bn", 300, 132, 0, 1, 0.0, False),
    ("bn_leaky", "bn", 129, 12, 0, 1, 0.2, False),
    ("bn_pool", "bn", (33, 7), 12, 0, 1, 0.0, False),
    ("bn_pool_leaky", "bn", (17, 9), 64, 0, 1, 0.2, False),
    ("gn_offset", "gn", 3 * 128, 64, 2, 3, 0.2, True),
    ("gn", "gn", 2 * 256, 12, 3, 2, 0.0, False),
    ("gn_pool", "gn", (32, 16), 12, 3, 2, 0.2, True),
]
BN_EPS, BN_MOMENTUM, GN_EPS = 1e-5, 0.1, 1e-5


def chain_forward(case, Y, dtype=F64):
    """Y [P, C] (float32 values) -> the layer's tables, output (pooled or not), arg, in `dtype`"""
    C, rps, slope = case["C"], case["rps"], case["slope"]
    y = Y.to(dtype)
    P = y.shape[0]
    if case["norm"] == "bn":
        fin = bn_finalize(y.sum(0), (y * y).sum(0), float(P), case["gamma"], case["beta"], BN_EPS, BN_MOMENTUM, case["rmean"],
                          case["rvar"], dtype)
    else:
        ys = y.view(-1, rps, C)
        fin = gn_finalize(ys.sum(1), (ys * ys).sum(1), case["groups"], float(rps * (C // case["groups"])), case["gamma"],
                          case["beta"], GN_EPS, case["offset"], float(rps), dtype)
    if case["pool"]:
        G, K = case["pool"]
        out, arg = pool_fwd(y, fin["scale"], fin["shift"], G, K, rps, slope, dtype)
    else:
        out, arg = affine_act(y, fin["scale"], fin["shift"], rps, slope, dtype), None
    return fin, out, arg


def chain_backward(case, Y, fin, arg, gout, dtype=F64):
    """-> dY, dgamma, dbeta, doffset (GroupNorm with offset) from the gradient of the layer's output"""
    C, rps, slope = case["C"], case["rps"], case["slope"]
    y = Y.to(dtype)
    P = y.shape[0]
    if case["pool"]:
        G, K = case["pool"]
        Gm = pooled_grad(gout, y, arg, fin["scale"], fin["shift"], G, K, rps, slope, dtype)
    else:
        Gm = masked_grad(gout, y, fin["scale"], fin["shift"], rps, slope, dtype)
    t0, t1 = bwd_terms(Gm, y, fin["mean"], fin["invstd"], rps, dtype)
    if case["norm"] == "bn":
        co = bn_bwd_finalize(t0.sum(0), t1.sum(0), float(P), 1, fin["scale"], fin["mean"], fin["invstd"], dtype)
        return apply_bwd(Gm, y, co["a"], co["b"], co["d"], 0, dtype), co["dgamma"], co["dbeta"], None
    co = gn_bwd_finalize(t0.view(-1, rps, C).sum(1), t1.view(-1, rps, C).sum(1), case["groups"], float(rps * (C // case["groups"])),
                         case["gamma"], fin["mean"], fin["invstd"], fin["chsum"], float(rps), dtype)
    pg = param_grads(co["S"], co["dsum"], dtype)
    return apply_bwd(Gm, y, fin["scale"], co["cb"], co["cd"], rps, dtype), pg["dgamma"], pg["dbeta"], co["dsum"]


def chain_case(name):
    """Inputs of one whole layer, Y nudged until the decisions under the layer's OWN float64 tables keep the margin"""
    _, norm, shape, C, groups, samples, slope, offset = next(c for c in CHAIN_CASES if c[0] == name)
    pool = shape if isinstance(shape, tuple) else None
    P = shape[0] * shape[1] if pool else shape
    gen = gen_of(seed_of(4, P, C, groups, samples, slope))
    case = dict(kind="chain", name=name, norm=norm, P=P, C=C, groups=groups, samples=samples, slope=slope, pool=pool,
                rps=0 if norm == "bn" else P // samples, gamma=signed(C, 0.5, 1.5, gen), beta=signed(C, 0.1, 1.0, gen),
                rmean=(0.1 * torch.randn(C, generator=gen)).to(F32), rvar=(0.5 + torch.rand(C, generator=gen)).to(F32),
                offset=(0.5 * torch.randn(samples, C, generator=gen)).to(F32) if offset else None)
    if pool:
        case["gamma"][1] = 0.0
    Y = (0.3 + 1.5 * torch.randn(P, C, generator=gen)).to(F32)
    if pool:
        Y = duplicate_rows(Y, pool[0], pool[1], gen)
    for _ in range(30):
        fin, _, _ = chain_forward(case, Y)
        sc, sh = fin["scale"].to(F32), fin["shift"].to(F32)
        if pool:
            ok = not bool(pool_violations(Y, fin["scale"], fin["shift"], pool[0], pool[1], case["rps"]).any())
            Y2 = nudge_pool(Y, sc, sh, pool[0], pool[1], case["rps"])
        else:
            ok = not bool(act_violations(Y, fin["scale"], fin["shift"], case["rps"]).any())
            Y2 = nudge_act(Y, sc, sh, case["rps"])
        if ok:
            break
        Y = Y2
    else:
        raise AssertionError("chain_case did not converge")
    case["Y"] = Y
    case["gout"] = torch.randn(pool[0] if pool else P, C, generator=gen).to(F32)
    return case


# ---------------------------------------------------------------------------------------------------------------------------
# the decisions of a case, in two precisions
# ---------------------------------------------------------------------------------------------------------------------------
def decisions(case, dtype):
    """Every discrete decision the kernels take on a case: activation masks and pool winners"""
    if case["kind"] == "plain":
        return [pre_act(case["Y"], case["scale"], case["shift"], case["rps"], dtype) > 0]
    if case["kind"] == "pool":
        G, K, rps = case["G"], case["K"], case["rps"]
        out, arg = pool_fwd(case["Y"], case["scale"], case["shift"], G, K, rps, case["slope"], dtype)
        return [arg, out > 0]
    if case["kind"] == "gather":
        y = gather_linear(case["U"].to(dtype), case["Vc"].to(dtype), case["bias"], case["idx"], dtype).view(case["P"], -1)
        return [pre_act(y, case["bn"]["scale"], case["bn"]["shift"], 0, dtype) > 0,
                pre_act(y, case["gn"]["scale"], case["gn"]["shift"], case["S"] * case["K"], dtype) > 0]
    fin, out, arg = chain_forward(case, case["Y"], dtype)
    if case["pool"]:
        return [arg, out > 0]
    return [pre_act(case["Y"], fin["scale"], fin["shift"], case["rps"], dtype) > 0]


def margin_violations(case):
    """Number of decisions of a case inside the margin (float64)"""
    if case["kind"] == "plain":
        return int(act_violations(case["Y"], case["scale"], case["shift"], case["rps"]).sum())
    if case["kind"] == "pool":
        return int(pool_violations(case["Y"], case["scale"], case["shift"], case["G"], case["K"], case["rps"]).sum())
    if case["kind"] == "gather":
        return int(act_violations(case["Y"], case["bn"]["scale"], case["bn"]["shift"], 0).sum()
                   + act_violations(case["Y"], case["gn"]["scale"], case["gn"]["shift"], case["S"] * case["K"]).sum())
    fin, _, _ = chain_forward(case, case["Y"])
    if case["pool"]:
        return int(pool_violations(case["Y"], fin["scale"], fin["shift"], case["pool"][0], case["pool"][1], case["rps"]).sum())
    return int(act_violations(case["Y"], fin["scale"], fin["shift"], case["rps"]).sum())


def all_cases():
    """(label, builder) of every case of every table"""
    out = []
    for c in sorted(set(REDUCE_CASES + ELEMENT_CASES)):
        out.append(("plain%s" % (c,), lambda c=c: element_case(*c)))
    for G, K, C, m, sl in POOL_CASES:
        out.append(("pool%s" % ((G, K, C, m, sl),), lambda a=(G, K, C, m * K, sl): pool_case(*a)))
    for G, K, C, ps, sl in POOL_REDUCE_CASES:
        out.append(("poolred%s" % ((G, K, C, ps, sl),), lambda a=(G, K, C, 16 * K if ps else 0, sl): pool_case(*a, seed=5)))
    for N, S, K in GATHER_SHAPES:
        for C in sorted(set(GATHER_C_GENERIC + GATHER_C_STAGED)):
            for bias, oob in ((True, False), (False, False), (True, True), (False, True)):
                out.append(("gather%s" % ((N, S, K, C, bias, oob),), lambda a=(N, S, K, C, bias, oob): gather_case(*a)))
    for c in CHAIN_CASES:
        out.append(("chain_" + c[0], lambda n=c[0]: chain_case(n)))
    return out

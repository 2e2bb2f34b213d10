"""Restatements of the primitive-fitting path in plain torch (float64; float32 through `dtype`), the input families of
tests/test_gpu_fit_guards.py and the comparison helpers.  Written from the formulas of the loss (weighted ellipsoid fit with
the CustomSVD backward, ellipsoid / cuboid SDF, the area-proportional sample budget, the Fibonacci and box-surface tables of
oracle/prifit_oracle.py, exact nearest target, the chamfer combination), not from the kernels' structure: batched tensor
algebra over [B, KM] slots, LAPACK's SVD, autograd for every gradient.

Bars: for every continuous quantity the error is max |x - fp64| / max |fp64|; a kernel passes when its error is at most
MARGIN x the error of the float32 restatement of the same formula on the same inputs, with a floor of MARGIN x 2^-24 where
that restatement is (nearly) exact.  tests/test_fit_restatement.py pins the restatements against the reference fixtures and
finite differences, asserts the stated conditions on every input family, and shows that the bars reject wrong formulas."""
import math

import numpy as np
import torch

MARGIN = 4.0
EPS32 = 2.0 ** -24
F64 = torch.float64
F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------------------
# comparison helpers
# ---------------------------------------------------------------------------------------------------------------------------
def rel_err(a, ref64):
    """max |a - ref| / max |ref| (absolute where the reference is all zero)."""
    ref64 = torch.as_tensor(ref64).detach().to("cpu", F64)
    a = torch.as_tensor(a).detach().to("cpu", F64)
    assert a.shape == ref64.shape, (a.shape, ref64.shape)
    if ref64.numel() == 0:
        return 0.0
    scale = ref64.abs().max().item()
    d = (a - ref64).abs().max().item()
    if not math.isfinite(d):
        return float("inf")
    return d / scale if scale > 0 else d


def bar_of(err32):
    return MARGIN * max(err32, EPS32)


def check(name, got, ref64, ref32, report):
    """Record (kernel error, float32 restatement's error) of one quantity and print both with their ratio."""
    ek, e32 = rel_err(got, ref64), rel_err(ref32, ref64)
    report[name] = (ek, e32)
    print("%-22s kernel %.3e  fp32 restatement %.3e  ratio %6.3f  (bar %.3e)" % (name, ek, e32, ek / max(e32, EPS32), bar_of(e32)))
    return ek, e32


def assert_bars(report):
    bad = {k: v for k, v in report.items() if not v[0] <= bar_of(v[1])}
    assert not bad, "above %g x the fp32 restatement's error: %s" % (MARGIN, bad)


# ---------------------------------------------------------------------------------------------------------------------------
# weighted ellipsoid fit
# ---------------------------------------------------------------------------------------------------------------------------
class Svd3(torch.autograd.Function):
    """Batched 3x3 SVD with the reference's CustomSVD backward: dL/dU ignored, 1 / (S_i - S_j) clamped at 1e-6,
    dM = U diag(gS) V^T + 2 U S sym(K^T o (V^T gV)) V^T.  wrong_k: K in place of K^T (a sensitivity mutation)."""

    @staticmethod
    def forward(ctx, M, wrong_k=False):
        U, S, Vh = torch.linalg.svd(M)
        V = Vh.transpose(-2, -1).contiguous()
        ctx.save_for_backward(U, S, V)
        ctx.wrong_k = wrong_k
        return U, S, V

    @staticmethod
    def backward(ctx, gU, gS, gV):
        U, S, V = ctx.saved_tensors
        eye = torch.eye(3, dtype=S.dtype, device=S.device)
        diff = S.unsqueeze(-1) - S.unsqueeze(-2)
        plus = S.unsqueeze(-1) + S.unsqueeze(-2)
        kneg = torch.sign(diff) * diff.abs().clamp(min=1e-6)
        kneg = torch.where(eye.bool(), torch.full_like(kneg, 1e-6), kneg)
        K = (1 / kneg) * (1 / plus) * (1 - eye)
        Kt = K if ctx.wrong_k else K.transpose(-2, -1)
        inner = Kt * (V.transpose(-2, -1) @ gV)
        inner = (inner + inner.transpose(-2, -1)) / 2.0
        out = 2 * U @ torch.diag_embed(S) @ inner @ V.transpose(-2, -1)
        return U @ torch.diag_embed(gS) @ V.transpose(-2, -1) + out, None


def fit64(points, W, count, rnd, canonical, dtype=F64, col_sign=None, mutate=()):
    """Weighted ellipsoid fit of every slot: points [B,N,3], W [B,N,KM] (differentiable), count [B], rnd [3,3] | [B,KM,3,3].
    centre c = sum w p / sum w; cov = sum w q q^T / sum w about it; M = cov + 1e-4 mean(cov) rnd; SVD; canonical: every column
    of V signed so that its largest-magnitude component is positive; third column negated when det V < 0; extents
    r = |max - min| / 2 of the weight-scaled re-centred points w q along the columns of V.  valid = !(S0 / S2 > 1e5).
    Dead slots (k >= count): r = 0, V = I, c = 0, valid = 0.  col_sign [B,KM,3]: a +-1 per column multiplied onto V at the
    end (the SVD leaves the signs free when canonical is off; the caller passes the kernel's choice).
    -> dict r, V, c, valid, live, S, det (before the flip), sign_margin [B,KM,3], ext_margin [B,KM,3]."""
    P = points.to(dtype)
    W = W.to(dtype)
    B, N, _ = P.shape
    KM = W.shape[2]
    dev = P.device
    count = torch.as_tensor(count, device=dev).view(B, 1).long()
    live = torch.arange(KM, device=dev).view(1, KM) < count
    Wl = torch.where(live.unsqueeze(1), W, torch.ones_like(W))          # dead slots: any harmless weights
    Wt = Wl.transpose(1, 2).unsqueeze(-1)                               # [B,KM,N,1]
    sw = Wl.sum(1)                                                      # [B,KM]
    c = torch.einsum("bnk,bnd->bkd", Wl, P) / sw.unsqueeze(-1)
    q = P.unsqueeze(1) - c.unsqueeze(2)                                 # [B,KM,N,3]
    cov = (q * Wt).transpose(-1, -2) @ q / sw.view(B, KM, 1, 1)
    R = rnd.to(dtype)
    R = R.view(1, 1, 3, 3) if R.dim() == 2 else R
    M = cov + 1e-4 * cov.mean(dim=(-1, -2), keepdim=True) * R
    U, S, V = Svd3.apply(M, "svd_k" in mutate)
    Sd = S.detach()
    valid = live & ~(Sd[..., 0] / Sd[..., 2] > 1e5)
    absV = V.detach().abs().sort(dim=-2, descending=True)[0]
    sign_margin = absV[..., 0, :] - absV[..., 1, :]
    if canonical:
        i = V.detach().abs().argmax(dim=-2, keepdim=True)
        V = V * torch.sign(torch.gather(V.detach(), -2, i))
    det = torch.linalg.det(V.detach())
    if "no_flip" not in mutate:
        V = torch.cat([V[..., :2], torch.where((det < 0).view(B, KM, 1, 1), -V[..., 2:], V[..., 2:])], -1)
    if col_sign is not None:
        V = V * col_sign.to(dtype).unsqueeze(-2)
    base = (P - P.mean(1, keepdim=True)).unsqueeze(1).expand_as(q) if "unweighted_centre" in mutate else q
    t = (base * Wt) @ V                                                 # [B,KM,N,3]
    mx, mn = t.max(dim=2)[0], t.min(dim=2)[0]
    r = (mx - mn).abs() / 2.0
    td = t.detach()
    if N >= 2:
        top = td.topk(2, dim=2)[0]
        bot = td.topk(2, dim=2, largest=False)[0]
        ext = (top[:, :, 0] - bot[:, :, 0]).clamp(min=1e-300)
        ext_margin = torch.minimum(top[:, :, 0] - top[:, :, 1], bot[:, :, 1] - bot[:, :, 0]) / ext
    else:
        ext_margin = torch.full_like(r, float("inf"))
    lv = live.unsqueeze(-1)
    eye = torch.eye(3, dtype=dtype, device=dev).expand(B, KM, 3, 3)
    return dict(r=torch.where(lv, r, torch.zeros_like(r)), V=torch.where(lv.unsqueeze(-1), V, eye),
                c=torch.where(lv, c, torch.zeros_like(c)), valid=valid, live=live, S=Sd, det=det,
                sign_margin=sign_margin, ext_margin=ext_margin)


def fit_loss(out, g_r, g_V, g_c):
    """The scalar whose dW the fit's backward returns for seeds (g_r, g_V, g_c): invalid and dead slots contribute nothing."""
    m = out["valid"].to(out["r"].dtype)
    dt = out["r"].dtype
    return ((out["r"] * g_r.to(dt)).sum(-1) * m).sum() + ((out["V"] * g_V.to(dt)).sum((-1, -2)) * m).sum() + \
        ((out["c"] * g_c.to(dt)).sum(-1) * m).sum()


def fit_conditions(out, canonical):
    """The stated conditions on one fit64 result (float64): validity, sign and extreme-row margins on every live slot."""
    live, valid = out["live"], out["valid"]
    cond = (out["S"][..., 0] / out["S"][..., 2])[live]
    assert bool(((cond < 1e3) | (cond > 1e7)).all()), "S0 / S2 between 1e3 and 1e7: %s" % cond[(cond >= 1e3) & (cond <= 1e7)]
    assert bool(((out["det"].abs() - 1).abs() < 1e-9).all())
    assert float(out["sign_margin"][valid].min()) > 1e-3, "canonical sign margin %.3e" % float(out["sign_margin"][valid].min())
    assert float(out["ext_margin"][valid].min()) > 1e-4, "extreme-row margin %.3e" % float(out["ext_margin"][valid].min())
    if canonical:
        d = out["det"][valid]
        assert bool((d < 0).any()) and bool((d > 0).any()), "both branches of the determinant flip must occur"


def _rotations(n, gen):
    Q, Rr = torch.linalg.qr(torch.randn(n, 3, 3, generator=gen, dtype=F64))
    Q = Q * torch.sign(torch.diagonal(Rr, dim1=-2, dim2=-1)).unsqueeze(-2)
    return Q * torch.sign(torch.linalg.det(Q)).view(n, 1, 1)


_ICO = None


def _iso_shell(gen):
    """60 points whose covariance is exactly isotropic (five icosahedra in generic orientations), scaled by (1.002, 1.001, 1):
    singular-value gaps of about 1e-3 of their size."""
    global _ICO
    if _ICO is None:
        p = (1 + 5 ** 0.5) / 2
        v = [(0, s1, s2 * p) for s1 in (-1, 1) for s2 in (-1, 1)]
        v = v + [(b, c, a) for a, b, c in v] + [(c, a, b) for a, b, c in v]
        _ICO = torch.tensor(v, dtype=F64) / (1 + p * p) ** 0.5
    Q = _rotations(5, gen)
    rad = torch.tensor([0.100, 0.105, 0.110, 0.115, 0.120], dtype=F64).view(5, 1, 1)
    pts = (rad * (_ICO.unsqueeze(0) @ Q.transpose(1, 2))).reshape(60, 3)
    return pts * torch.tensor([1.002, 1.001, 1.0], dtype=F64)


# (name, N, KM, count, rnd "shared" | "slot", canonical, family, seed).  Seeds: the first for which every stated condition
# holds on every slot (tests/test_fit_restatement.py asserts them).
FIT_CASES = [
    ("n40_soft", 40, 4, (3,), "shared", 1, "soft", 0),
    ("n5_soft", 5, 32, (0, 1, 32), "shared", 1, "soft", 0),
    ("n255_hard", 255, 32, (0, 1, 32), "slot", 1, "hard", 1),
    ("n256_soft64", 256, 64, (40, 64), "shared", 1, "soft", 2),
    ("n257_soft", 257, 32, (0, 1, 32), "slot", 0, "soft", 0),
    ("n256_hard_b1", 256, 32, (7,), "shared", 0, "hard", 0),
    ("n700_special", 700, 32, (0, 1, 32), "shared", 1, "special", 0),
    ("n700_soft64", 700, 64, (40, 64), "slot", 1, "soft", 8),
]
ISO_SLOT, PLANE_SLOT = 3, 5     # of the last shape of the "special" family


def fit_case(name):
    """-> dict points [B,N,3], W [B,N,KM], count, rnd, canonical, g_r, g_V, g_c (float32 / int32, on the CPU)."""
    _, N, KM, count, rmode, canonical, family, seed = next(c for c in FIT_CASES if c[0] == name)
    gen = torch.Generator().manual_seed(1000 * seed + N + KM)
    B = len(count)
    P = torch.zeros(B, N, 3, dtype=F64)
    W = torch.zeros(B, N, KM, dtype=F64)
    for b, K in enumerate(count):
        Kg = max(K, 1)
        lab = torch.arange(N) % Kg
        lab = lab[torch.randperm(N, generator=gen)]
        if N < 4 * Kg:                                  # fewer rows than clusters could hold: one cloud, mild weights
            P[b] = 0.3 * torch.randn(N, 3, generator=gen, dtype=F64)
            sharp, noise = 0.0, 1.0
        else:
            cen = 1.2 * torch.rand(Kg, 3, generator=gen, dtype=F64) - 0.6
            sc = (0.04 + 0.06 * torch.rand(Kg, 1, generator=gen, dtype=F64)) * \
                torch.tensor([1.0, 0.7, 0.45], dtype=F64) * (0.85 + 0.3 * torch.rand(Kg, 3, generator=gen, dtype=F64))
            Q = _rotations(Kg, gen)
            z = torch.randn(N, 3, generator=gen, dtype=F64) * sc[lab]
            P[b] = cen[lab] + (Q[lab] @ z.unsqueeze(-1)).squeeze(-1)
            sharp, noise = 4.0, 0.5
        if family == "special" and K == KM:
            # hard labels: slot ISO_SLOT <- 60 shell points, slot PLANE_SLOT <- 40 points in a plane normal to (1, 1, 1) (so that
            # mean(cov) = 0 and the random table cannot lift the smallest singular value), the rest 20 each
            lab = torch.cat([torch.full((60,), ISO_SLOT), torch.full((40,), PLANE_SLOT),
                             torch.tensor([k for k in range(K) if k not in (ISO_SLOT, PLANE_SLOT)]).repeat_interleave(20)])
            assert lab.numel() == N
            z = torch.randn(N, 3, generator=gen, dtype=F64) * sc[lab]
            P[b] = cen[lab] + (Q[lab] @ z.unsqueeze(-1)).squeeze(-1)
            P[b, :60] = cen[ISO_SLOT] + _iso_shell(gen)
            e1 = torch.tensor([1.0, -1.0, 0.0], dtype=F64) / 2 ** 0.5
            e2 = torch.tensor([1.0, 1.0, -2.0], dtype=F64) / 6 ** 0.5
            ab = torch.randn(40, 2, generator=gen, dtype=F64) * torch.tensor([0.08, 0.05], dtype=F64)
            P[b, 60:100] = torch.tensor([0.25, -0.125, 0.5], dtype=F64) + ab[:, :1] * e1 + ab[:, 1:] * e2
        if K == 0:
            continue
        if family in ("hard", "special"):
            W[b, torch.arange(N), lab] = 1.0
        else:
            score = sharp * torch.nn.functional.one_hot(lab, Kg).to(F64) + noise * torch.randn(N, Kg, generator=gen, dtype=F64)
            W[b, :, :K] = torch.softmax(score, dim=1)
    rnd = torch.rand((3, 3) if rmode == "shared" else (B, KM, 3, 3), generator=gen, dtype=F64)
    seeds = [torch.randn(B, KM, *s, generator=gen, dtype=F64) for s in ((3,), (3, 3), (3,))]
    f = lambda t: t.to(F32)
    return dict(points=f(P), W=f(W), count=torch.tensor(count, dtype=torch.int32), rnd=f(rnd), canonical=canonical,
                g_r=f(seeds[0]), g_V=f(seeds[1]), g_c=f(seeds[2]), family=family)


def fit_reference(case, dtype=F64, col_sign=None, mutate=(), device="cpu"):
    """fit64 + autograd on one case -> (out dict, dW)."""
    d = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in case.items()}
    W = d["W"].detach().to(dtype).clone().requires_grad_(True)
    out = fit64(d["points"], W, d["count"], d["rnd"], d["canonical"], dtype, col_sign, mutate)
    fit_loss(out, d["g_r"], d["g_V"], d["g_c"]).backward()
    return {k: v.detach() for k, v in out.items()}, W.grad


# ---------------------------------------------------------------------------------------------------------------------------
# signed distances
# ---------------------------------------------------------------------------------------------------------------------------
def sdf64(kind, points, r, V, c, dtype=F64, mutate=()):
    """Signed distance of every point to every slot's primitive, [B,M,KM] (dead slots are the caller's to mask).
    q = V^T (p - c).  ellipsoid: k0 = |q / (r + 1e-6)|, k1 = |q / (r^2 + 1e-6)|, k0 (k0 - 1) / (k1 + 1e-6);
    cuboid (half-sides r): t = |q| - r, |relu(t)| + min(max t, 0), the maximum taken at its first index."""
    P, r, V, c = (x.to(dtype) for x in (points, r, V, c))
    d = P.unsqueeze(2) - c.unsqueeze(1)                                 # [B,M,KM,3]
    q = torch.einsum("bkia,bmki->bmka", V, d)
    ru = r.unsqueeze(1)
    if kind == "ellipsoid":
        k0 = torch.linalg.vector_norm(q / (ru + 1e-6), dim=-1)
        k1 = torch.linalg.vector_norm(q / (ru * ru + 1e-6), dim=-1)
        return k0 * (k0 - 1.0) / (k1 + 1e-6)
    t = q.abs() - ru
    nrm = torch.linalg.vector_norm(torch.relu(t), dim=-1)
    eq = t.detach() == t.detach().max(dim=-1, keepdim=True)[0]
    first = eq & (eq.cumsum(-1) == 1)
    inner = torch.clamp((t * first).sum(-1), max=0.0)
    return nrm + (inner.detach() if "no_plus_one" in mutate else inner)


def sdf_reduce(mat, valid):
    """-> dict absmin [B,M] (0 where no slot is valid), arg (-1 there), fval (signed value at arg), sum_sq [B], full (the
    matrix with 0 in dead slots), clear [B,M] (best and second-best |sdf| more than 1e-4 apart, relative)."""
    ok = (valid != 0).unsqueeze(1)
    a = mat.abs().masked_fill(~ok, float("inf"))
    has = ok.any(-1)
    best, arg = a.min(-1)
    fval = torch.where(has, torch.gather(mat, 2, arg.unsqueeze(-1)).squeeze(-1), torch.zeros_like(best))
    arg = torch.where(has, arg, torch.full_like(arg, -1))
    if a.shape[-1] >= 2:
        two = a.detach().topk(2, dim=-1, largest=False)[0]
        clear = ~((two[..., 1] - two[..., 0]) <= 1e-4 * two[..., 1])
    else:
        clear = torch.ones_like(has)
    return dict(absmin=fval.abs(), arg=arg, fval=fval, sum_sq=(fval * fval).sum(1), full=mat * ok, clear=clear | ~has)


PLACED = 8      # rows of shape 0 that sdf_case places (M >= 255)


def prims(B, KM, live, gen, nan_dead=True):
    """Random primitives: r in [0.05, 0.3], V a rotation, c in [-0.5, 0.5]; live: per shape the list of valid slots.  Dead
    slots hold NaN (nothing may read them)."""
    r = 0.05 + 0.25 * torch.rand(B, KM, 3, generator=gen, dtype=F64)
    V = _rotations(B * KM, gen).view(B, KM, 3, 3)
    c = torch.rand(B, KM, 3, generator=gen, dtype=F64) - 0.5
    valid = torch.zeros(B, KM, dtype=torch.int32)
    for b, ks in enumerate(live):
        valid[b, list(ks)] = 1
    if nan_dead:
        dead = valid == 0
        r[dead], V[dead], c[dead] = float("nan"), float("nan"), float("nan")
    return r, V, c, valid


SDF_CASES = [(M, 32) for M in (1, 255, 257, 1000)] + [(300, 64)]


def sdf_case(kind, M, KM, seed=0):
    """B = 2: shape 0 with live slots {0, 3, 31} (KM = 32) or the first 40 (KM = 64), shape 1 without a valid slot.  Slot 0
    of shape 0 is axis-aligned with dyadic r and c, slot 3 has r of about 1e-3.  The first PLACED targets of shape 0 (M >= 255)
    sit exactly at a centre, on a face, an edge and a vertex of slot 0, deep inside and far outside, and around the tiny slot."""
    gen = torch.Generator().manual_seed(7000 + 10 * M + KM + seed + (0 if kind == "ellipsoid" else 1))
    live0 = (0, 3, 31) if KM == 32 else tuple(range(40))
    r, V, c, valid = prims(2, KM, [live0, ()], gen)
    r[0, 0] = torch.tensor([0.125, 0.25, 0.0625], dtype=F64)
    V[0, 0] = torch.eye(3, dtype=F64)
    c[0, 0] = torch.tensor([0.25, -0.5, 0.125], dtype=F64)
    r[0, 3] = torch.tensor([1e-3, 2e-3, 1.5e-3], dtype=F64)
    T = 1.6 * torch.rand(2, M, 3, generator=gen, dtype=F64) - 0.8
    if M >= 255:
        r0, c0, big = r[0, 0], c[0, 0], live0[-1]
        T[0, 0] = c0
        T[0, 1] = c0 + r0 * torch.tensor([1.0, 0.5, -0.25], dtype=F64)           # on the +x face
        T[0, 2] = c0 + r0 * torch.tensor([1.0, -1.0, 0.5], dtype=F64)            # on an edge
        T[0, 3] = c0 + r0                                                        # a vertex
        T[0, 4] = c[0, big] + V[0, big] @ (0.05 * r[0, big])                     # deep inside
        T[0, 5] = torch.tensor([3.0, -3.0, 3.0], dtype=F64)                      # far outside
        T[0, 6] = c[0, 3]                                                        # centre of the tiny slot
        T[0, 7] = c[0, 3] + torch.tensor([2e-3, 0.0, 0.0], dtype=F64)            # a radius away from it
    g = torch.randn(2, M, KM, generator=gen, dtype=F64)
    g[torch.rand(2, M, KM, generator=gen) < 0.3] = 0.0                           # exact zeros; dead slots keep non-zero values
    f = lambda t: t.to(F32)
    return dict(kind=kind, targets=f(T), r=f(r), V=f(V), c=f(c), valid=valid, g=f(g),
                gscale=f(0.5 + torch.rand(2, generator=gen, dtype=F64)), placed=PLACED if M >= 255 else 0)


def clean(x):
    """NaN (dead slots) -> 0, for a restatement that evaluates every slot and masks afterwards."""
    return torch.nan_to_num(x, nan=0.0)


def sdf_reference(case, dtype=F64, arg=None, mutate=(), device="cpu"):
    """Forward quantities and the gradients of (a) sum_b gscale[b] sum_sq[b] with the slot of every point fixed to `arg`
    (default: this evaluation's own argmin) and (b) sum(g * full): -> (reduce dict, grads_a, grads_b), grads = (g_r, g_V, g_c)."""
    d = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in case.items()}
    leaves = [clean(d[k]).to(dtype).requires_grad_(True) for k in ("r", "V", "c")]
    mat = sdf64(d["kind"], d["targets"], *leaves, dtype=dtype, mutate=mutate)
    red = sdf_reduce(mat, d["valid"])
    use = red["arg"] if arg is None else arg.to(device).long()
    fv = torch.where(use >= 0, torch.gather(mat, 2, use.clamp(min=0).unsqueeze(-1)).squeeze(-1), torch.zeros_like(red["fval"]))
    ga = torch.autograd.grad(((fv * fv).sum(1) * d["gscale"].to(dtype)).sum(), leaves, retain_graph=True, allow_unused=True)
    gb = torch.autograd.grad((red["full"] * d["g"].to(dtype)).sum(), leaves, allow_unused=True)
    z = lambda gs: tuple(torch.zeros_like(l) if g is None else g for g, l in zip(gs, leaves))
    return {k: v.detach() for k, v in red.items()}, z(ga), z(gb)


# ---------------------------------------------------------------------------------------------------------------------------
# sample budget, surface tables, nearest target
# ---------------------------------------------------------------------------------------------------------------------------
def budget64(kind, r, valid, cap, dtype=F64, mutate=()):
    """Samples per slot.  area: ellipsoid 4 * 3.142 * ((ab)^p + (bc)^p + (ca)^p)^(1/p), p = 1.585; cuboid 8 (ab + bc + ca).
    n = round-half-even(10000 area / total); n <= 0 -> 100; then, in slot order, n = cap - off where off + n would pass cap.
    -> n [B,KM] int32, off [B,KM+1] int32, frac [B,KM] float64 (10000 area / total, 0 in dead slots)."""
    npd = np.float64 if dtype == F64 else np.float32
    rr = np.nan_to_num(r.detach().cpu().numpy().astype(npd))
    ok = valid.cpu().numpy() != 0
    a, b, c = rr[..., 0], rr[..., 1], rr[..., 2]
    if kind == "cuboid":
        area = npd(8.0) * (a * b + b * c + c * a)
    else:
        p = npd(1.585)
        area = npd(4.0) * npd(3.142) * ((a * b) ** p + (b * c) ** p + (c * a) ** p) ** (npd(1.0) / p)
    area = np.where(ok, area.astype(np.float64), 0.0)
    B, KM = ok.shape
    n = np.zeros((B, KM), np.int32)
    off = np.zeros((B, KM + 1), np.int32)
    frac = np.zeros((B, KM))
    for bb in range(B):
        total, o = area[bb].sum(), 0
        for k in range(KM):
            if ok[bb, k]:
                frac[bb, k] = 10000.0 * (area[bb, k] / total)
                v = int(np.rint(frac[bb, k]))
                if v <= 0 and "no_hundred" not in mutate:
                    v = 100
                if o + v > cap:
                    v = cap - o
                n[bb, k] = v
            off[bb, k] = o
            o += n[bb, k]
        off[bb, KM] = o
    return torch.from_numpy(n), torch.from_numpy(off), torch.from_numpy(frac)


def budget_conditions(frac, valid):
    f = frac[valid != 0]
    away = ((f - 0.5) - torch.round(f - 0.5)).abs()       # distance to the nearest half-integer
    assert float(away.min()) >= 0.01 and float((f - 0.5).abs().min()) >= 0.01, "a budget within 0.01 of a rounding boundary"


def fib_dir(j, n):
    """Fibonacci direction j of n: z = 1 - (2j + 1) / n, longitude 2 pi frac(j / phi) -> cos lon, sin lon, z, sqrt(1 - z^2)."""
    j = np.arange(n, dtype=np.float64) if j is None else j
    z = 1.0 - (2.0 * j + 1.0) / n
    lon = 2.0 * np.pi * np.modf(j * 0.6180339887498949)[0]
    return np.cos(lon), np.sin(lon), z, np.sqrt(np.maximum(0.0, 1.0 - z * z))


def cuboid_unit(n, a, b, c):
    """Box-surface parameter j of n for half-sides (a, b, c): the face whose slice of the cumulative area [+z, -z, +x, -x, +y,
    -y] holds (j + 0.5) / n, the free coordinates from the R2 sequence; scaled (v s) / (s + 1e-6).  float64 [n,3]."""
    w = [a * b, a * b, b * c, b * c, c * a, c * a]
    total = 0.0
    for f in range(6):
        total += w[f]
    j = np.arange(n, dtype=np.float64)
    t = (j + 0.5) / n
    face = np.zeros(n, dtype=np.int64)
    run = 0.0
    for f in range(5):
        run += w[f]
        face[t >= run / total] = f + 1
    s1 = 2.0 * np.modf(0.5 + j * 0.7548776662466927)[0] - 1.0
    s2 = 2.0 * np.modf(0.5 + j * 0.5698402909980532)[0] - 1.0
    sg = np.where(face % 2 == 1, -1.0, 1.0)
    v = np.empty((n, 3))
    zf, xf, yf = face < 2, (face >= 2) & (face < 4), face >= 4
    v[zf] = np.stack([s1[zf], s2[zf], sg[zf]], 1)
    v[xf] = np.stack([sg[xf], s1[xf], s2[xf]], 1)
    v[yf] = np.stack([s2[yf], sg[yf], s1[yf]], 1)
    side = np.array([[a, b, c]])
    return (v * side) / (side + 1e-6)


def samples64(kind, r, V, c, n, off, dtype=F64, mutate=()):
    """Surface samples of every shape: sample s of slot k (off[k] <= s < off[k] + n[k]) is V_k (r_k * u) + c_k with u the unit
    parameter s - off[k] of n[k] (Fibonacci direction | box-surface table, constants of the graph).  The tables are formed
    in float64 and rounded to `dtype`.  -> pts [B,S,3] (S = the largest total; zeros behind a shape's total), slot [B,S] (-1)."""
    r_, V_, c_ = (clean(x).to(dtype) for x in (r, V, c))
    dev = r_.device
    B, KM = n.shape
    nn, oo = n.cpu().numpy(), off.cpu().numpy()
    S = int(oo[:, KM].max())
    pts, slot = [], torch.full((B, max(S, 1)), -1, dtype=torch.long)
    for b in range(B):
        rows = []
        for k in range(KM):
            nk = int(nn[b, k])
            if nk <= 0:
                continue
            if kind == "cuboid":
                a, bb, cc = (float(x) for x in r_[b, k].detach().float().cpu())
                u = torch.from_numpy(cuboid_unit(nk, a, bb, cc)).to(dtype)
            else:
                cu, su, cv, sv = (torch.from_numpy(x).to(dtype) for x in fib_dir(None, nk))
                u = torch.stack([cu * sv, su * sv, cv], 1)
            ks = k
            if "slot_before_empty" in mutate and k > 0 and nn[b, k - 1] == 0:
                ks = k - 1                                  # the wrong walk: the sample lands in the empty slot in front
            rows.append((u.to(dev) * r_[b, ks]) @ V_[b, ks].transpose(0, 1) + c_[b, ks])
            slot[b, oo[b, k]:oo[b, k] + nk] = k
        rows.append(torch.zeros(max(S, 1) - int(oo[b, KM]), 3, dtype=dtype, device=dev))
        pts.append(torch.cat(rows, 0))
    return torch.stack(pts), slot.to(dev)


def nearest64(pts, total, targets, dtype=F64, last=False, chunk=512):
    """Exact nearest target of every live sample (s < total[b]), the first index on ties (last=True: the wrong rule).
    -> idx [B,S] (-1 on dead rows), d2 [B,S] (0 there), sum_d2 [B]."""
    P, T = pts.detach().to(dtype), targets.to(dtype)
    B, S, _ = P.shape
    M = T.shape[1]
    idx = torch.full((B, S), -1, dtype=torch.long, device=P.device)
    d2 = torch.zeros(B, S, dtype=dtype, device=P.device)
    for b in range(B):
        nb = int(total[b])
        for s0 in range(0, nb, chunk):
            s1 = min(nb, s0 + chunk)
            d = ((P[b, s0:s1, None, :] - T[b, None, :, :]) ** 2).sum(-1)
            i = (M - 1 - d.flip(1).argmin(1)) if last else d.argmin(1)
            idx[b, s0:s1] = i
            d2[b, s0:s1] = torch.gather(d, 1, i.unsqueeze(1)).squeeze(1)
    return idx, d2, d2.sum(1)


def dist_to(pts, idx, targets):
    """Squared distance of every sample to targets[idx] (0 where idx < 0), differentiable in pts."""
    T = targets.to(pts.dtype)
    t = torch.gather(T, 1, idx.clamp(min=0).unsqueeze(-1).expand(-1, -1, 3))
    return ((pts - t) ** 2).sum(-1) * (idx >= 0)


def dup_pairs(M):
    """(original, copy) target rows, original < copy, placed against the search's structure (8 ranges of ceil(M / 8) targets,
    LDS tiles of 1024, groups of four counted from the start of a tile): same group, adjacent groups, adjacent ranges,
    adjacent tiles of one range, the short last group."""
    chunk = -(-M // 8)
    want = [(0, 2), (3, 4), (chunk - 1, chunk), (chunk + 1, chunk + 3), (2 * chunk + 3, 2 * chunk + 4), (1023, 1024),
            (chunk + 1023, chunk + 1024), (M - 2, M - 1), (5, 6)]
    used, out = set(), []
    for a, b in want:
        if 0 <= a < b < M and a not in used and b not in used:
            used.update((a, b))
            out.append((a, b))
    return out


NN_LIVE = {32: [(0,), (0, 3, 31), (), tuple(range(32))], 64: [tuple(range(40)), ()]}
NN_M = (1, 7, 8, 1000, 1030, 8200)


def nn_case(kind, M, KM, cap, seed=0):
    """Primitives with live slots {0}, {0, 3, 31}, none, all 32 (KM = 32) or the first 40 and none (KM = 64); slot 0 of the
    {0, 3, 31} shape is tiny (its share of the budget rounds to 0 -> 100 samples).  Targets: uniform around the primitives;
    then, for every pair of dup_pairs(M), both rows are set to (the float32 image of) one surface sample of every shape that
    has samples, so that the float64 nearest target of that sample is a duplicated row."""
    gen = torch.Generator().manual_seed(9000 + 10 * M + KM + seed + (0 if kind == "ellipsoid" else 1))
    live = NN_LIVE[KM]
    B = len(live)
    for _ in range(256):    # the first draw whose budgets are clear of every rounding boundary (budget_conditions)
        r, V, c, valid = prims(B, KM, live, gen)
        if KM == 32:
            r[1, 0] = torch.tensor([2e-4, 4e-4, 3e-4], dtype=F64)
        try:
            for cp in {cap, 600}:
                budget_conditions(budget64(kind, r.to(F32), valid, cp)[2], valid)
            break
        except AssertionError:
            continue
    T = 1.6 * torch.rand(B, M, 3, generator=gen, dtype=F64) - 0.8
    r, V, c = r.to(F32), V.to(F32), c.to(F32)
    n, off, frac = budget64(kind, r, valid, cap)
    pts, _ = samples64(kind, r, V, c, n, off)
    pairs = dup_pairs(M)
    for b in range(B):
        tot = int(off[b, KM])
        for i, (a, bb) in enumerate(pairs):
            if tot:
                T[b, a] = T[b, bb] = pts[b, (i * 37 + 11) % tot].to(F32).to(F64)
    return dict(kind=kind, r=r, V=V, c=c, valid=valid, targets=T.to(F32), cap=cap, pairs=pairs, frac=frac,
                gscale=(0.5 + torch.rand(B, generator=gen, dtype=F64)).to(F32))


def nn_reference(case, dtype=F64, idx=None, mutate=(), device="cpu", last=False):
    """Budget, samples, nearest target and the gradients of sum_b gscale[b] sum_s |sample - targets[idx]|^2 with the neighbour
    fixed to `idx` (default: this evaluation's own) -> dict n, off, total, pts, slot, idx, d2, sum_d2, grads (g_r, g_V, g_c)."""
    d = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in case.items()}
    KM = d["valid"].shape[1]
    n, off, _ = budget64(d["kind"], d["r"], d["valid"], d["cap"], dtype, mutate)
    leaves = [clean(d[k]).to(dtype).requires_grad_(True) for k in ("r", "V", "c")]
    pts, slot = samples64(d["kind"], *leaves, n, off, dtype, mutate)
    total = off[:, KM]
    own, d2, s = nearest64(pts, total, d["targets"], dtype, last)
    use = own if idx is None else torch.where(own >= 0, idx.to(device).long()[:, :own.shape[1]], own)
    loss = (dist_to(pts, use, d["targets"]).sum(1) * d["gscale"].to(dtype)).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True) if loss.requires_grad and int(total.sum()) else [None] * 3
    grads = tuple(torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves))
    return dict(n=n, off=off, total=total, pts=pts.detach(), slot=slot, idx=own, d2=d2, sum_d2=s, grads=grads)


# ---------------------------------------------------------------------------------------------------------------------------
# small reductions
# ---------------------------------------------------------------------------------------------------------------------------
def combine64(d2_sum, total, sdf_sum, valid, M, dtype=F64):
    """Per shape pd = d2_sum / max(total, 1), ps = sdf_sum / M; loss = mean over the shapes with a valid slot of (pd + ps) / 2
    (0 when none has) -> loss, pd, ps.  Differentiable in d2_sum and sdf_sum."""
    has = (valid != 0).any(1)
    pd = d2_sum.to(dtype) / total.clamp(min=1).to(dtype)
    ps = sdf_sum.to(dtype) / float(M)
    per = torch.where(has, (pd + ps) / 2.0, torch.zeros_like(pd))
    return per.sum() / max(int(has.sum()), 1), pd, ps


def assert_exact(name, got, ref):
    """Integer results (budget, offsets, indices, flags): equal element for element."""
    got, ref = torch.as_tensor(got).detach().cpu().long(), torch.as_tensor(ref).detach().cpu().long()
    assert got.shape == ref.shape and torch.equal(got, ref), "%s: %d element(s) differ, first %s" % (
        name, int((got != ref).sum()) if got.shape == ref.shape else -1,
        (got != ref).nonzero()[:1].tolist() if got.shape == ref.shape else "(shape)")


def check_neighbours(name, idx, ref, d2_32, targets, pairs, report):
    """The nearest-target indices `idx` [B, >= S] against the float64 search `ref` (nn_reference): in range on every live
    sample; where the float64 nearest target is a duplicated row, exactly the lower index of the pair; elsewhere accepted
    when the float64 distance from the float64 sample to targets[idx] exceeds the float64 minimum by no more than the bar
    (recorded in `report` as the excess relative to the largest minimum, next to the float32 restatement's distance error)."""
    own = ref["idx"].cpu()
    S, M = own.shape[1], targets.shape[1]
    idx = idx.detach().cpu().long()[:, :S]
    live = own >= 0
    assert bool(((idx >= 0) & (idx < M))[live].all()), "%s: neighbour index out of range" % name
    lower = torch.arange(M)
    isdup = torch.zeros(M, dtype=torch.bool)
    for a, b in pairs:
        lower[b] = a
        isdup[a] = isdup[b] = True
    hit = live & isdup[own.clamp(min=0)]
    want = lower[own.clamp(min=0)]
    assert bool((idx[hit] == want[hit]).all()), "%s: %d duplicated target(s) answered with another index than the lower one" % (
        name, int((idx[hit] != want[hit]).sum()))
    got = dist_to(ref["pts"].cpu().to(F64), torch.where(live, idx, own), targets.cpu())
    d2 = ref["d2"].cpu().to(F64)
    scale = float(d2.max()) if d2.numel() and float(d2.max()) > 0 else 1.0
    excess = float(((got - d2) * live).max()) / scale if live.any() else 0.0
    e32 = rel_err(d2_32, d2)
    report[name] = (excess, e32)
    print("%-22s excess %.3e  fp32 restatement %.3e  ratio %6.3f  (%d on duplicated rows)" % (name, excess, e32, excess / max(e32, EPS32),
                                                                                      int(hit.sum())))
    return int(hit.sum())


def bandwidth64(kth, dtype=F64):
    """mean_i sqrt(max(kth[b][i], 1e-6))"""
    return torch.sqrt(kth.to(dtype).clamp(min=1e-6)).mean(1)


def verdict(count, used, cap, max_clusters, slots):
    """Python statement of the cluster-count check -> (nuniq list, bad)."""
    nuniq = [int(c) if int(c) > cap else int((u != 0).sum()) for c, u in zip(count.tolist(), used)]
    bad = int(any(u > max_clusters or int(c) > slots for u, c in zip(nuniq, count.tolist())))
    return nuniq, bad


def chamfer_chain(kind, r, V, c, valid, targets, cap, dtype=F64, arg=None, idx=None, device="cpu"):
    """The whole analytic chamfer distance -> (loss, pd, ps, (g_r, g_V, g_c)); the SDF slot / the neighbour of the points
    where the caller passes `arg` / `idx` are fixed to those."""
    r, V, c, valid, targets = (x.to(device) for x in (r, V, c, valid, targets))
    KM, M = valid.shape[1], targets.shape[1]
    leaves = [clean(x).to(dtype).requires_grad_(True) for x in (r, V, c)]
    mat = sdf64(kind, targets, *leaves, dtype=dtype)
    red = sdf_reduce(mat, valid)
    use = red["arg"] if arg is None else torch.where(red["clear"], red["arg"], arg.to(device).long())
    fv = torch.where(use >= 0, torch.gather(mat, 2, use.clamp(min=0).unsqueeze(-1)).squeeze(-1), torch.zeros_like(red["fval"]))
    n, off, _ = budget64(kind, r, valid, cap, dtype)
    pts, _ = samples64(kind, *leaves, n, off, dtype)
    total = off[:, KM].to(device)
    own, _, _ = nearest64(pts, total, targets, dtype)
    nbr = own if idx is None else torch.where(own >= 0, idx.to(device).long()[:, :own.shape[1]], own)
    loss, pd, ps = combine64(dist_to(pts, nbr, targets).sum(1), total, (fv * fv).sum(1), valid, M, dtype)
    grads = torch.autograd.grad(loss, leaves, allow_unused=True) if loss.requires_grad else [None] * 3
    grads = tuple(torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves))
    return loss.detach(), pd.detach(), ps.detach(), grads, dict(arg=red["arg"], clear=red["clear"], idx=own, pts=pts.detach(), total=total)

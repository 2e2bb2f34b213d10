"""Restatements of the DGCNN graph kernels (csrc/dgcnn.hip, csrc/edge_conv.hip, csrc/pool_alg.hip) in plain torch, float64 by
default and float32 through `dtype`, the case tables of tests/test_gpu_dgcnn_graph_guards.py and the input builders.  Written
from the definitions in include/prifit_hip.h -- the edge block on the EXPLICIT [B, N, k, C] tensor, torch reductions, autograd
of sum(dy y) for the backward, bincount / cumsum for the CSR, a stable argsort for the neighbour search -- not from the kernels'
loops.  No GPU import: tests/test_dgcnn_graph_restatement.py pins all of it on the CPU.

Bars: bn_common's (a kernel's error against float64 at most MARGIN x the float32 restatement's error on the same inputs, floored
at 2^-24).

Inputs keep every discrete decision independent of the precision:
- U, Vc (or Vb) lie on the grid of multiples of 2^-20 in [-2, 2): the centre term, every y = U_j - centre_i and hence every
  maximum, minimum and winner are EXACT in float32 (|y| < 8 with a 2^-20 unit is 23 bits), while sums of y do round;
- a table entry shift[b, c] is redrawn until every activation argument scale y* + shift of its sample keeps
  bn_common.DECISION_MARGIN from 0;
- kNN clouds lie on the lattice of multiples of 2^-6 in [-2, 2): products, squared norms and distances are exact in float32
  whatever the fma order, so the float64 stable sort IS the expected answer, ties included."""
import torch

from bn_common import DECISION_MARGIN, act, gen_of, gn_bwd_finalize, gn_finalize, seed_of, signed
from fit_common import F32, F64

EC_PTS = 16             # points per statistics slab (prifit_edge_points_per_slab)
GRID = 2.0 ** -20
LATTICE = 2.0 ** -6
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


# ---------------------------------------------------------------------------------------------------------------------------
# the edge block on the explicit tensor
# ---------------------------------------------------------------------------------------------------------------------------
def edge_y(U, V2, idx, selfterm):
    """-> y [B, N, k, C], ok [B, N, k], centre [B, N, C].  y[b,i,j] = ok ? U[b, idx[b,i,j]] - centre[b,i] : 0 with centre = V2
    (Vc) or U_i - V2_i (V2 = Vb, selfterm).  Differentiable in U and V2; an out-of-range entry is a constant zero row."""
    B, N, C = U.shape
    k = idx.shape[2]
    ok = (idx >= 0) & (idx < N)
    centre = U - V2 if selfterm else V2
    rows = torch.gather(U, 1, torch.where(ok, idx, 0).long().view(B, N * k, 1).expand(-1, -1, C)).view(B, N, k, C)
    y = torch.where(ok.unsqueeze(-1), rows - centre.unsqueeze(2), torch.zeros((), dtype=U.dtype))
    return y, ok, centre


def first_pos(y, best):
    k = y.shape[2]
    ks = torch.arange(k).view(1, 1, k, 1)
    return torch.where(y == best.unsqueeze(2), ks, k).min(2).values


def edge_stats(U, V2, idx, selfterm, dtype=F64):
    """The tables of prifit_edge_stats: ymax, ymin, kx, kn (first positions), nv (valid neighbours), karg (packed), ysum, vct
    [B, N, C]; slab [B N / 16][2][C]; and y itself."""
    y, ok, centre = edge_y(U.to(dtype), V2.to(dtype), idx, selfterm)
    B, N, k, C = y.shape
    ymax, ymin = y.max(2).values, y.min(2).values
    kx, kn = first_pos(y, ymax), first_pos(y, ymin)
    nv = ok.sum(2, keepdim=True).expand(B, N, C)
    ys = y.reshape(B * N // EC_PTS, EC_PTS * k, C)
    return dict(y=y, ok=ok, ymax=ymax, ymin=ymin, kx=kx, kn=kn, nv=nv, karg=(kx | (kn << 10) | (nv << 20)).to(torch.int32),
                ysum=y.sum(2), vct=centre, slab=torch.stack([ys.sum(1), (ys * ys).sum(1)], 1))


def edge_pool(ymax, ymin, scale, shift, slope, dtype=F64):
    """-> out, ystar [B, N, C], z (the activation argument): y* = ymin where scale < 0, else ymax; tables [B, C]"""
    s, t = scale.to(dtype).unsqueeze(1), shift.to(dtype).unsqueeze(1)
    ystar = torch.where(s < 0, ymin.to(dtype), ymax.to(dtype))
    z = ystar * s + t
    return act(z, slope), ystar, z


def winners(kx, kn, scale):
    """[B, N, C]: the position of y* in the neighbour list"""
    return torch.where(scale.unsqueeze(1) < 0, kn, kx)


def edge_T(gp, ystar, scale, shift, slope, dtype=F64):
    """T [B, N, C] = act'(scale y* + shift) gp"""
    g = gp.to(dtype)
    z = ystar.to(dtype) * scale.to(dtype).unsqueeze(1) + shift.to(dtype).unsqueeze(1)
    return torch.where(z > 0, g, g * slope)


def edge_dy(y, win, T, ca, cb, cd):
    """dy [B, N, k, C] = a T [j == winner] + b y + d"""
    k = y.shape[2]
    hot = torch.arange(k).view(1, 1, k, 1) == win.unsqueeze(2)
    a, b, d = (t.to(y.dtype).view(t.shape[0], 1, 1, -1) for t in (ca, cb, cd))
    return a * T.unsqueeze(2) * hot + b * y + d


def edge_bwd(U, V2, idx, selfterm, win, T, ca, cb, cd, dtype=F64):
    """Autograd of sum(dy.detach() * y).  selfterm 0: (dU, dVc); selfterm 1: (dU, dVb), the halves of the gradient with respect
    to the stacked [U | Vb]."""
    C = U.shape[2]
    if selfterm:
        F = torch.cat([U, V2], 2).detach().to(dtype).requires_grad_(True)
        u, v = F[:, :, :C], F[:, :, C:]
    else:
        u, v = U.detach().to(dtype).requires_grad_(True), V2.detach().to(dtype).requires_grad_(True)
    y, _, _ = edge_y(u, v, idx, selfterm)
    dy = edge_dy(y.detach(), win, T.to(dtype), ca, cb, cd)
    (dy.detach() * y).sum().backward()
    if selfterm:
        return F.grad[:, :, :C], F.grad[:, :, C:]
    return u.grad, v.grad


def edge_bwd_absum(U, V2, idx, selfterm, win, T, ca, cb, cd):
    """float64 sums of the |terms|: of dVc its k + 2 terms (a T, b y_j, valid d), of dU the same terms over its in-edges (plus
    the point's own dVc terms with selfterm)"""
    y, ok, _ = edge_y(U.to(F64), V2.to(F64), idx, selfterm)
    B, N, k, C = y.shape
    hot = torch.arange(k).view(1, 1, k, 1) == win.unsqueeze(2)
    a, b, d = (t.to(F64).abs().view(B, 1, 1, C) for t in (ca, cb, cd))
    terms = (a * T.to(F64).abs().unsqueeze(2) * hot + b * y.abs() + d) * ok.unsqueeze(-1)
    av = terms.sum(2)
    au = torch.zeros(B, N, C, dtype=F64)
    for bb in range(B):
        m = ok[bb].reshape(-1)
        au[bb].index_add_(0, idx[bb].reshape(-1)[m].long(), terms[bb].reshape(N * k, C)[m])
    return (au + av if selfterm else au), av


def in_degrees(idx, N):
    """[B, N] valid in-edges of every point"""
    return torch.stack([csr_offsets(i.reshape(-1), N).diff() for i in idx])


# ---------------------------------------------------------------------------------------------------------------------------
# CSR, neighbour search, edge features, the winners' terms of the global pool, slab sums
# ---------------------------------------------------------------------------------------------------------------------------
def csr_offsets(idx, nbins):
    """idx [E] -> offs [nbins + 1]: the exclusive cumsum of the bincount of the entries in [0, nbins)"""
    v = idx[(idx >= 0) & (idx < nbins)].long()
    cnt = torch.bincount(v, minlength=nbins)
    return torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)])


def knn_values(G, xx, dtype=F64):
    """v[b,i,j] = (-xx_i - (-2 G_ij)) - xx_j"""
    G, xx = G.to(dtype), xx.to(dtype)
    return (-xx.unsqueeze(2) - (-2.0 * G)) - xx.unsqueeze(1)


def knn_ref(G, xx, k, dtype=F64):
    """idx [B, N, k]: stable descending argsort of the values (ties to the lower index)"""
    return torch.sort(knn_values(G, xx, dtype), dim=2, descending=True, stable=True).indices[:, :, :k].to(torch.int32)


def gram(x, dtype=F64):
    """x [B, N, 3] -> G = x x^T, xx = |x|^2 (the squares added in the order of the network's own expression)"""
    x = x.to(dtype)
    xx = (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2]
    return x @ x.transpose(1, 2), xx


def edge_feature(x, idx, ld, dtype=F64):
    """[B, N, k, ld]: [x_j - x_i | x_i | 0]"""
    B, N, C = x.shape
    k = idx.shape[2]
    rows = torch.gather(x, 1, idx.long().view(B, N * k, 1).expand(-1, -1, C)).view(B, N, k, C)
    ctr = x.unsqueeze(2).expand(B, N, k, C)
    return torch.cat([rows - ctr, ctr, torch.zeros(B, N, k, ld - 2 * C, dtype=x.dtype)], -1)


def edge_scatter(gout, idx, dx0, C, dtype=F64):
    """dx0 + the gradient of sum(gout[..., :2C] feature) with respect to x; gout [B, N, k, >= 2C]"""
    x = torch.zeros(dx0.shape, dtype=dtype, requires_grad=True)
    f = edge_feature(x, idx, 2 * C)
    (f * gout[..., :2 * C].to(dtype)).sum().backward()
    return dx0.to(dtype) + x.grad


def edge_scatter_absum(gout, idx, dx0, C):
    B, N, k = idx.shape
    g = gout[..., :2 * C].to(F64).abs()
    a = dx0.to(F64).abs() + (g[..., :C] + g[..., C:]).sum(2)
    for b in range(B):
        a[b].index_add_(0, idx[b].reshape(-1).long(), g[b, :, :, :C].reshape(N * k, C))
    return a


def winners_S(arg, T, K, dtype=F64):
    """S [Bs, K, Cout]: T at (winning row, channel), zero elsewhere; where T == 0 the entry of arg is not used"""
    Bs, Cout = T.shape
    live = T != 0
    S = torch.zeros(Bs, K, Cout, dtype=dtype)
    b, c = live.nonzero(as_tuple=True)
    S[b, arg[b, c].long(), c] = T.to(dtype)[b, c]
    return S


def winners_terms(arg, T, W, X, K, dtype=F64):
    """(S W [Bs K, Cin], S^T X [Cout, Cin]) -- what prifit_global_pool_winners_f32 adds to dX and dW"""
    S = winners_S(arg, T, K, dtype)
    Bs, _, Cout = S.shape
    return (S @ W.to(dtype)).view(Bs * K, -1), torch.einsum("bkc,bki->ci", S, X.to(dtype).view(Bs, K, -1))


def slab_sum(part, dtype=F64):
    return part.to(dtype).sum(0)


# ---------------------------------------------------------------------------------------------------------------------------
# input builders
# ---------------------------------------------------------------------------------------------------------------------------
def on_grid(shape, gen, unit=GRID, span=2.0):
    """float32 multiples of `unit` in [-span, span)"""
    n = int(round(span / unit))
    return (torch.randint(-n, n, shape, generator=gen).to(F64) * unit).to(F32)


DEGREES = (0, 1, 11, 12, 13, 63, 64, 65, 76, 77, 130)      # around the 64-entry chunk and the 12-wide batches of the gather pass


def graph_with_degrees(N, k, gen, degrees=DEGREES):
    """idx [N, k] in which point p < len(degrees) has exactly degrees[p] in-edges; the other points share the rest"""
    assert N > len(degrees) and N * k >= sum(degrees)
    flat = torch.cat([torch.full((d,), p, dtype=torch.long) for p, d in enumerate(degrees)]
                     + [torch.randint(len(degrees), N, (N * k - sum(degrees),), generator=gen)])
    return flat[torch.randperm(N * k, generator=gen)].view(N, k).to(torch.int32)


def edge_graph(B, N, k, gen, degrees=False):
    """idx [B, N, k] int32.  Sample 0: prescribed in-degrees (where N k allows) or random, with a repeated neighbour in every
    list; sample 1 (B > 1): entries -1 and N, point 1 without a valid neighbour, point 2 with an out-of-range entry first;
    sample 2: a hub, every edge into point 3 mod N."""
    idx = torch.randint(0, N, (B, N, k), generator=gen, dtype=torch.int32)
    if degrees and N > len(DEGREES) and N * k >= sum(DEGREES):
        idx[0] = graph_with_degrees(N, k, gen)
    elif k >= 2:
        idx[0, :, k - 1] = idx[0, :, (k - 1) // 2]
    if B > 1:
        flat = idx[1].view(-1)
        pick = torch.randperm(flat.numel(), generator=gen)[:max(2, flat.numel() // 6)]
        flat[pick[0::2]] = N
        flat[pick[1::2]] = -1
        if N > 2:
            idx[1, 1] = torch.where(torch.arange(k) % 2 == 0, -1, N).to(torch.int32)
            idx[1, 2, 0] = -1
    if B > 2:
        idx[2] = 3 % N
    return idx


def settle_shift(scale, shift, ystar_of, gen):
    """shift [B, C] redrawn wherever an activation argument scale y* + shift of the sample comes closer to 0 than the margin;
    ystar_of(scale) -> y* [B, N, C]"""
    shift = shift.clone()
    s = scale.to(F64).unsqueeze(1)
    sy = ystar_of(scale).to(F64) * s
    for _ in range(200):
        t = shift.to(F64).unsqueeze(1)
        bad = ((sy + t).abs() < DECISION_MARGIN * (sy.abs() + t.abs())).any(1)
        if not bool(bad.any()):
            return shift
        shift = torch.where(bad, signed(shift.numel(), 0.1, 1.0, gen).view_as(shift), shift)
    raise AssertionError("settle_shift did not converge")


def scale_table(B, C, gen):
    """[B, C] with both signs and, in channels 1 / 2 / 3, the entries 0.0 / -0.0 / a negative one"""
    s = signed(B * C, 0.5, 1.5, gen).view(B, C)
    s[:, 1], s[:, 2], s[:, 3] = 0.0, -0.0, -s[:, 3].abs()
    return s


def edge_case(C, k, N, selfterm, B=3, degrees=False):
    """Inputs of prifit_edge_stats / _bwd.  Sample 1, points 2 .. 4, channels 8 .. 15: the centre is moved so that every valid y
    is negative, the scale is positive there, and point 2 holds an out-of-range entry: the zero row wins."""
    gen = gen_of(seed_of(21, C, k, N, selfterm, B))
    idx = edge_graph(B, N, k, gen, degrees)
    U, V2 = on_grid((B, N, C), gen), on_grid((B, N, C), gen)
    scale = scale_table(B, C, gen)
    if B > 1 and N > 4:
        V2[1, 2:5, 8:16] = (U[1, 2:5, 8:16].to(F64) - 3.0).to(F32) if selfterm else 3.0
        scale[1, 8:16] = scale[1, 8:16].abs()
    st = edge_stats(U, V2, idx, selfterm)
    shift = settle_shift(scale, signed(B * C, 0.1, 1.0, gen).view(B, C), lambda s: edge_pool(st["ymax"], st["ymin"], s, s, 0.0)[1], gen)
    return dict(kind="edge", C=C, k=k, N=N, B=B, selfterm=selfterm, idx=idx, U=U, V2=V2, scale=scale, shift=shift,
                ca=signed(B * C, 0.5, 1.5, gen).view(B, C), cb=(0.1 * torch.randn(B, C, generator=gen)).to(F32),
                cd=(0.1 * torch.randn(B, C, generator=gen)).to(F32), gp=torch.randn(B, N, C, generator=gen).to(F32),
                slope=0.2 if (k + N // 16) % 2 else 0.0)


def pool_case(C, N, slope, B=3):
    """Inputs of prifit_edge_pool alone: ymin <= ymax [B, N, C], tables [B, C]"""
    gen = gen_of(seed_of(22, C, N, slope, B))
    a, b = torch.randn(B, N, C, generator=gen).to(F32), torch.randn(B, N, C, generator=gen).to(F32)
    ymax, ymin = torch.maximum(a, b), torch.minimum(a, b)
    scale = scale_table(B, C, gen)
    shift = settle_shift(scale, signed(B * C, 0.1, 1.0, gen).view(B, C), lambda s: edge_pool(ymax, ymin, s, s, 0.0)[1], gen)
    return dict(kind="pool", C=C, N=N, B=B, slope=slope, ymax=ymax, ymin=ymin, scale=scale, shift=shift)


def knn_cloud(kind, B, N, gen):
    """[B, N, 3] float32 on the lattice.  same: N copies of one point; doubled: every point twice and one point ten times"""
    x = on_grid((B, N, 3), gen, LATTICE)
    if kind == "same":
        x = x[:, :1].expand(B, N, 3).contiguous()
    elif kind == "doubled":
        h = (N + 1) // 2
        x = torch.cat([x[:, :h], x[:, :h]], 1)[:, torch.randperm(2 * h, generator=gen)[:N]].contiguous()
        x[:, torch.randperm(N, generator=gen)[:10]] = x[:, :1].clone()
    else:
        assert kind == "lattice"
    return x


def chain_case(C, N=128, k=9, B=3, groups=2, slope=0.2):
    """One whole block (stats -> GroupNorm -> pool, and back) on the stacked form: beta is redrawn until the activation
    arguments under the block's OWN float64 tables keep the margin (beta moves the shift alone)."""
    gen = gen_of(seed_of(23, C, N, k, B))
    idx = edge_graph(B, N, k, gen)
    U, V2 = on_grid((B, N, C), gen), on_grid((B, N, C), gen, span=1.0)
    gamma, beta = signed(C, 0.5, 1.5, gen), signed(C, 0.1, 1.0, gen)
    case = dict(kind="chain", C=C, N=N, k=k, B=B, groups=groups, slope=slope, selfterm=1, idx=idx, U=U, V2=V2, gamma=gamma,
                gout=torch.randn(B, N, C, generator=gen).to(F32))
    for _ in range(200):
        case["beta"] = beta
        f = chain_forward(case)
        sy, t = f["ystar"] * f["fin"]["scale"].unsqueeze(1), f["fin"]["shift"].unsqueeze(1)
        bad = ((sy + t).abs() < DECISION_MARGIN * (sy.abs() + t.abs())).any(1).any(0)
        if not bool(bad.any()):
            return case
        beta = torch.where(bad, signed(C, 0.1, 1.0, gen), beta)
    raise AssertionError("chain_case did not converge")


GN_EPS = 1e-5


def chain_forward(case, dtype=F64):
    st = edge_stats(case["U"], case["V2"], case["idx"], case["selfterm"], dtype)
    B, N, k, C = st["y"].shape
    sl = st["slab"].view(B, N // EC_PTS, 2, C).sum(1)
    fin = gn_finalize(sl[:, 0], sl[:, 1], case["groups"], float(N * k * (C // case["groups"])), case["gamma"], case["beta"],
                      GN_EPS, dtype=dtype)
    out, ystar, z = edge_pool(st["ymax"], st["ymin"], fin["scale"], fin["shift"], case["slope"], dtype)
    return dict(st=st, fin=fin, out=out, ystar=ystar, z=z, win=winners(st["kx"], st["kn"], fin["scale"]))


def chain_backward(case, f, dtype=F64):
    """-> dU, dVb (or dVc), dgamma, dbeta, and the coefficient tables"""
    fin, st = f["fin"], f["st"]
    B, N, k, C = st["y"].shape
    T = edge_T(case["gout"], f["ystar"], fin["scale"], fin["shift"], case["slope"], dtype)
    yhat = (f["ystar"] - fin["mean"].unsqueeze(1)) * fin["invstd"].unsqueeze(1)
    co = gn_bwd_finalize(T.sum(1), (T * yhat).sum(1), case["groups"], float(N * k * (C // case["groups"])), case["gamma"],
                         fin["mean"], fin["invstd"], dtype=dtype)
    dU, dV = edge_bwd(case["U"], case["V2"], case["idx"], case["selfterm"], f["win"], T, fin["scale"], co["cb"], co["cd"], dtype)
    return dict(dU=dU, dV=dV, dgamma=co["S"][:, 1].sum(0), dbeta=co["S"][:, 0].sum(0), cb=co["cb"], cd=co["cd"], T=T)


# ---------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------
# prifit_knn_topk / prifit_knn3_topk: (N, k); B = 1 and 3, B = 1 alone for N > 2048
KNN_TOPK_CASES = [(1, 1), (63, 63), (65, 3), (64, 64), (130, 65), (130, 130), (1025, 20), (2049, 20), (4096, 64), (4096, 65)]
KNN3_CASES = [(64, 1), (64, 64), (65, 7), (1024, 64), (1025, 20), (2047, 40), (2048, 64)]


def knn_Bs(N):
    return (1,) if N > 2048 else (1, 3)


KNN_KINDS = ("lattice", "same", "doubled")
EDGE_BS = (1, 3)        # every case of the edge tables runs at both (B = 1: the graph of sample 0 alone)


# prifit_edge_gather: (C, k, ld); N = 37 points, B = 3
GATHER_VECTOR_CASES = [(4, 3, 8), (4, 3, 24), (64, 20, 128), (64, 2, 132), (128, 5, 1024)]
GATHER_SCALAR_CASES = [(3, 20, 8), (6, 7, 12), (5, 1, 11), (128, 2, 1028)]
GATHER_N = 37
# prifit_edge_scatter: (C, k, pad of ld_gout, hub)
SCATTER_CASES = [(C, k, pad, hub) for C in (3, 64) for i, k in enumerate((1, 3, 4, 20)) for pad, hub in (((i % 2) * 4, False), (4 - (i % 2) * 4, True))]
# prifit_list_csr / prifit_edge_csr: (nbins, E)
CSR_CASES = [(1, 1), (16, 160), (1023, 1023 * 3), (1024, 1024 * 3), (1025, 1025 * 3), (8192, 8192 * 2), (256, 8193), (7, 1000)]
CSR_GRAPHS = ("random", "hub", "outside")
# prifit_edge_stats: (C, k, N, selfterm, pad of the row strides)
_NS = (16, 48, 128)
STATS_CASES = ([(64, k, _NS[(i + r) % 3], (i + r) % 2, 4 * ((i // 2 + r) % 2)) for r in (0, 1)
                for i, k in enumerate((1, 7, 10, 20, 64, 65, 70, 130))]
               + [(C, k, _NS[(i + r) % 3], (i + r) % 2, 4 * ((i + 1) % 2 if r else i % 2)) for C in (128, 256) for r in (0, 1)
                  for i, k in enumerate((7, 20, 70))])
# prifit_edge_pool: (C, N, pad of ldo: 0, 4 or C, slope)
POOL_CASES = [(C, N, (0, 4, C)[(i + j) % 3], 0.2 if (i + j) % 2 else 0.0) for i, C in enumerate((4, 64, 256)) for j, N in enumerate((1, 5, 128))]
POOL_CASES += [(C, 5, pad, 0.0 if pad == 4 else 0.2) for C in (4, 64, 256) for pad in (0, 4, C)]
POOL_CASES = sorted(set(POOL_CASES))
# prifit_edge_bwd: (C, k, N, selfterm, pad of ldd, pad of ldgp)
BWD_CASES = [(C, k, N, (i + j + r) % 2, 4 * ((i + r) % 2), 4 * ((j + r) % 2)) for C in (64, 128, 256) for r in (0, 1)
             for i, k in enumerate((7, 20, 70)) for j, N in enumerate((16, 48)) if r == 0 or C == 64 or k == 20]
# prifit_global_pool_winners_f32: (Bs, K, Cout, Cin)
WINNERS_CASES = [(1, 1, 64, 64), (3, 63, 64, 128), (3, 65, 128, 256), (2, 130, 1024, 64)]
SLAB_SUM_NSLAB = (1, 7, 8, 9, 31, 32, 33, 57, 1000)
SLAB_SUM_N = (1, 31, 32, 33, 384)
CHAIN_C = (64, 128, 256)


def winners_case(Bs, K, Cout, Cin, one_row=False):
    """arg, T [Bs, Cout], W [Cout, Cin], X [Bs K, Cin], the outputs' starting values.  A fifth of T is 0 and its arg out of
    range (K + 5, -1).  one_row: every channel of sample 0 won by one row."""
    gen = gen_of(seed_of(24, Bs, K, Cout, Cin, one_row))
    arg = torch.randint(0, K, (Bs, Cout), generator=gen, dtype=torch.int32)
    T = torch.randn(Bs, Cout, generator=gen).to(F32)
    if one_row:
        arg[0] = K // 2
    dead = torch.rand(Bs, Cout, generator=gen) < 0.2
    if one_row:
        dead[0] = False
    T[dead] = 0.0
    arg[dead] = torch.where(torch.arange(int(dead.sum())) % 2 == 0, K + 5, -1).to(torch.int32)
    return dict(arg=arg, T=T, W=torch.randn(Cout, Cin, generator=gen).to(F32), X=torch.randn(Bs * K, Cin, generator=gen).to(F32),
                dX0=torch.randn(Bs * K, Cin, generator=gen).to(F32), dW0=torch.randn(Cout, Cin, generator=gen).to(F32))


def csr_graph(kind, B, nbins, E, gen):
    """idx [B, E] int32"""
    idx = torch.randint(0, nbins, (B, E), generator=gen, dtype=torch.int64)
    if kind == "hub":
        idx[:] = nbins // 2
    elif kind == "outside":
        pick = torch.randperm(E, generator=gen)[:max(1, E // 3)]
        vals = torch.tensor([-1, nbins, INT32_MAX, INT32_MIN])
        idx[:, pick] = vals[torch.arange(pick.numel()) % 4]
    return idx.to(torch.int32)


def gather_case(C, k, ld, N=GATHER_N, B=3):
    gen = gen_of(seed_of(25, C, k, ld))
    idx = torch.randint(0, N, (B, N, k), generator=gen, dtype=torch.int32)
    return dict(x=torch.randn(B, N, C, generator=gen).to(F32), idx=idx)


def scatter_case(C, k, pad, hub, N=GATHER_N, B=3):
    gen = gen_of(seed_of(26, C, k, pad, hub))
    idx = torch.randint(0, N, (B, N, k), generator=gen, dtype=torch.int32)
    if hub:
        idx[:] = 5
    return dict(idx=idx, gout=torch.randn(B, N, k, 2 * C, generator=gen).to(F32), dx0=torch.randn(B, N, C, generator=gen).to(F32))


# ---------------------------------------------------------------------------------------------------------------------------
# the decisions of a case, in two precisions
# ---------------------------------------------------------------------------------------------------------------------------
def decisions(case, dtype):
    """Every discrete decision the kernels take on a case: winners' positions, valid counts, activation signs"""
    if case["kind"] == "pool":
        _, ystar, z = edge_pool(case["ymax"], case["ymin"], case["scale"], case["shift"], case["slope"], dtype)
        return [z > 0, ystar == case["ymax"].to(dtype)]
    if case["kind"] == "chain":
        f = chain_forward(case, dtype)
        return [f["st"]["karg"], f["win"], f["z"] > 0]
    st = edge_stats(case["U"], case["V2"], case["idx"], case["selfterm"], dtype)
    _, _, z = edge_pool(st["ymax"], st["ymin"], case["scale"], case["shift"], case["slope"], dtype)
    return [st["karg"], z > 0]


def all_cases():
    """(label, builder) of every case of the edge tables"""
    out = []
    for B in EDGE_BS:
        for c in STATS_CASES:
            out.append(("stats%s B=%d" % (c, B), lambda c=c, B=B: edge_case(*c[:4], B=B)))
        for c in BWD_CASES:
            out.append(("bwd%s B=%d" % (c, B), lambda c=c, B=B: edge_case(*c[:4], B=B, degrees=True)))
    for c in POOL_CASES:
        out.append(("pool%s" % (c,), lambda c=c: pool_case(c[0], c[1], c[3])))
    for C in CHAIN_C:
        out.append(("chain(%d)" % C, lambda C=C: chain_case(C)))
    return out

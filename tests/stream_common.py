"""Restatements of the weights-stationary streaming products (csrc/gemm_stream.hip) and of the fused dA + dW kernel
(csrc/gemm_stream_bwd.hip) in plain torch, float64 by default and float32 through `dtype`, with the inputs and the case
tables of tests/test_gpu_stream_gemm_guards.py.  Written from the definitions in include/prifit_hip.h -- whole-tensor algebra
and torch reductions -- not from the kernels' loops; the pieces tests/bn_common.py already states (the masked gradient, the
(m1, m2) terms, bn_relu_bwd_apply's expression) are taken from there.  tests/test_stream_restatement.py pins all of it
against torch autograd of the layers written with torch.nn.functional.

What IS taken from the launchers is which 64-row tile belongs to which per-workgroup slab (tile t -> workgroup t mod grid):
the slabs are an output of the C ABI, and comparing them one by one keeps the float32 yardstick honest (a float32 sum of 64
rows against a kernel's sum of 64 rows, not against a cascade over 32768).

Every product comes with its float64 sum of |terms| (the same expression with every factor replaced by its magnitude): the
element-by-element normaliser of the bars."""
import torch

import bn_common as bc
from bn_common import F32, F64

TILE = 64               # rows of a streamed tile (SBM of both kernels)
STREAM_MIN = 32768      # least M / P of the _f32, _dgrad*, _tn* entry points
WIDTHS = (64, 96, 128)
BWD_PAIRS = ((128, 128), (128, 96), (128, 64), (96, 64), (64, 64))      # (Cout, Cin) of prifit_gemm_stream_bwd_f32
T_SWEEP = (0, 1, 4, 5, 36, 63)      # 4 | 5: the lane row 4 * lh; 36: the wave row wm * 32 (+ 4)
T_RAGGED = 37                       # the one ragged tail of the width sweeps: rows 32, 36 exist, 37 .. 63 do not
# one (N, K) per WN / TM configuration of gemm_stream_kernel (N == 64: WN = 2, TM = 1; else WN = 4, TM = 2) for the t sweep
SWEEP_PAIRS = ((64, 128), (96, 64))


# ---------------------------------------------------------------------------------------------------------------------------
# slabs
# ---------------------------------------------------------------------------------------------------------------------------
def stream_grid(M, K):
    """prifit_gemm_stream_slabs: the slabs the caller reads"""
    tiles = -(-M // TILE)
    return min(tiles, 256 * (4 if K <= 64 else 3 if K <= 96 else 2))


def launched_grid(M, K, heavy):
    """The workgroups gemm_stream_kernel runs on (the resident ones of the variant; `heavy`: the dA forms and the pool-candidate
    forward); the slabs from there to stream_grid(M, K) are written as zeros."""
    occ = (3 if heavy else 4) if K <= 64 else (2 if heavy else 3) if K <= 96 else 2
    return min(stream_grid(M, K), 256 * occ)


def wg_slabs(T0, T1, grid, nslab, dtype=F64):
    """[nslab][2][C]: the column sums of the two term matrices over the rows of each workgroup's tiles (tile t belongs to
    workgroup t mod grid; slabs grid .. nslab - 1 are zero)"""
    out = []
    for T in (T0, T1):
        T = T.to(dtype)
        P, C = T.shape
        tiles = -(-P // TILE)
        pad = torch.zeros(tiles * TILE, C, dtype=dtype)
        pad[:P] = T
        per_tile = pad.view(tiles, TILE, C).sum(1)
        out.append(torch.zeros(nslab, C, dtype=dtype).index_add_(0, torch.arange(tiles) % grid, per_tile))
    return torch.stack(out, 1)


def stats_terms(C):
    """(y, y^2) of the stored product: col_stats"""
    return C, C * C


def red_terms(G, Yprev, scale, shift, mean, invstd, dtype=F64):
    """(Gm, Gm yhat) of the layer below: Gm = (Yprev scale + shift > 0 ? G : 0), yhat = (Yprev - mean) invstd"""
    Gm = bc.masked_grad(G, Yprev, scale, shift, 0, 0.0, dtype)
    return bc.bwd_terms(Gm, Yprev, mean, invstd, 0, dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------
def prologue(A, scale=None, shift=None, dtype=F64):
    """relu(a scale + shift), or a itself"""
    a = A.to(dtype)
    return a if scale is None else torch.relu(a * scale.to(dtype) + shift.to(dtype))


def gather_rows(U, Vc, idx, n_points, n_centres, rows_per_centre, dtype=F64):
    """y1 [M, C]: row r = U[b, idx[r]] - Vc[b, s] with b = r // (n_centres rows_per_centre), s = (r // rows_per_centre) %
    n_centres; an index outside [0, n_points) reads point 0."""
    M = idx.numel()
    C = U.shape[-1]
    B = M // (n_centres * rows_per_centre)
    i = idx.view(-1).long()
    i = torch.where((i >= 0) & (i < n_points), i, torch.zeros_like(i))
    r = torch.arange(M)
    b = r // (n_centres * rows_per_centre)
    s = (r // rows_per_centre) % n_centres
    return U.to(dtype).view(B, n_points, C)[b, i] - Vc.to(dtype).view(B, n_centres, C)[b, s]


def one_hot_T(arg, T, pool_K, dtype=F64):
    """[G pool_K, C]: T[g, c] at row arg[g, c] of group g, 0 elsewhere"""
    G, C = arg.shape
    z = torch.zeros(G, pool_K, C, dtype=dtype)
    return z.scatter(1, arg.long().unsqueeze(1), T.to(dtype).unsqueeze(1)).view(G * pool_K, C)


def dy_middle(G, Y, s, t, a, b, d, dtype=F64):
    """dY = a (Y s + t > 0 ? G : 0) + (b Y + d), and the sum of the magnitudes of its three terms"""
    Gm = bc.masked_grad(G, Y, s, t, 0, 0.0, dtype)
    dY = bc.apply_bwd(Gm, Y, a, b, d, 0, dtype)
    mag = (a.to(dtype) * Gm).abs() + (b.to(dtype) * Y.to(dtype)).abs() + d.to(dtype).abs()
    return dY, mag


def dy_pooled(Y, arg, T, b, d, pool_K, dtype=F64, with_d=True):
    """dY = b Y + d + (k == arg ? T : 0) (with_d = False: without d, which prifit_gemm_stream_dgrad_pool_f32 takes folded into
    bias_dW), and the sum of the magnitudes of its terms"""
    y, oh = Y.to(dtype), one_hot_T(arg, T, pool_K, dtype)
    dd = d.to(dtype) if with_d else torch.zeros((), dtype=dtype)
    return b.to(dtype) * y + dd + oh, (b.to(dtype) * y).abs() + dd.abs() + oh.abs()


# ---------------------------------------------------------------------------------------------------------------------------
# entry points
# ---------------------------------------------------------------------------------------------------------------------------
def gemm_fwd(A, B, layout, a_scale=None, a_shift=None, bias=None, dtype=F64):
    """prifit_gemm_stream_f32 / _pool_f32 / _gather_f32 (A = the gathered rows): C = op(A) B^T (layout 0, B [N, K]) or op(A) B
    (layout 1, B [K, N]) + bias -> (C, sum of |terms|)"""
    a, b = prologue(A, a_scale, a_shift, dtype), B.to(dtype)
    b = b.t() if layout == 0 else b
    C, ab = a @ b, a.abs() @ b.abs()
    if bias is not None:
        C, ab = C + bias.to(dtype), ab + bias.to(dtype).abs()
    return C, ab


def cand_of(C):
    """cand [M / 32][4][N] of the STORED product (exact): max, row of its first occurrence, min, row of its first occurrence
    per 32-row block; the rows as integers"""
    M, N = C.shape
    v = C.view(M // 32, 32, N)
    ks = torch.arange(32).view(1, 32, 1)
    vmax, vmin = v.max(1).values, v.min(1).values
    amax = torch.where(v == vmax.unsqueeze(1), ks, 32).min(1).values
    amin = torch.where(v == vmin.unsqueeze(1), ks, 32).min(1).values
    return vmax, amax, vmin, amin


def dgrad(dY, mag, W, bias=None, dtype=F64):
    """G = dY W (+ bias) for W [K, N] -> (G, sum of |terms|); dY and the magnitudes of its terms from dy_middle / dy_pooled, or
    a given dY with mag = |dY|"""
    w = W.to(dtype)
    G, ab = dY.to(dtype) @ w, mag.to(dtype) @ w.abs()
    if bias is not None:
        G, ab = G + bias.to(dtype), ab + bias.to(dtype).abs()
    return G, ab


def wgrad(dY, mag, A, b_scale=None, b_shift=None, out0=None, dtype=F64):
    """out = out0 + dY^T relu(bn(A)) -> (out [Mo, No], sum of |terms|)"""
    a = prologue(A, b_scale, b_shift, dtype)
    out, ab = dY.to(dtype).t() @ a, mag.to(dtype).t() @ a.abs()
    if out0 is not None:
        out, ab = out + out0.to(dtype), ab + out0.to(dtype).abs()
    return out, ab


def fused_bwd(dY, mag, W, Yp, p_scale, p_shift, dtype=F64):
    """prifit_gemm_stream_bwd_f32 / _bwd_gather_f32 (Yp = the gathered rows): Gp = dY W and dW = dY^T relu(p_scale Yp +
    p_shift), each with its sum of |terms|; W [Cout, Cin]"""
    return dgrad(dY, mag, W, None, dtype), wgrad(dY, mag, Yp, p_scale, p_shift, None, dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs whose decisions do not depend on the precision
# ---------------------------------------------------------------------------------------------------------------------------
DUP0, DUP1 = 20, 110        # rows DUP0 .. DUP1 - 1 repeat row DUP0: three whole 32-row blocks of equal rows, both lane halves


def with_dups(X):
    X = X.clone()
    if X.shape[0] > DUP1:
        X[DUP0:DUP1] = X[DUP0]
    return X


def rows_randn(P, C, gen):
    return torch.randn(P, C, generator=gen).to(F32)


def fwd_case(M, N, K, layout, aff=True, bias=True, seed=0):
    """A [M, K] (a run of duplicated rows; nudged away from the prologue's threshold), B, the prologue tables (both signs, a zero
    scale in channel 1), bias"""
    gen = bc.gen_of(bc.seed_of(21, N, K, layout, seed))
    t = bc.rand_tables(1, K, gen, zero_scale=1)
    A = with_dups(rows_randn(M, K, gen))
    if aff:
        A = bc.nudge_act(A, t["scale"], t["shift"], 0)
    B = (torch.randn((N, K) if layout == 0 else (K, N), generator=gen) / K ** 0.5).to(F32)
    return dict(M=M, N=N, K=K, layout=layout, A=A, B=B, scale=t["scale"][0] if aff else None,
                shift=t["shift"][0] if aff else None, bias=(0.3 * torch.randn(N, generator=gen)).to(F32) if bias else None)


def gather_fwd_case(n_points, n_centres, rpc, Bs, N, seed=0):
    """The by-linearity rows: idx [M] with one index of -1 and one of n_points, never n_points - 1 (the index poison of the GPU
    tests, whose row of U is NaN there).  The rows are differences and cannot be nudged one by one; they need not be: the
    forward's relu is continuous, so a mask that differs between the precisions next to 0 moves the operand by a rounding."""
    K = 64
    M = Bs * n_centres * rpc
    gen = bc.gen_of(bc.seed_of(22, n_points, n_centres, rpc, Bs, N, seed))
    idx = torch.randint(0, n_points - 1, (M,), generator=gen).to(torch.int32)
    idx[DUP0:DUP1] = idx[DUP0]
    idx[DUP1 + 3], idx[M - 2] = -1, n_points
    U, Vc = rows_randn(Bs * n_points, K, gen).view(Bs, n_points, K), rows_randn(Bs * n_centres, K, gen).view(Bs, n_centres, K)
    t = bc.rand_tables(1, K, gen, zero_scale=1)
    return dict(M=M, N=N, K=K, idx=idx, U=U, Vc=Vc, n_points=n_points, n_centres=n_centres, rpc=rpc, Bs=Bs,
                B=(torch.randn(N, K, generator=gen) / 8.0).to(F32), scale=t["scale"][0], shift=t["shift"][0],
                bias=(0.3 * torch.randn(N, generator=gen)).to(F32))


def bwd_case(P, Cout, Cin, pool_K=0, seed=0, gather=None):
    """Inputs of the backward of one layer Y [P, Cout] = relu(bn(Yp)) W^T on top of the layer Yp [P, Cin]: G (the gradient w.r.t.
    relu(bn(Y))), the layer's tables (s, t, a, b, d), W [Cout, Cin], the tables of the layer below (scale, shift, mean, invstd);
    pooled: arg / T [P / pool_K, Cout] with a tie-free winner per (group, channel) by construction (arg is an input).
    gather = (n_points, n_centres, rows_per_centre, Bs): Yp is re-formed from (idx, U, Vc)."""
    gen = bc.gen_of(bc.seed_of(23, Cout, Cin, pool_K, seed))
    t, tp = bc.rand_tables(1, Cout, gen, zero_scale=1), bc.rand_tables(1, Cin, gen, zero_scale=1)
    c = dict(P=P, Cout=Cout, Cin=Cin, pool_K=pool_K, W=(torch.randn(Cout, Cin, generator=gen) / Cout ** 0.5).to(F32))
    c["Y"] = bc.nudge_act(with_dups(rows_randn(P, Cout, gen)), t["scale"], t["shift"], 0)
    c["G"] = with_dups(rows_randn(P, Cout, gen))
    if gather:
        n_points, n_centres, rpc, Bs = gather
        assert P == Bs * n_centres * rpc and Cin == 64
        idx = torch.randint(0, n_points - 1, (P,), generator=gen).to(torch.int32)
        idx[3], idx[P - 2] = -1, n_points
        U, Vc = rows_randn(Bs * n_points, Cin, gen).view(Bs, n_points, Cin), rows_randn(Bs * n_centres, Cin, gen).view(Bs, n_centres, Cin)
        for _ in range(50):
            bad = bc.act_violations(gather_rows(U, Vc, idx, n_points, n_centres, rpc).to(F32), tp["scale"], tp["shift"], 0)
            if not bool(bad.any()):
                break
            tp["shift"] = torch.where(bad.any(0), bc.signed(Cin, 0.1, 1.0, gen), tp["shift"][0]).view(1, Cin)
        else:
            raise AssertionError("bwd_case did not converge")
        c.update(idx=idx, U=U, Vc=Vc, n_points=n_points, n_centres=n_centres, rpc=rpc, Bs=Bs)
        c["Yp"] = gather_rows(U, Vc, idx, n_points, n_centres, rpc).to(F32)      # the stored form of the rows, for the masks
    else:
        c["Yp"] = bc.nudge_act(with_dups(rows_randn(P, Cin, gen)), tp["scale"], tp["shift"], 0)
    if pool_K:
        Gn = P // pool_K
        c["arg"] = torch.randint(0, pool_K, (Gn, Cout), generator=gen).to(torch.int32)
        c["arg"][0, :4] = torch.tensor([0, pool_K - 1, min(TILE, pool_K) - 1, max(pool_K - TILE, 0)])      # the edges of a group and of a tile
        c["T"] = rows_randn(Gn, Cout, gen)
    for k in ("scale", "shift", "a", "b", "d"):
        c[k] = t[k][0]
    for k in ("scale", "shift", "mean", "invstd"):
        c["p_" + k] = tp[k][0]
    return c


def bwd_dy(c, dtype=F64, rows=None, with_d=True):
    """(dY, magnitudes) of a bwd_case, its first `rows` rows"""
    P = c["P"] if rows is None else rows
    if c["pool_K"]:
        return dy_pooled(c["Y"][:P], c["arg"][:P // c["pool_K"]], c["T"][:P // c["pool_K"]], c["b"], c["d"], c["pool_K"], dtype, with_d)
    return dy_middle(c["G"][:P], c["Y"][:P], c["scale"], c["shift"], c["a"], c["b"], c["d"], dtype)


def decision_violations(c):
    """Activation arguments of a case that are closer to 0 than bn_common's margin (prologue, both masks)"""
    n = 0
    if "A" in c and c.get("scale") is not None:
        n += int(bc.act_violations(c["A"], c["scale"].view(1, -1), c["shift"].view(1, -1), 0).sum())
    if "Y" in c:
        n += int(bc.act_violations(c["Y"], c["scale"].view(1, -1), c["shift"].view(1, -1), 0).sum())
        n += int(bc.act_violations(c["Yp"], c["p_scale"].view(1, -1), c["p_shift"].view(1, -1), 0).sum())
    return n

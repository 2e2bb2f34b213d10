"""Restatements of the point-index kernels (csrc/pointops.hip) and of the set-abstraction front end (csrc/sa_group.hip) in plain
torch, float64 by default and float32 through `dtype`, the case tables of tests/test_gpu_sa_front_guards.py and the input
builders.  Written from the definitions in include/prifit_hip.h -- whole-tensor algebra, a cumulative count for the ball lists,
a stable sort for the three nearest, one-hot matrices for the column packers -- not from the kernels' loops.  No GPU import:
tests/test_sa_front_restatement.py pins all of it on the CPU.

Bars: bn_common's (a kernel's error against float64 at most MARGIN x the float32 restatement's error on the same inputs, floored
at 2^-24; element-wise outputs by max |fp64|, reduced outputs element by element by the float64 sum of |terms|).

Inputs keep every discrete decision independent of the precision:
- lattice clouds: coordinates are multiples of 2^-6 in [-1, 1] (a far centre at (9, 9, 9)).  Products are multiples of 2^-12,
  every partial sum of the direct and of the expanded squared distance is a multiple of 2^-12 below 2^10: 22 bits, exact in
  float32 in any order and with or without fma.  The float64 statement of FPS, ball query, 3-NN and square distance IS the
  expected answer, ties and points on a radius included; radii are square roots of lattice distances;
- off-lattice clouds (synth.cloud): integer results and distances are compared with prifit_oracle.c_*, the bit-exact recipe;
- the BatchNorm forms of the weight gradient: U and Vc lie on the grid of multiples of 2^-4 in [-2, 2), so y1 = U_j - Vc is
  exact in float32, and it is one value for BOTH forms (the gather form re-forms it, so an element cannot move on its own):
  the entries of `shift` are redrawn until every activation argument scale y1 + shift keeps bn_common.DECISION_MARGIN from 0,
  then bn_common.nudge_act runs over the result, finds nothing to move, and the builder asserts that no violation remains."""
import numpy as np
import torch

from bn_common import act_violations, gen_of, nudge_act, seed_of, signed
from fit_common import F32, F64

LATTICE = 2.0 ** -6
UNIT2 = 2.0 ** -12                       # unit of the squared lattice distances
NN_EPS = float(np.float32(1e-8))         # the kernel's 1e-8f
FAR = 9.0                                # the centre of an empty ball
Y1_GRID = 2.0 ** -4


# ---------------------------------------------------------------------------------------------------------------------------
# distances and index results
# ---------------------------------------------------------------------------------------------------------------------------
def sqdist_direct(src, dst, dtype=F64):
    """[B, S, N]: (dx^2 + dy^2) + dz^2 of the differences"""
    d = src.to(dtype).unsqueeze(2) - dst.to(dtype).unsqueeze(1)
    q = d * d
    return (q[..., 0] + q[..., 1]) + q[..., 2]


def norm2(x):
    q = x * x
    return (q[..., 0] + q[..., 1]) + q[..., 2]


def sqdist_expanded(src, dst, dtype=F64):
    """[B, S, N]: -2 s.d + |s|^2 + |d|^2 (models/pointnet_util.py:37-39), every product and sum an operation of its own"""
    s, d = src.to(dtype), dst.to(dtype)
    t = s[..., 0].unsqueeze(2) * d[..., 0].unsqueeze(1)
    t = t + s[..., 1].unsqueeze(2) * d[..., 1].unsqueeze(1)
    t = t + s[..., 2].unsqueeze(2) * d[..., 2].unsqueeze(1)
    return (-2.0 * t + norm2(s).unsqueeze(2)) + norm2(d).unsqueeze(1)


def fps(xyz, npoint, start, dtype=F64):
    """[B, npoint] int64: the start index, then always the point farthest from the picked set (direct distances, the running
    minimum starts at 1e10), the LOWEST index among equal distances"""
    x = xyz.to(dtype)
    B, N, _ = x.shape
    near = torch.full((B, N), 1e10, dtype=dtype)
    cur = start.to(torch.int64).clone()
    out = torch.empty(B, npoint, dtype=torch.int64)
    rows = torch.arange(B)
    for i in range(npoint):
        out[:, i] = cur
        near = torch.minimum(near, sqdist_direct(x[rows, cur].unsqueeze(1), x, dtype).squeeze(1))
        far = near.max(1, keepdim=True).values
        cur = torch.where(near == far, torch.arange(N).expand(B, N), N).min(1).values
    return out


def ball_query(xyz, ctr, r2, K, dtype=F64):
    """[B, S, K] int64: the first K indices with not (d > r2) in ascending order (a point ON the radius is inside), the free
    slots filled with the first of them, every slot N for an empty ball.  r2 is the float32 value the kernel receives."""
    d = sqdist_expanded(ctr, xyz, dtype)
    B, S, N = d.shape
    inside = ~(d > torch.tensor(r2, dtype=F32).to(dtype))
    rank = inside.cumsum(-1) - 1
    first = torch.where(inside.any(-1), inside.int().argmax(-1), N)
    out = first.unsqueeze(-1).expand(B, S, K).clone()
    b, s, n = (inside & (rank < K)).nonzero(as_tuple=True)
    out[b, s, rank[b, s, n]] = n
    return out


def three_nn(xyz1, xyz2, dtype=F64):
    """-> d3 [B, N, 3], idx3 [B, N, 3] int64: the three smallest expanded-form distances, the lower index among equal ones"""
    d = sqdist_expanded(xyz1, xyz2, dtype)
    v, i = torch.sort(d, dim=-1, stable=True)
    return v[..., :3], i[..., :3]


def nn_weights(d3, dtype=F64):
    """recip = 1 / (d + 1e-8f); w = recip / ((recip0 + recip1) + recip2)"""
    recip = 1.0 / (d3.to(dtype) + torch.tensor(NN_EPS, dtype=dtype))
    return recip / ((recip[..., 0] + recip[..., 1]) + recip[..., 2]).unsqueeze(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# grouping, the first layer, its statistics and tables
# ---------------------------------------------------------------------------------------------------------------------------
def take_rows(table, idx):
    """table [B, N, C], idx [B, ...] -> ([B, ..., C], ok [B, ...]); an entry < 0 or >= N gives a zero row.  Differentiable."""
    B, N, C = table.shape
    ok = (idx >= 0) & (idx < N)
    flat = torch.where(ok, idx, 0).long().reshape(B, -1, 1).expand(-1, -1, C)
    rows = torch.gather(table, 1, flat).reshape(*idx.shape, C)
    return torch.where(ok.unsqueeze(-1), rows, torch.zeros((), dtype=table.dtype)), ok


def grouped_rows(xyz, ctr, feat, idx, feat_first, dtype=F64):
    """[B, S, K, D + 3]: [feat_j | xyz_j - c_s] (feat_first) or [xyz_j - c_s | feat_j]; zero rows for entries outside [0, N)"""
    x, c = xyz.to(dtype), ctr.to(dtype)
    p, ok = take_rows(x, idx)
    rel = torch.where(ok.unsqueeze(-1), p - c.unsqueeze(2), torch.zeros((), dtype=dtype))
    if feat is None or feat.shape[-1] == 0:
        return rel
    f, _ = take_rows(feat.to(dtype), idx)
    return torch.cat([f, rel] if feat_first else [rel, f], -1)


def first_layer(rows, W, bias, dtype=F64):
    """rows W^T + b"""
    y = rows.to(dtype) @ W.to(dtype).t()
    return y if bias is None else y + bias.to(dtype)


def gather_layer(U, Vc, bias, idx, dtype=F64):
    """[B, S, K, C]: (U_j - Vc_s) + b; the bias alone for an entry outside [0, N)"""
    u, ok = take_rows(U.to(dtype), idx)
    y = torch.where(ok.unsqueeze(-1), u - Vc.to(dtype).unsqueeze(2), torch.zeros((), dtype=dtype))
    return y if bias is None else y + bias.to(dtype)


def slab_stats(Y, q, dtype=F64):
    """Y [B, S, K, C] -> [B ceil(S / q)][2][C]: column sums and sums of squares over the rows of every q queries (the last slab
    of a shape holds the queries that are left: absent queries contribute nothing)"""
    y = Y.to(dtype)
    B, S, K, C = y.shape
    out = []
    for b in range(B):
        for s0 in range(0, S, q):
            t = y[b, s0:s0 + q].reshape(-1, C)
            out.append(torch.stack([t.sum(0), (t * t).sum(0)]))
    return torch.stack(out)


def slab_absum(Y, q):
    return slab_stats(Y.to(F64).abs(), q)


def point_tables(xyz, ctr, feat, W, bias, feat_first, dtype=F64):
    """U [B, N, C] = [feat | xyz] W^T + b, Vc [B, S, C] = c Wx^T (W [C][D + 3] in the column order of grouped_rows)"""
    W = W.to(dtype)
    D = W.shape[1] - 3
    Wx = W[:, D:] if feat_first else W[:, :3]
    Wf = W[:, :D] if feat_first else W[:, 3:]
    U = xyz.to(dtype) @ Wx.t()
    if D:
        U = U + feat.to(dtype) @ Wf.t()
    if bias is not None:
        U = U + bias.to(dtype)
    return U, ctr.to(dtype) @ Wx.t()


def bn_dy(G, Y1, scale, shift, ca, cb, cd, dtype=F64):
    """dY = ca (Y1 scale + shift > 0 ? g : 0) + cb y + cd; tables [C]"""
    g, y = G.to(dtype), Y1.to(dtype)
    z = y * scale.to(dtype) + shift.to(dtype)
    return ca.to(dtype) * torch.where(z > 0, g, torch.zeros((), dtype=dtype)) + cb.to(dtype) * y + cd.to(dtype)


def first_layer_dw(dY, rows, dtype=F64):
    """dW [C, D + 3] = dY^T rows over all P grouped samples"""
    return dY.to(dtype).t() @ rows.to(dtype).reshape(dY.shape[0], -1)


def first_layer_dw_absum(dY, rows):
    return dY.to(F64).abs().t() @ rows.to(F64).abs().reshape(dY.shape[0], -1)


# ---------------------------------------------------------------------------------------------------------------------------
# scatter-adds, interpolation, feature-propagation rows, column packers
# ---------------------------------------------------------------------------------------------------------------------------
def scatter_add(g, idx, d0, dtype=F64):
    """d0 [B, N, C] + the rows g [B, S K, C] added at idx [B, S K]; entries outside [0, N) are dropped"""
    out = d0.to(dtype).clone()
    N = out.shape[1]
    g = g.to(dtype)
    for b in range(out.shape[0]):
        i = idx[b].reshape(-1).long()
        ok = (i >= 0) & (i < N)
        for r in ok.nonzero().squeeze(1).tolist():
            out[b, i[r]] += g[b, r]
    return out


def scatter_add_absum(g, idx, d0):
    return scatter_add(g.to(F64).abs(), idx, d0.to(F64).abs())


def interpolate(p2, idx3, w, dtype=F64):
    """[B, N, C] = (p2[i0] w0 + p2[i1] w1) + p2[i2] w2"""
    rows, _ = take_rows(p2.to(dtype), idx3)
    t = rows * w.to(dtype).unsqueeze(-1)
    return (t[:, :, 0] + t[:, :, 1]) + t[:, :, 2]


def fp_rows(p2, idx3, w, p1, kp, N, dtype=F64):
    """[B, N, kp] = [interpolated | points1 | 0]; idx3 None: S == 1, every point takes p2[b, 0]"""
    B = p2.shape[0]
    left = p2.to(dtype)[:, :1].expand(B, N, -1) if idx3 is None else interpolate(p2, idx3, w, dtype)
    parts = [left] + ([p1.to(dtype)] if p1 is not None and p1.shape[-1] else [])
    used = sum(p.shape[-1] for p in parts)
    return torch.cat(parts + [torch.zeros(B, N, kp - used, dtype=dtype)], -1)


def interpolate_bwd(g, idx3, w, d0, dtype=F64):
    """d0 [B, S, C] + sum over (point, slot) of g[b, n] w[b, n, j] at row idx3[b, n, j]"""
    B, N, C = g.shape
    t = (g.to(dtype).unsqueeze(2) * w.to(dtype).unsqueeze(-1)).reshape(B, N * 3, C)
    return scatter_add(t, idx3.reshape(B, N * 3), d0, dtype)


def interpolate_bwd_absum(g, idx3, w, d0):
    return interpolate_bwd(g.to(F64).abs(), idx3, w.to(F64).abs(), d0.to(F64).abs())


def col_matrix(cmap, scols, dtype=F64):
    """[scols, len(cmap)]: a one in (cmap[j], j); a column of zeros for cmap[j] == -1"""
    M = torch.zeros(scols, len(cmap), dtype=dtype)
    for j, c in enumerate(cmap):
        if c >= 0:
            M[c, j] = 1.0
    return M


def pack_cols(w, cmap, dtype=F64):
    return w.to(dtype) @ col_matrix(cmap, w.shape[1], dtype)


def unpack_cols(g, cmap, scols, dtype=F64):
    return g.to(dtype) @ col_matrix(cmap, scols, dtype).t()


def inverse_map(cmap, scols):
    """(inv_off [scols + 1], inv_idx) int32: for every source column the output columns it feeds, ascending"""
    lists = [[j for j, c in enumerate(cmap) if c == s] for s in range(scols)]
    off = np.cumsum([0] + [len(x) for x in lists])
    flat = [j for x in lists for j in x] or [0]
    return torch.tensor(off, dtype=torch.int32), torch.tensor(flat, dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# input builders
# ---------------------------------------------------------------------------------------------------------------------------
def on_lattice(shape, gen, unit=LATTICE, span=1.0):
    """float32 multiples of `unit` in [-span, span]"""
    n = int(round(span / unit))
    return (torch.randint(-n, n + 1, shape, generator=gen).to(F64) * unit).to(F32)


def lattice_cloud(kind, B, N, gen):
    """[B, N, 3] on the lattice.  lattice: about a fifth of the points are exact copies of earlier ones; same: one point N times"""
    x = on_lattice((B, N, 3), gen)
    if kind == "same":
        return x[:, :1].expand(B, N, 3).contiguous()
    assert kind == "lattice"
    if N >= 5:
        src = torch.randint(0, N, (N // 5,), generator=gen)
        dst = torch.randint(0, N, (N // 5,), generator=gen)
        x[:, dst] = x[:, src].clone()
    return x


# squared radii in units of 2^-12, each a sum of three squares of lattice steps (the offset that attains it beside it)
R2_TINY, R2_SMALL, R2_MID, R2_BIG, R2_ALL = 1, 64, 512, 3072, 12 * 4096
OFFSETS = {R2_TINY: (1, 0, 0), R2_SMALL: (0, 8, 0), R2_MID: (16, 0, 16), R2_BIG: (32, 32, 32)}
# (squared radii, nsample): the largest radius first, in the middle, last; one that takes every point beside one that never
# fills (every candidate passes through the ring)
BALL_RK = [
    ((R2_BIG,), (1,)),
    ((R2_BIG, R2_SMALL), (16, 63)),
    ((R2_SMALL, R2_BIG, R2_MID), (64, 65, 128)),
    ((R2_SMALL, R2_MID, R2_TINY, R2_BIG), (128, 1, 16, 64)),
    ((R2_ALL, R2_TINY), (65, 128)),
]
BALL_N = (1, 63, 64, 65, 2047, 2048)
BALL_N_QUERY_ONLY = (2049, 4097)        # two and three LDS tiles of prifit_ball_query; the front end stops at 2048
BALL_S = (1, 3, 4, 5, 9)
BALL_K_MAX = 1024


def ball_case(N, S, r2u, B, exact_k=0):
    """xyz [B, N, 3], ctr [B, S, 3] on the lattice.  Centres are points of the cloud (d = 0); beside the first centres sits a
    point exactly ON every radius; the last centre of S > 1 is (9, 9, 9): an empty ball.  exact_k: centre 0 of sample 0 is a
    point that the cloud holds exactly exact_k times, every other point at least 2^-6 away."""
    gen = gen_of(seed_of(41, N, S, len(r2u), r2u[0], B, exact_k))
    xyz = lattice_cloud("lattice", B, N, gen)
    ctr = xyz[:, torch.randint(0, N, (S,), generator=gen)].clone()
    slot = 0
    for s in range(min(S, 2)):
        for u in r2u:
            if u in OFFSETS and slot < N:
                off = torch.tensor(OFFSETS[u], dtype=F64) * LATTICE
                c = ctr[:, s].to(F64)
                xyz[:, (7 * slot + 3) % N] = (c - torch.where(c > 0, off, -off)).to(F32)
                slot += 1
    if exact_k:
        assert N >= exact_k
        p0 = torch.tensor([1.0, 0.5, -0.25])
        xyz[0] = torch.where((xyz[0] == p0).all(-1, keepdim=True), xyz[0] - LATTICE, xyz[0])
        xyz[0, torch.randperm(N, generator=gen)[:exact_k]] = p0
        ctr[0, 0] = p0
    if S > 1:
        ctr[:, S - 1] = FAR
    return xyz, ctr


def r2_of(units):
    return [float(u) * UNIT2 for u in units]


def oob_index(shape, N, gen, share=6):
    """int32 indices in [0, N - 1) -- no list names point N - 1, the index the guards around the lists hold -- with N (the
    empty-ball value) and -1 in about 1 / share of the slots"""
    idx = torch.randint(0, max(N - 1, 1), shape, generator=gen, dtype=torch.int32)
    flat = idx.view(-1)
    if flat.numel() >= 2 and share:
        pick = torch.randperm(flat.numel(), generator=gen)[:max(2, flat.numel() // share)]
        flat[pick[0::2]] = N
        flat[pick[1::2]] = -1
    return idx


# prifit_fps: N (npoint 1 and N, the starts 0 / N - 1 / N // 2 in the three samples)
FPS_N = (1, 2, 255, 256, 257, 513, 1025, 2049, 4095, 4096)
FPS_PPT = {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 513: 4, 1025: 8, 2049: 16, 4095: 16, 4096: 16}


def fps_ppt(N):
    """the instantiation the launcher selects: the least of 1, 2, 4, 8, 16 that holds ceil(N / 256) points per thread"""
    need = -(-N // 256)
    return next(p for p in (1, 2, 4, 8, 16) if need <= p)


THREE_NN_N = (1, 255, 256, 257)
THREE_NN_S = (3, 4, 2047, 2048, 2049)
SQDIST_SIZES = (1, 255, 257)

# prifit_group_gather: (C, order, ld, bytes the output pointer is off 16); B = 3, S = 5, K = 7, N = 37
GATHER_B, GATHER_N, GATHER_S, GATHER_K = 3, 37, 5, 7
GATHER_VECTOR = [(4, 0, 8, 0), (64, 0, 68, 0), (320, 0, 324, 0)]
GATHER_ROW8 = [(0, 0, 8, 0), (1, 0, 8, 0), (3, 0, 8, 0), (5, 0, 8, 0)]
GATHER_SCALAR = [(7, 1, 12, 0), (6, 0, 9, 0), (4, 0, 8, 4), (3, 1, 8, 0)]


def gather_path(C, order, ld, off):
    """the kernel prifit_group_gather selects"""
    if order == 0 and C > 0 and C % 4 == 0 and ld % 4 == 0 and off % 16 == 0:
        return "vector"
    if order == 0 and C <= 5 and ld == 8 and off % 16 == 0:
        return "row8"
    return "scalar"


# prifit_group_scatter_add / prifit_three_interpolate_bwd: (C, col0, ld, hub)
SCATTER_CASES = [(1, 3, 8, False), (3, 1, 4 + 3, True), (64, 4, 72, False), (64, 8, 76, True), (3, 2, 6, False)]
# prifit_three_interpolate / prifit_fp_rows: (C or D2, N, col0, ld pad)
INTERP_CASES = [(1, 1, 0, 0), (3, 37, 2, 3), (24, 37, 8, 0), (130, 1, 0, 4), (130, 37, 1, 1)]
FP_ROWS_CASES = [(D2, D1, pad, N) for D2 in (1, 3, 24, 130) for D1, pad in ((0, 0), (6, 0), (6, 3), (0, 5)) for N in (1, 37)]
INTERP_S = 9
# the column maps of tests/test_gpu_pointops.py: -1 columns, repeated sources
PACK_SHAPES = [(64, 6), (128, 131), (196, 323), (16, 3), (256, 515)]
PACK_MAPS = [(3, 4, 5, 0, 1, 2, -1, -1), tuple(range(3, 131)) + (0, 1, 2) + (-1,), tuple(range(3, 323)) + (0, 1, 2, -1),
             (0, 0, 1, 2), tuple(range(512, 515)) + tuple(range(0, 512)) + (-1,)]


# ---------------------------------------------------------------------------------------------------------------------------
# the front end's rows and slabs
# ---------------------------------------------------------------------------------------------------------------------------
def row_block(C):
    """rows of one unrolled step of the emission: 64 / (C / 4) rows per wave instruction, 4 in flight"""
    return 64 // (C // 4) * 4


def waves_per_group(B, S):
    return 8 if B * -(-S // 8) >= 1024 else 4


SG_WIDTHS = (16, 32, 64, 128)
SG_PARTIAL_K = (1, 7, 65)
SG_FULL = ((16, 128, 32, 64), (64, 128, 96, 32))        # widths, nsample: sum 320, every K a whole number of row blocks
# direct mode: (D, feat_first, B, S, N, rotation of SG_PARTIAL_K over the four widths)
SG_DIRECT = [(D, ff, B, S, N, rot) for (D, ff), (B, S, N), rot in zip(
    [(0, 0), (0, 1), (3, 0), (3, 1), (6, 0), (6, 1)],
    [(1, 1, 1), (3, 5, 65), (9, 9, 65), (1, 9, 2048), (3, 1, 65), (3, 9, 1)], (0, 1, 2, 0, 1, 2))]
SG_DIRECT.append((3, 1, 3, 5, 65, "full"))
# gather mode: (which of Y / slab / bias is NULL, B, S, N, rotation)
SG_GATHER = [("none", 3, 5, 65, 0), ("Y", 3, 9, 65, 1), ("slab", 1, 5, 2048, 2), ("bias", 9, 1, 65, 0), ("none", 3, 5, 65, "full")]
SG_EIGHT_WAVE = dict(B=8, S=1021, N=64, K=4, C=16)


def sg_shape(rot):
    """-> widths, nsample of a launch with four radii"""
    if rot == "full":
        return SG_FULL
    return SG_WIDTHS, tuple(SG_PARTIAL_K[(i + rot) % 3] for i in range(4))


def sg_case(B, S, N, D, C_list, seed, far=True):
    """Lattice cloud, centres, features ([xyz | extra] so that feat_xyz is allowed), weights, biases, U / Vc per radius"""
    gen = gen_of(seed_of(42, B, S, N, D, len(C_list), seed))
    xyz = lattice_cloud("lattice", B, N, gen)
    ctr = xyz[:, torch.randint(0, N, (S,), generator=gen)].clone()
    if far and S > 1:
        ctr[:, S - 1] = FAR
    feat = None
    if D:
        feat = torch.cat([xyz] + ([torch.randn(B, N, D - 3, generator=gen).to(F32)] if D > 3 else []), -1)
    return dict(xyz=xyz, ctr=ctr, feat=feat, W=[(0.5 * torch.randn(C, D + 3, generator=gen)).to(F32) for C in C_list],
                bias=[torch.randn(C, generator=gen).to(F32) for C in C_list],
                U=[torch.randn(B, N, C, generator=gen).to(F32) for C in C_list],
                Vc=[torch.randn(B, S, C, generator=gen).to(F32) for C in C_list])


# prifit_sa_point_tables: (D, feat_first, widths, bias given); B = 3, N = 65, S = 5
TABLES_CASES = [(D, (i + j) % 2, w, bool((i + j // 2) % 2)) for i, D in enumerate((0, 3, 6, 9))
                for j, w in enumerate(((4, 128), (12, 64, 16), (4, 128), (12, 64, 16)))]
TABLES_B, TABLES_N, TABLES_S = 3, 65, 5

# the weight gradient: P = B S K -> (B, S, K); (P, C, D, feat_first)
DW_SHAPES = {1: (1, 1, 1), 255: (3, 5, 17), 256: (1, 4, 64), 257: (1, 257, 1), 1000: (1, 8, 125)}
DW_CASES = [(P, C, (0, 3, 6)[(i + j) % 3], (i + j // 2) % 2) for i, P in enumerate(sorted(DW_SHAPES)) for j, C in enumerate(SG_WIDTHS)]
DW_N = 37


def dw_nblocks(P):
    return (1, 3, -(-P // 256) + 2)


def settle_shift(y, scale, shift, gen):
    """shift [C] redrawn wherever a pre-activation scale y + shift of the column comes closer to 0 than the margin"""
    shift = shift.clone()
    for _ in range(400):
        bad = act_violations(y, scale, shift, 0).any(0)
        if not bool(bad.any()):
            return shift
        shift = torch.where(bad, signed(shift.numel(), 0.1, 1.0, gen), shift)
    raise AssertionError("settle_shift did not converge")


def dw_case(P, C, D, feat_first):
    """Inputs of the three weight-gradient forms on ONE case: dY = G for the plain form; (G, Y1, tables) for _dw_bn; (G, U, Vc,
    tables) with Y1 == U_j - Vc bit for bit for _dw_bn_gather.  Index lists hold N and -1."""
    B, S, K = DW_SHAPES[P]
    N = DW_N
    gen = gen_of(seed_of(43, P, C, D, feat_first))
    xyz, ctr = torch.randn(B, N, 3, generator=gen).to(F32), torch.randn(B, S, 3, generator=gen).to(F32)
    feat = torch.randn(B, N, D, generator=gen).to(F32) if D else None
    idx = oob_index((B, S, K), N, gen, share=6 if P > 1 else 0)
    U, Vc = on_lattice((B, N, C), gen, Y1_GRID, 2.0), on_lattice((B, S, C), gen, Y1_GRID, 2.0)
    u, ok = take_rows(U, idx)
    # (an entry outside the cloud: the gather form re-forms y1 from row 0 of U; its x row is zero, so that y1 never counts)
    u0 = U[:, :1].unsqueeze(1).expand(B, S, K, C)
    Y1 = (torch.where(ok.unsqueeze(-1), u, u0) - Vc.unsqueeze(2)).reshape(P, C)
    scale, ca = signed(C, 0.5, 1.5, gen), signed(C, 0.5, 1.5, gen)
    shift = settle_shift(Y1, scale, signed(C, 0.1, 1.0, gen), gen)
    moved = nudge_act(Y1, scale, shift, 0)
    assert torch.equal(moved, Y1) and not bool(act_violations(Y1, scale, shift, 0).any())
    return dict(B=B, S=S, K=K, N=N, P=P, C=C, D=D, feat_first=feat_first, xyz=xyz, ctr=ctr, feat=feat, idx=idx, U=U, Vc=Vc, Y1=Y1,
                scale=scale, shift=shift, ca=ca, cb=(0.1 * torch.randn(C, generator=gen)).to(F32),
                cd=(0.1 * torch.randn(C, generator=gen)).to(F32), G=torch.randn(P, C, generator=gen).to(F32))


def dw_violations(case):
    return int(act_violations(case["Y1"], case["scale"], case["shift"], 0).sum())


# the chained test: tables -> front end (gather mode) -> fused-BatchNorm weight gradient
CHAIN = dict(B=3, N=65, S=5, K=7, C=64, D=3, feat_first=1, r2u=R2_BIG)


def chain_case():
    c = dict(CHAIN)
    gen = gen_of(seed_of(44, c["N"], c["C"]))
    B, N, S, K, C, D = c["B"], c["N"], c["S"], c["K"], c["C"], c["D"]
    xyz = lattice_cloud("lattice", B, N, gen)
    ctr = xyz[:, torch.randint(0, N, (S,), generator=gen)].clone()
    ctr[:, S - 1] = FAR
    c.update(xyz=xyz, ctr=ctr, feat=torch.randn(B, N, D, generator=gen).to(F32), W=(0.5 * torch.randn(C, D + 3, generator=gen)).to(F32),
             bias=torch.randn(C, generator=gen).to(F32), scale=signed(C, 0.5, 1.5, gen), ca=signed(C, 0.5, 1.5, gen),
             cb=(0.1 * torch.randn(C, generator=gen)).to(F32), cd=(0.1 * torch.randn(C, generator=gen)).to(F32),
             G=torch.randn(B * S * K, C, generator=gen).to(F32))
    f = chain_forward(c)
    # (the rows of an empty ball are excluded from nothing: their y1 is re-formed from row 0 of U and multiplies a zero x row)
    c["shift"] = settle_shift(chain_y1(c, f).reshape(-1, C).to(F32), c["scale"], signed(C, 0.1, 1.0, gen), gen)
    assert not bool(act_violations(chain_y1(c, f).reshape(-1, C), c["scale"], c["shift"], 0).any())
    return c


def chain_forward(c, dtype=F64):
    U, Vc = point_tables(c["xyz"], c["ctr"], c["feat"], c["W"], c["bias"], c["feat_first"], dtype)
    idx = ball_query(c["xyz"], c["ctr"], c["r2u"] * UNIT2, c["K"])
    return dict(U=U, Vc=Vc, idx=idx, Y=gather_layer(U, Vc, None, idx, dtype))


def chain_y1(c, f):
    """what the weight-gradient kernel re-forms: U[idx in range ? idx : 0] - Vc"""
    N = c["N"]
    ok = (f["idx"] >= 0) & (f["idx"] < N)
    u, _ = take_rows(f["U"], torch.where(ok, f["idx"], 0))
    return u - f["Vc"].unsqueeze(2)


def chain_dw(c, f, dtype=F64):
    P = c["B"] * c["S"] * c["K"]
    dY = bn_dy(c["G"], chain_y1(c, f).reshape(P, -1), c["scale"], c["shift"], c["ca"], c["cb"], c["cd"], dtype)
    rows = grouped_rows(c["xyz"], c["ctr"], c["feat"], f["idx"], c["feat_first"], dtype)
    return first_layer_dw(dY, rows, dtype), first_layer_dw_absum(dY, rows)


def fps_Bs(N):
    return (1, 3) if N <= 1025 else (3,)


def fps_cloud(kind, B, N):
    """the lattice clouds of the FPS cases (kind: lattice / same)"""
    return lattice_cloud(kind, B, N, gen_of(seed_of(40, N, B)))


def sqdist_case(S, N, B):
    gen = gen_of(seed_of(46, S, N, B))
    return lattice_cloud("lattice", B, S, gen), lattice_cloud("lattice", B, N, gen)


EXACT_K = 64
EXACT_K_CASE = (300, 3, (0,), 3, EXACT_K)              # arguments of ball_case: radius 0, the centre's copies are the ball
K_MAX_CASES = [(N, 3, (R2_ALL,), 1) for N in (63, 1500)]


def ball_Bs(N):
    return (1, 3) if N <= 2048 else (1,)


def ball_Ss(N):
    return BALL_S if N <= 2048 else (1, 9)


def front_cases():
    """arguments of sg_case of every front-end case of the GPU file"""
    out = [(B, S, N, D, sg_shape(rot)[0], 1) for D, _, B, S, N, rot in SG_DIRECT]
    out += [(B, S, N, 0, sg_shape(rot)[0], 2) for _, B, S, N, rot in SG_GATHER]
    e = SG_EIGHT_WAVE
    return out + [(e["B"], e["S"], e["N"], 3, [e["C"]], 3), SG_REJECT_CASE]


SG_REJECT_CASE = (1, 3, 65, 3, [16, 128, 32, 64], 4)


def lattice_cases():
    """(label, src, dst) of EVERY pair of lattice clouds whose expanded-form distances the GPU file takes as exact (the FPS
    clouds, whose direct distances count: fps_cloud)"""
    out = []
    for N in BALL_N + BALL_N_QUERY_ONLY:
        for S in ball_Ss(N):
            for r2u, _ in BALL_RK:
                for B in ball_Bs(N):
                    xyz, ctr = ball_case(N, S, r2u, B)
                    out.append(("ball(%d, %d, %d, %d)" % (N, S, len(r2u), B), ctr, xyz))
    for args in [EXACT_K_CASE] + K_MAX_CASES:
        xyz, ctr = ball_case(*args)
        out.append(("ball%s" % (args,), ctr, xyz))
    for N in THREE_NN_N:
        for S in THREE_NN_S:
            for B in (1, 3):
                q, p = nn_case(N, S, B)
                out.append(("nn(%d, %d, %d)" % (N, S, B), q, p))
    for S in SQDIST_SIZES:
        for N in SQDIST_SIZES:
            for B in (1, 3):
                out.append((("sqdist(%d, %d, %d)" % (S, N, B),) + sqdist_case(S, N, B)))
    for args in front_cases():
        c = sg_case(*args)
        out.append(("front%s" % (args[:4],), c["ctr"], c["xyz"]))
    c = chain_case()
    out.append(("chain", c["ctr"], c["xyz"]))
    return out


def nn_case(N, S, B):
    """queries [B, N, 3] and candidates [B, S, 3] on the lattice; half of the queries coincide with a candidate"""
    gen = gen_of(seed_of(45, N, S, B))
    p = lattice_cloud("lattice", B, S, gen)
    q = lattice_cloud("lattice", B, N, gen)
    pick = torch.randint(0, S, (N,), generator=gen)
    half = torch.arange(N) % 2 == 0
    q[:, half] = p[:, pick[half]]
    return q, p

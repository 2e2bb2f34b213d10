"""Restatements of the cluster-selection stage in plain torch, the input families of tests/test_gpu_cluster_select_guards.py
and the comparison helpers.  The stage sits between the mean-shift trajectory and the primitive fit: the symmetric
chord / gram / mask product (src/mean_shift.py:154,168,185), the k-th smallest entry of every row (:156-158), nms (:162-202),
the soft membership (:230-247), the double normalisation of the embedding and the mean-shift update (:70-82).

Two kinds of restatement:
  - selection steps (owner, counts, pick, compaction, k-th value, keys, mask) are integer or compare-only work ON THE KERNEL'S
    OWN float32 INPUT, so they are exact: "first minimum" and "first maximum" are written out (the smallest index among the
    entries equal to the extreme value), never taken from the index convention of torch.min / torch.max;
  - continuous formulas (the products, labels' dot products, membership, normalisations, the update) take a dtype: float64 is the
    reference, float32 -- dot products added in k order, one rounding per multiply and per add -- gives the error a plain float32
    evaluation of the same formula makes on the same inputs.  The bars are MARGIN x that error (fit_common.check).

A discrete decision that rests on a continuous quantity (a label = the larger of two dot products, the gate of a clamp, the
branch of a normalisation) is compared only where float64 decides it by more than LEAVE_OUT x the float32 restatement's worst
error on that case; tests/test_cluster_select_restatement.py asserts on every input family that at most CAP_LEFT_OUT of a case
is left out, and nothing at all in the separated-cluster families."""
import functools

import numpy as np
import torch

from fit_common import EPS32, F32, F64, MARGIN, assert_bars, check, rel_err  # noqa: F401  (re-exported to the test modules)

LEAVE_OUT = 8.0         # x the float32 restatement's worst error: closer to a decision edge than this = left out
CAP_LEFT_OUT = 0.01     # at most this fraction of a case's points / elements
NMS_CAP = 64            # fit_ops.NMS_CAP
BW_MID = 0.3            # the "separated clusters" threshold: one centre per cluster
BW_HUGE = 5.0           # above every chord distance (<= 4): one centre remains


def gen_of(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (hash(k) if not isinstance(k, str) else sum(ord(c) * (i + 1) for i, c in enumerate(k)))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------
# first extreme, written out
# ---------------------------------------------------------------------------------------------------------------------------
def first_min(M, dim):
    """-> (min value, smallest index holding it) along `dim`.  By value: -0 == +0, as `<` in the kernels."""
    m = M.min(dim=dim, keepdim=True).values
    n = M.shape[dim]
    shape = [1] * M.dim()
    shape[dim] = n
    idx = torch.arange(n).view(shape).expand_as(M)
    first = torch.where(M == m, idx, torch.full_like(idx, n)).min(dim=dim).values
    return m.squeeze(dim), first


def first_max(M, dim):
    v, i = first_min(-M, dim)
    return -v, i


# ---------------------------------------------------------------------------------------------------------------------------
# products
# ---------------------------------------------------------------------------------------------------------------------------
def dots(A, Bm, dtype=F64):
    """A [.., n, K] . Bm [.., m, K] -> [.., n, m].  float64: matmul.  float32: sum_k a_k b_k added in k order, every product
    and every sum rounded once (no fused multiply-add, no blocked partial sums): bitwise symmetric when A is Bm."""
    A, Bm = A.to(dtype), Bm.to(dtype)
    if dtype == F64:
        return A @ Bm.transpose(-1, -2)
    acc = torch.zeros(A.shape[:-1] + (Bm.shape[-2],), dtype=dtype)
    for k in range(A.shape[-1]):
        acc = acc + A[..., :, k].unsqueeze(-1) * Bm[..., :, k].unsqueeze(-2)
    return acc


def chord(A, Bm, dtype=F64):
    """2 - 2 A Bm^T (src/mean_shift.py:154)."""
    return 2.0 - 2.0 * dots(A, Bm, dtype)


def chord_input(A, Bm=None):
    """A float32 chord matrix to hand to nms as its input: the float64 product rounded once, made bitwise symmetric when the
    point set is paired with itself (nms_owner_kernel reads a column's minimum as a row's)."""
    M = chord(A, A if Bm is None else Bm).to(F32)
    if Bm is None:
        M = torch.triu(M) + torch.triu(M, 1).transpose(-1, -2)
    return M.contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# keys and mask of the symmetric kernel, restated on a float32 matrix C [n, n]
# ---------------------------------------------------------------------------------------------------------------------------
def float_key(x):
    """Order-preserving unsigned image of float32 values -> numpy uint64 (< 2^32)."""
    u = x.contiguous().view(torch.int32).numpy().astype(np.int64) & 0xffffffff
    return np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000).astype(np.uint64)


def owner_keys(C):
    """C [.., n, n] float32 -> int64 [.., n]: key of point j = float_key(min_i C[i][j]) << 32 | first argmin."""
    m, arg = first_min(C, -2)
    key = (float_key(m) << np.uint64(32)) | arg.numpy().astype(np.uint64)
    return torch.from_numpy(key.view(np.int64).copy())


def pack_mask(near):
    """bool [.., n, n] -> int32 words [.., n, n / 32]: bit col % 32 of word col / 32."""
    n = near.shape[-1]
    w = near.view(near.shape[:-1] + (n // 32, 32)).numpy().astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return torch.from_numpy(w.sum(-1).astype(np.uint32).view(np.int32).copy())


def unpack_mask(words, n):
    w = words.numpy().view(np.uint32).astype(np.uint64)
    bits = (w[..., None] >> np.arange(32, dtype=np.uint64)) & np.uint64(1)
    return torch.from_numpy(bits.astype(bool).reshape(words.shape[:-1] + (n,)))


# ---------------------------------------------------------------------------------------------------------------------------
# nms (src/mean_shift.py:162-202), one shape
# ---------------------------------------------------------------------------------------------------------------------------
def nms_select(own_src, near, cap=NMS_CAP, owner=None):
    """The compare-only part.  own_src [N, N] float32: row j = the distances of point j to every centre, owner[j] = its first
    minimum (or `owner` given, from the keys); near bool [N, N]: near[u][j] = centre j is within the bandwidth of centre u.
    -> owner, counts, flags [N], ids [cap] (ascending flagged ids in [:min(count, cap)], 0 behind), count (may exceed cap)."""
    N = near.shape[0]
    if owner is None:
        _, owner = first_min(own_src, 1)
    counts = torch.bincount(owner, minlength=N)
    V = torch.where(near, counts.unsqueeze(0).expand(N, N), torch.zeros(N, N, dtype=counts.dtype))
    _, chosen = first_max(V, 1)             # (no neighbour with a count: every entry 0, the first maximum is column 0)
    flags = torch.zeros(N, dtype=torch.int64)
    flags[chosen[counts > 0]] = 1
    flagged = torch.nonzero(flags).view(-1)     # ascending
    count = int(flagged.numel())
    ids = torch.zeros(cap, dtype=torch.int64)
    ids[:min(count, cap)] = flagged[:cap]
    return dict(owner=owner, counts=counts, flags=flags, ids=ids, count=count)


def nms_labels(X, Cen, ids, count, cap=NMS_CAP, dtype=F64):
    """labels[j] = first argmax_k <Cen[ids[k]], X[j]> over the first min(count, cap) centres -> labels, margin (top minus second
    dot product; inf with one centre), second (the runner-up's slot), the dot products."""
    K = min(count, cap)
    d = dots(X, Cen[ids[:K]], dtype)
    top, lab = first_max(d, 1)
    if K > 1:
        rest = d.clone()
        rest[torch.arange(d.shape[0]), lab] = -float("inf")
        sec, second = first_max(rest, 1)
    else:
        sec, second = torch.full_like(top, -float("inf")), lab
    return lab, top - sec, second, d


def nms_reference(own_src, near, X, Cen, cap=NMS_CAP, owner=None):
    """Everything nms writes for one shape + which points are left out of the label comparison -> dict."""
    out = nms_select(own_src, near, cap, owner)
    lab, margin, second, d64 = nms_labels(X, Cen, out["ids"], out["count"], cap, F64)
    _, _, _, d32 = nms_labels(X, Cen, out["ids"], out["count"], cap, F32)
    err32 = float((d32.double() - d64).abs().max())
    left = margin < LEAVE_OUT * err32
    used_lo = torch.zeros(cap, dtype=torch.int64)
    used_lo[lab[~left]] = 1
    used_hi = used_lo.clone()
    used_hi[lab[left]] = 1
    used_hi[second[left]] = 1
    out.update(labels=lab, margin=margin, left=left, err32=err32, used_lo=used_lo, used_hi=used_hi)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# input families: unit rows
# ---------------------------------------------------------------------------------------------------------------------------
def prototypes(D, gen):
    """Up to six mutually orthogonal (D = 3: the six axis directions) unit vectors."""
    if D < 6:
        eye = torch.eye(D, dtype=F64)
        return torch.cat([eye, -eye])[:6]
    q, _ = torch.linalg.qr(torch.randn(D, 6, generator=gen, dtype=F64))
    return q.t().contiguous()


def separated(N, D, *key, spread=0.05, proto=None):
    """Separated clusters: rows at an angle of ~`spread` around orthogonal prototypes (dot products of ~1 inside a cluster,
    <= ~0 across).  float32 [N, D]."""
    gen = gen_of("separated", N, D, *key)
    if proto is None:
        proto = prototypes(D, gen_of("proto", D))
    lab = torch.randint(0, proto.shape[0], (N,), generator=gen)
    X = proto[lab] + spread / D ** 0.5 * torch.randn(N, D, generator=gen, dtype=F64)
    return torch.nn.functional.normalize(X, dim=1).to(F32)


def collapsed(N, D, *key):
    """A collapsed cloud: every row within 1e-7 of one unit vector -- chord distances of a few ulp of 1 around zero, many exact
    ties, negative values."""
    gen = gen_of("collapsed", N, D, *key)
    base = torch.nn.functional.normalize(torch.randn(1, D, generator=gen, dtype=F64), dim=1)
    X = base + 1e-7 / D ** 0.5 * torch.randn(N, D, generator=gen, dtype=F64)
    return torch.nn.functional.normalize(X, dim=1).to(F32)


def duplicated(N, D, *key):
    """Separated clusters with exact duplicate rows: row j + 128 t (another 128-row tile where N allows, j + 64 t in the same
    tile otherwise) = row j for a few j -- the same minimum distance at two indices of different tiles."""
    X = separated(N, D, "dup", *key).clone()
    step = 128 if N > 128 else max(1, N // 2)
    for j in (0, 5, 77 % step, step - 1):
        for t in range(1, (N - 1 - j) // step + 1):
            X[j + step * t] = X[j]
    return X


FAMILIES = {"separated": separated, "collapsed": collapsed, "duplicated": duplicated}


# ---------------------------------------------------------------------------------------------------------------------------
# symmetric kernel cases
# ---------------------------------------------------------------------------------------------------------------------------
SYM_N = (128, 256, 384)
SYM_K = (32, 64, 128, 160)
SYM_BATCH = (1, 3, 9, 11)       # 9 and 11 take both branches of xcd_shape_block (eight shapes round-robin, then the tail)
SYM_BMAX = max(SYM_BATCH)


@functools.lru_cache(maxsize=4)
def sym_case(family, n, K):
    """A [SYM_BMAX, n, K] float32 (smaller batches take its first shapes) with the float64 and float32 chord and gram."""
    A = torch.stack([FAMILIES[family](n, K, z) for z in range(SYM_BMAX)])
    g64, g32 = dots(A, A, F64), dots(A, A, F32)
    return dict(A=A, gram64=g64, gram32=g32, chord64=2.0 - 2.0 * g64, chord32=2.0 - 2.0 * g32)


def thresholds(C, rot):
    """One threshold per shape of C [B, n, n], shape z of kind (z + rot) % 3: 0 = the minimum of C (strict `<`: no bit set),
    1 = above its maximum (every bit set), 2 = exactly one of its values (the median: that element's bit clear)."""
    out = []
    for z in range(C.shape[0]):
        kind = (z + rot) % 3
        flat = C[z].reshape(-1)
        out.append(flat.min() if kind == 0 else (flat.max() + 1.0 if kind == 1 else flat.sort().values[flat.numel() // 2]))
    return torch.stack(out).to(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# k-th smallest
# ---------------------------------------------------------------------------------------------------------------------------
KTH_C = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 516, 1024, 1028, 2048, 2052, 4095, 4096)
KTH_ROWS = (1, 5, 37)
KTH_FAMILIES = ("distinct", "signed_zero", "constant", "shared_top_bits", "three_values", "kth_duplicated")


def kth_ks(C):
    return sorted({min(max(k, 1), C) for k in (1, 2, 64, 65, 255, 256, 257, C - 1, C)})


def kth_rows(family, rows, C, k):
    """float32 [rows, C].  Only "kth_duplicated" depends on k."""
    gen = gen_of("kth", family, rows, C, k if family == "kth_duplicated" else 0)
    perm = torch.stack([torch.randperm(C, generator=gen) for _ in range(rows)])
    if family == "distinct":
        return ((perm.to(F32) - C // 2) * 0.37 + 0.11).contiguous()            # distinct, both signs
    if family == "signed_zero":
        M = torch.randn(rows, C, generator=gen)
        z = torch.rand(rows, C, generator=gen)
        M[z < 0.2] = 0.0
        M[z < 0.1] = -0.0
        return M
    if family == "constant":
        return torch.full((rows, C), 0.625) * torch.arange(1, rows + 1).view(rows, 1).to(F32)
    if family == "shared_top_bits":
        return (1.0 + perm.to(F64) * 2.0 ** -23).to(F32)                          # exact: C <= 2^12
    if family == "three_values":
        return torch.tensor([-1.5, 0.25, 3.0])[torch.randint(0, 3, (rows, C), generator=gen)]
    if family == "kth_duplicated":
        rank = perm.clone()                                   # rank of every entry; ranks k - 3 .. k + 2 share one value
        lo, hi = max(k - 3, 0), min(k + 2, C - 1)
        rank[(rank >= lo) & (rank <= hi)] = lo
        return (rank.to(F32) * 0.5 - 7.0).contiguous()
    raise KeyError(family)


def kth_expected(M, k):
    return torch.topk(M, k, dim=1, largest=False).values[:, -1]


# ---------------------------------------------------------------------------------------------------------------------------
# nms cases
# ---------------------------------------------------------------------------------------------------------------------------
NMS_N = (1, 2, 63, 64, 65, 300, 511, 512, 513, 1030)
NMS_D = (3, 32, 128, 256)
NMS_FAMILY = ("own_centre", "one_centre", "separated")     # shape z of a case: its bandwidth below


def spread_of(D, z):
    """Angular cluster radius.  The separated shapes: 0.05 (D = 3: 0.1), every chord inside a cluster far below BW_MID.  Shape
    0, where every point is to own itself and the labels are taken over up to 64 centres of which several lie in a point's own
    cluster: 0.5, so that the closest pair stays further apart than float32 resolves around 1 (1030 points on six caps of the
    sphere at D = 3) and the dot products to neighbouring centres differ by more than their float32 error."""
    return 0.5 if z == 0 else (0.1 if D == 3 else 0.05)


def small_bandwidth(dist_cc):
    """Half the smallest off-diagonal chord distance (1e-4 for a single point): above the diagonal's rounding (|d_uu| <~ 2e-7),
    below every other distance, so every point owns itself and picks itself."""
    N = dist_cc.shape[0]
    if N == 1:
        return 1e-4
    off = dist_cc + torch.diag(torch.full((N,), float("inf")))
    return 0.5 * float(off.min())


def _nms_draw(N, D, pair, draw):
    proto = prototypes(D, gen_of("proto", D))
    X = torch.stack([separated(N, D, "nms", z, draw, spread=spread_of(D, z), proto=proto) for z in range(3)])
    Cen = torch.stack([separated(N, D, "cen", z, draw, spread=spread_of(D, z), proto=proto) for z in range(3)]) if pair else X
    dist_cc = chord_input(Cen)
    dist_xc = chord_input(X, Cen) if pair else dist_cc
    bw = torch.tensor([small_bandwidth(dist_cc[0]), BW_HUGE, BW_MID], dtype=F32)
    return dict(X=X, Cen=Cen, dist_xc=dist_xc, dist_cc=dist_cc, bw=bw, pair=pair)


def left_out_ok(left, none):
    n = int(left.sum())
    return n == 0 if none else n <= CAP_LEFT_OUT * max(int(left.numel()), 1)


@functools.lru_cache(maxsize=4)
def nms_case(N, D, pair=False):
    """B = 3 shapes with the bandwidths (every owner keeps itself, one centre remains, BW_MID).  pair: centres C that are not
    the points X (another draw around the same prototypes) and the non-symmetric point x centre matrix.  A draw whose float64
    reference leaves out more than the cap allows (a near-tie of two dot products among a few dozen points) is drawn again;
    case["refs"]: nms_reference of every shape."""
    for draw in range(8):
        case = _nms_draw(N, D, pair, draw)
        case["refs"] = nms_case_reference(case)
        if all(left_out_ok(r["left"], fam != "own_centre") for fam, r in zip(NMS_FAMILY, case["refs"])):
            return case
    raise AssertionError("no draw of nms_case(%d, %d, %s) within the left-out cap" % (N, D, pair))


def nms_case_reference(case, dist_xc=None, dist_cc=None, cap=NMS_CAP):
    """nms_reference of every shape of a case (on other float32 matrices when given: the symmetric kernel's own output)."""
    dist_xc = case["dist_xc"] if dist_xc is None else dist_xc
    dist_cc = case["dist_cc"] if dist_cc is None else dist_cc
    return [nms_reference(dist_xc[z], dist_cc[z] < case["bw"][z], case["X"][z], case["Cen"][z], cap) for z in range(len(case["bw"]))]


def assert_left_out(left, none, what=""):
    """The cap on what a case may leave out of a discrete comparison."""
    n, tot = int(left.sum()), max(int(left.numel()), 1)
    if none:
        assert n == 0, "%s: %d of %d left out in a family that must leave out none" % (what, n, tot)
    assert n <= CAP_LEFT_OUT * tot, "%s: %d of %d left out (> %g)" % (what, n, tot, CAP_LEFT_OUT)


# ---------------------------------------------------------------------------------------------------------------------------
# nms on the mask
# ---------------------------------------------------------------------------------------------------------------------------
MASK_N = (128, 256, 384, 2176)      # 2176 / 32 = 68 mask words: the second trip of the lanes' word loop
MASK_D = (32, 128)


@functools.lru_cache(maxsize=2)
def mask_case(N, D):
    """B = 2: shape 0 with the bandwidth under which every owner keeps itself, shape 1 at BW_MID."""
    X = torch.stack([separated(N, D, "mask", z, spread=spread_of(D, z)) for z in range(2)])
    bw = torch.tensor([small_bandwidth(chord_input(X[0])), BW_MID], dtype=F32)
    return dict(X=X, Cen=X, bw=bw)


def handmade_mask(near, counts):
    """near bool [N, N] with two rows of owning centres replaced: the first owner's row all zero, the last owner's row with bits
    only under zero counts (when there are any).  Either way the pick finds no neighbour with a count: column 0."""
    near = near.clone()
    owners = torch.nonzero(counts > 0).view(-1)
    near[owners[0]] = False
    near[owners[-1]] = counts == 0
    return near


# ---------------------------------------------------------------------------------------------------------------------------
# membership (src/mean_shift.py:230-247)
# ---------------------------------------------------------------------------------------------------------------------------
MEM_N = (1, 255, 256, 257, 300)
MEM_KM = (1, 4, 5, 32, 33)
MEM_B = 4
CLAMP_LO, CLAMP_HI = -13.0, 75.0


def membership(d, bw, gmax, count, dtype=F64):
    """d [B, N, KM] raw dot products -> W [B, N, KM] (0 at slots k >= min(count, KM)), the exponent s before the clamp."""
    B, N, KM = d.shape
    d, bw, gmax = d.to(dtype), bw.to(dtype), gmax.to(dtype)
    s = d / (bw * bw).view(B, 1, 1) - gmax.view(B, 1, 1)
    e = torch.exp(s.clamp(CLAMP_LO, CLAMP_HI))
    live = (torch.arange(KM).view(1, 1, KM) < count.view(B, 1, 1)).expand(B, N, KM)
    e = torch.where(live, e, torch.zeros_like(e))
    tot = e.sum(-1, keepdim=True)
    W = torch.where(live, e / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.zeros_like(e))
    return W, s, live


@functools.lru_cache(maxsize=4)
def membership_case(N, KM):
    """count = 0, 1, a middle value, KM + 7; dot products in [-1, 1], b = 0.1 and gmax = -30: s in [-70, 130], below the lower
    clamp, inside and above the upper clamp on different elements of every row (KM >= 4)."""
    gen = gen_of("membership", N, KM)
    d = (2.0 * torch.rand(MEM_B, N, KM, generator=gen) - 1.0).to(F32)
    bw = torch.tensor([0.1, 0.1, 0.11, 0.09], dtype=F32)
    gmax = torch.tensor([-30.0, -30.0, -25.0, -35.0], dtype=F32)
    count = torch.tensor([0, 1, (KM + 1) // 2, KM + 7])
    gW = torch.randn(MEM_B, N, KM, generator=gen).to(F32)
    return dict(dots=d, bw=bw, gmax=gmax, count=count, gW=gW)


def membership_reference(case):
    """W, gdots in float64 and float32 (autograd of the restatement), the gate (clamp inactive), dead slots and the elements left
    out of the gdots comparison: exponent closer to a clamp edge than LEAVE_OUT x the float32 restatement's worst error in it."""
    out = {}
    for name, dtype in (("64", F64), ("32", F32)):
        d = case["dots"].detach().to(dtype).clone().requires_grad_(True)
        W, s, live = membership(d, case["bw"], case["gmax"], case["count"], dtype)
        (W * case["gW"].to(dtype)).sum().backward()
        out["W" + name], out["s" + name], out["g" + name] = W.detach(), s.detach(), d.grad
    out["live"] = live
    s64 = out["s64"]
    out["err32"] = float((out["s32"].double() - s64).abs().max())
    edge = torch.minimum((s64 - CLAMP_LO).abs(), (s64 - CLAMP_HI).abs())
    out["left"] = live & (edge < LEAVE_OUT * out["err32"])
    out["clamped"] = live & ((s64 < CLAMP_LO) | (s64 > CLAMP_HI))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# normalize(normalize(x)) (convex_loss.py:41,57) and the mean-shift update (src/mean_shift.py:70-82)
# ---------------------------------------------------------------------------------------------------------------------------
ROW_D = (1, 3, 32, 63, 64, 65, 128, 255, 256)
ROW_ROWS = (1, 5, 130)
EPS_NORM = 1e-12
ROW_CLASSES = ("regular", "zero", "norm_1e-13", "norm_1e-20")


def normalize2(x, dtype=F64, eps=EPS_NORM):
    x = x.to(dtype)
    return torch.nn.functional.normalize(torch.nn.functional.normalize(x, dim=-1, eps=eps), dim=-1, eps=eps)


@functools.lru_cache(maxsize=4)
def normalize2_case(rows, D):
    """Rows of norm O(1), with (from 5 rows up) a zero row, a row of norm 1e-13 (below eps) and one of norm 1e-20; the single-row
    shape cycles through the four classes with D.  cls [rows]: index into ROW_CLASSES."""
    gen = gen_of("normalize2", rows, D)
    x = torch.randn(rows, D, generator=gen, dtype=F64) * (0.5 + 3.0 * torch.rand(rows, 1, generator=gen, dtype=F64))
    cls = torch.zeros(rows, dtype=torch.int64)
    if rows == 1:
        cls[0] = ROW_D.index(D) % 4
    else:
        cls[1], cls[2], cls[rows - 1] = 1, 2, 3
    unit = torch.nn.functional.normalize(x, dim=1)
    x = torch.where((cls == 1).view(-1, 1), torch.zeros_like(x), x)
    x = torch.where((cls == 2).view(-1, 1), 1e-13 * unit, x)
    x = torch.where((cls == 3).view(-1, 1), 1e-20 * unit, x)
    g = torch.randn(rows, D, generator=gen).to(F32)
    return dict(x=x.to(F32), g=g, cls=cls)


def normalize2_reference(case, dtype=F64):
    """-> y, gx (autograd), and the two norms whose side of eps decides the branch."""
    x = case["x"].detach().to(dtype).clone().requires_grad_(True)
    y = normalize2(x, dtype)
    (y * case["g"].to(dtype)).sum().backward()
    n1 = x.detach().norm(dim=1)
    n2 = (x.detach() / n1.clamp_min(EPS_NORM).unsqueeze(1)).norm(dim=1)
    return y.detach(), x.grad, n1, n2


def update(O, rowsum, Z, dtype=F64):
    """new = Z + (O / rowsum - Z); out = new / |new| -> out, |new|."""
    O, rowsum, Z = O.to(dtype), rowsum.to(dtype), Z.to(dtype)
    new = Z + (O / rowsum.unsqueeze(-1) - Z)
    nrm = new.norm(dim=-1)
    return new / nrm.unsqueeze(-1), nrm


def update_inputs(lead, D, *key):
    """O = K X with positive weights K of row sum `rowsum`, Z unit rows, g a gradient on `out`: float32 tensors [*lead, D]."""
    gen = gen_of("update", D, *key)
    rowsum = (1.0 + 50.0 * torch.rand(*lead, generator=gen)).to(F32)
    Z = torch.nn.functional.normalize(torch.randn(*lead, D, generator=gen, dtype=F64), dim=-1).to(F32)
    O = (rowsum.unsqueeze(-1).double() * (0.7 * Z.double() + 0.3 / D ** 0.5 * torch.randn(*lead, D, generator=gen, dtype=F64))).to(F32)
    g = torch.randn(*lead, D, generator=gen).to(F32)
    return dict(O=O, rowsum=rowsum, Z=Z, g=g)


def update_reference(case, dtype=F64):
    """-> out, nrm, gO, g_rowsum (autograd through out = f(O, rowsum); Z's gradient through Z + (m - Z) is exactly zero)."""
    O = case["O"].detach().to(dtype).clone().requires_grad_(True)
    rs = case["rowsum"].detach().to(dtype).clone().requires_grad_(True)
    out, nrm = update(O, rs, case["Z"], dtype)
    (out * case["g"].to(dtype)).sum().backward()
    return out.detach(), nrm.detach(), O.grad, rs.grad


def update_bwd_free(case, dtype=F64):
    """The backward's formula on inputs `out_free` / `nrm_free` that are NOT the forward's: gnew = (g - out (g . out)) / nrm,
    gO = gnew / rowsum, g_rowsum = -(gnew . O) / rowsum^2.  With the forward's own `out` (parallel to O) g_rowsum is identically
    zero -- the normalisation removes the scale 1 / rowsum -- and what a kernel or the float64 autograd returns for it is the
    rounding of a cancelled sum, nothing a relative bar can be applied to; with an `out` at an angle to O the same arithmetic
    gives a well-conditioned value."""
    g, out, nrm, O, rs = (case[k].to(dtype) for k in ("g", "out_free", "nrm_free", "O", "rowsum"))
    gnew = (g - out * (g * out).sum(-1, keepdim=True)) / nrm.unsqueeze(-1)
    return gnew / rs.unsqueeze(-1), -(gnew * O).sum(-1) / (rs * rs)


def update_free_inputs(case, *key):
    """out_free: unit rows at ~45 degrees to the forward's out; nrm_free in [0.5, 1.5]."""
    gen = gen_of("update_free", case["O"].shape[-1], *key)
    out, _ = update(case["O"], case["rowsum"], case["Z"])
    D = out.shape[-1]
    free = torch.nn.functional.normalize(out + torch.randn(out.shape, generator=gen, dtype=F64) / D ** 0.5, dim=-1)
    case["out_free"] = free.to(F32)
    case["nrm_free"] = (0.5 + torch.rand(out.shape[:-1], generator=gen)).to(F32)
    return case


UPD_B, UPD_N, UPD_GAP = 3, 43, 12       # the backward's batched form: gO_batch_stride = N * D + 12

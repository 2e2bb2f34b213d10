"""Batch augmentation under the reference's names (provider.py:265-303), the ones its trainer calls
(train_partseg_shapenet.py:372-373):

    points[:, :, 0:3] = provider.random_scale_point_cloud(points[:, :, 0:3])
    points[:, :, 0:3] = provider.shift_point_cloud(points[:, :, 0:3])

A numpy batch is handled the reference's way -- one `np.random.uniform` draw per call, in the reference's order, applied in
place and returned -- so a seeded run reproduces the reference's batches bit for bit (tests/golden/data_readers.npz).  A torch
tensor (any device) gets the same law from torch's generator in one batched op on ITS device: that is the form the trainer of
this package uses (`train_step.random_scale_shift`), no host round trip per batch.

The rest of the per-shape affine family -- the rotations and the anisotropic scale, what pretrain_partseg_shapenet.py:319-337
calls -- follows below (`rotate_point_cloud` ... `random_anisotropic_scale_point_cloud`).  Each is one 3x4 matrix per shape.  A
numpy batch again goes the reference's way (same `np.random` draws in the same order, the same products, the same return / in-place
convention).  For a torch tensor the B parameter sets are drawn on the HOST from `generator` (a CPU torch.Generator, default the
global one), the matrices are composed in float64, rounded once to fp32, uploaded in one copy and applied by ONE launch of
`prifit_affine_points` (csrc/augment.hip) when the tensor lives on the GPU; a host tensor takes torch arithmetic in the kernel's
fixed order.  `compose_affine` / `apply_affine` are that machinery in the open: the trainer composes the script's whole chain with
them (train_step.Trainer._selfsup_batch).

The rest of upstream's module closes the file: the xyz + normal rotations, `random_point_dropout`, `shuffle_points`, `shuffle_data`,
`normalize_data`, and `perturb_batch`, which puts map, normals, jitter and dropout into ONE launch of `prifit_perturb_points`
(csrc/perturb.hip) with per-point random numbers from a counter-based generator.
"""
import numpy as np
import torch


def _is_np(x):
    return isinstance(x, np.ndarray)


def random_scale_point_cloud(batch_data, scale_low=0.8, scale_high=1.25, generator=None):
    """One scale per cloud, uniform in [scale_low, scale_high] (provider.py:292-303).  [B,N,3] in, the same object out."""
    B = batch_data.shape[0]
    if _is_np(batch_data):
        scales = np.random.uniform(scale_low, scale_high, B)
        # (float64 draws against a float32 batch: the product is formed in double and rounded once, as the reference's
        # per-cloud `batch_data[b] *= scales[b]` does under this numpy's promotion rules)
        np.multiply(batch_data, scales.reshape(B, 1, 1), out=batch_data, casting="same_kind")
        return batch_data
    scales = torch.empty(B, 1, 1, device=batch_data.device, dtype=batch_data.dtype).uniform_(scale_low, scale_high, generator=generator)
    return batch_data.mul_(scales)


def shift_point_cloud(batch_data, shift_range=0.1, generator=None):
    """One shift per cloud, uniform in [-shift_range, shift_range]^3 (provider.py:278-289)."""
    B = batch_data.shape[0]
    if _is_np(batch_data):
        shifts = np.random.uniform(-shift_range, shift_range, (B, 3))
        np.add(batch_data, shifts.reshape(B, 1, 3), out=batch_data, casting="same_kind")
        return batch_data
    shifts = torch.empty(B, 1, 3, device=batch_data.device, dtype=batch_data.dtype).uniform_(-shift_range, shift_range, generator=generator)
    return batch_data.add_(shifts)


def jitter_point_cloud(batch_data, sigma=0.01, clip=0.05, generator=None):
    """Per-point Gaussian jitter clipped to [-clip, clip] (provider.py:265-276); returns a new batch."""
    assert clip > 0
    if _is_np(batch_data):
        B, N, C = batch_data.shape
        jittered = np.clip(sigma * np.random.randn(B, N, C), -1 * clip, clip)
        jittered += batch_data
        return jittered
    noise = torch.randn(batch_data.shape, device=batch_data.device, dtype=batch_data.dtype, generator=generator)
    return batch_data + (sigma * noise).clamp_(-clip, clip)


# ---------------------------------------------------------------------------------------------------------------------------
# The per-shape affine family: rotations and the anisotropic scale (provider.py:46-147, :197-214, :240-262, :306-317)
# ---------------------------------------------------------------------------------------------------------------------------

def _rot_y(angle):
    """The reference's y ("up") rotation, provider.py:100-102; points are row vectors: rotated = pc . R."""
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s],
                     [0, 1, 0],
                     [-s, 0, c]])


def _rot_z(angle):
    """provider.py:79-81."""
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, s, 0],
                     [-s, c, 0],
                     [0, 0, 1]])


def _rot_perturbation(angles):
    """provider.py:250-259: R = Rz . (Ry . Rx) of three small angles."""
    cx, cy, cz = np.cos(angles)
    sx, sy, sz = np.sin(angles)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.dot(Rz, np.dot(Ry, Rx))


def _rotate_np(batch_data, matrix_of, xyz_only=False):
    """The reference's loop: a fresh float32 batch, shape k = pc_k . matrix_of(k) formed in double (float32 points against a float64
    matrix) and rounded on assignment.  `matrix_of(k)` makes its `np.random` draw when it is called, so the draws come shape by shape
    as upstream.  xyz_only: the `[k, :, 0:3]` form of rotate_point_cloud_by_angle -- further channels stay zero, as upstream."""
    rotated = np.zeros(batch_data.shape, dtype=np.float32)
    for k in range(batch_data.shape[0]):
        R = matrix_of(k)
        if xyz_only:
            rotated[k, :, 0:3] = np.dot(batch_data[k, :, 0:3].reshape((-1, 3)), R)
        else:
            rotated[k, ...] = np.dot(batch_data[k, ...].reshape((-1, 3)), R)
    return rotated


def _affine_of(matrices):
    """[B,3,3] float64 matrices -> [B,12] float32 (A row-major, then t = 0): the single rounding to fp32."""
    B = matrices.shape[0]
    aff = np.zeros((B, 12), dtype=np.float64)
    aff[:, :9] = matrices.reshape(B, 9)
    return aff.astype(np.float32)


def compose_affine(scale=None, shift=None, aniso=None, y_angle=None, y_angle2=None):
    """The chain of pretrain_partseg_shapenet.py:319-337 as one map per shape: p -> ((p * s + t) * a) . Ry(y_angle) . Ry(y_angle2),
    every stage optional.  scale [B], shift [B,3], aniso [B,3] (or the [B,1,3] the reference draws), y_angle / y_angle2 [B] in
    radians, Ry the matrix of provider.py:100-102.  Composed in float64 and rounded once: returns [B,12] float32, a row-major 3x3
    A then t[3] with out = p . A + t (what `apply_affine` and `prifit_affine_points` take)."""
    given = [np.asarray(v) for v in (scale, shift, aniso, y_angle, y_angle2) if v is not None]
    if not given:
        raise ValueError("compose_affine: no parameter given (the batch size is taken from them)")
    B = given[0].shape[0]
    A = np.tile(np.eye(3), (B, 1, 1))
    t = np.zeros((B, 3))
    if scale is not None:
        A = A * np.asarray(scale, dtype=np.float64).reshape(B, 1, 1)
    if shift is not None:
        t = t + np.asarray(shift, dtype=np.float64).reshape(B, 3)
    if aniso is not None:
        a = np.asarray(aniso, dtype=np.float64).reshape(B, 3)
        A = A * a[:, None, :]                   # p . (A diag(a)): column j times a_j
        t = t * a
    for angles in (y_angle, y_angle2):
        if angles is not None:
            R = np.stack([_rot_y(v) for v in np.asarray(angles, dtype=np.float64).reshape(B)])
            A = A @ R
            t = np.einsum("bi,bij->bj", t, R)
    return np.concatenate([A.reshape(B, 9), t], axis=1).astype(np.float32)


def _affine_torch(points, affine):
    """The kernel's expression in torch arithmetic (host tensors): o_j = ((p0*A[0][j] + p1*A[1][j]) + p2*A[2][j]) + t[j] in the
    tensor's own dtype, one rounding per operation, nothing fused."""
    B = points.shape[0]
    aff = affine.to(device=points.device, dtype=points.dtype)
    A, t = aff[:, :9].reshape(B, 1, 3, 3), aff[:, 9:].reshape(B, 1, 3)
    p0, p1, p2 = points[:, :, 0:1], points[:, :, 1:2], points[:, :, 2:3]
    return ((p0 * A[:, :, 0] + p1 * A[:, :, 1]) + p2 * A[:, :, 2]) + t


def _check_affine_args(points, affine):
    if points.dim() != 3 or points.shape[2] < 3:
        raise ValueError("expected a [B,N,3+] batch, got shape %s" % (tuple(points.shape),))
    affine = torch.as_tensor(affine)
    if tuple(affine.shape) != (points.shape[0], 12) or affine.dtype != torch.float32:
        raise ValueError("affine must be float32 [B,12], got %s %s" % (affine.dtype, tuple(affine.shape)))
    return affine


def apply_affine(points, affine, out=None):
    """out[b, n, 0:3] = points[b, n, 0:3] . A_b + t_b, further channels copied; `affine` [B,12] float32 as `compose_affine` returns
    it (numpy or tensor).  points: a [B,N,C] torch tensor.  On the GPU ONE `prifit_affine_points` launch (float32, contiguous,
    C <= 8); on the host torch arithmetic in the same fixed order.  out=None: a new tensor; out=points: in place."""
    affine = _check_affine_args(points, affine)
    if points.is_cuda:
        from . import ops
        return ops.affine_points(points, affine, out_cl=out, want_cl=True)[0]
    xyz = _affine_torch(points, affine)
    if out is None:
        out = points.clone()
    elif out is not points:
        out.copy_(points)
    out[:, :, 0:3] = xyz
    return out


def affine_batch(points, affine, subset):
    """What the self-supervised step takes, from one pass: (cham [B,C,M], sub [B,C,len(subset)]) channels-first, cham the
    transformed batch and sub its columns `subset` (the same bits).  subset: int indices into [0, M) -- a numpy array or host
    tensor is checked here and travels with the matrices in ONE upload; a device tensor is used as it is."""
    affine = _check_affine_args(points, affine)
    if points.is_cuda:
        from . import ops
        _, cham, sub = ops.affine_points(ops.cf(points), affine, subset=subset, want_cf=True)
        return cham, sub
    cham = apply_affine(points, affine).transpose(2, 1).contiguous()
    idx = torch.as_tensor(subset, dtype=torch.int64)
    return cham, cham[:, :, idx].contiguous()


def _host_draws(batch_data):
    if not torch.is_tensor(batch_data):
        raise TypeError("expected a numpy array or a torch tensor, got %s" % type(batch_data).__name__)
    if batch_data.dim() != 3 or batch_data.shape[2] != 3:
        raise ValueError("expected a [B,N,3] batch (the reference reshapes every shape to (-1, 3)), got %s"
                         % (tuple(batch_data.shape),))
    return batch_data.shape[0]


def _uniform_angles(B, generator):
    """B angles uniform in [0, 2 pi): `uniform() * 2 * pi` per shape, float64 from the host generator."""
    return torch.rand(B, dtype=torch.float64, generator=generator).numpy() * 2 * np.pi


def rotate_point_cloud(batch_data, generator=None):
    """One random rotation about the up (y) axis per shape (provider.py:46-64).  [B,N,3] in, a NEW float32 batch out.
    torch: angle_b = rand_b * 2 pi, one float64 `torch.rand(B)` from `generator`."""
    return rotate_point_cloud_y(batch_data, generator=generator)


def rotate_point_cloud_z(batch_data, generator=None):
    """One random rotation about z per shape (provider.py:66-84); torch: the draw of rotate_point_cloud."""
    if _is_np(batch_data):
        return _rotate_np(batch_data, lambda k: _rot_z(np.random.uniform() * 2 * np.pi))
    B = _host_draws(batch_data)
    return apply_affine(batch_data, _affine_of(np.stack([_rot_z(a) for a in _uniform_angles(B, generator)])))


def rotate_point_cloud_y(batch_data, generator=None):
    """One random rotation about y per shape (provider.py:87-105): what `--rotation_z` of the pre-training script applies
    (pretrain_partseg_shapenet.py:331-333).  torch: the draw of rotate_point_cloud."""
    if _is_np(batch_data):
        return _rotate_np(batch_data, lambda k: _rot_y(np.random.uniform() * 2 * np.pi))
    B = _host_draws(batch_data)
    return apply_affine(batch_data, _affine_of(np.stack([_rot_y(a) for a in _uniform_angles(B, generator)])))


def rotate_point_cloud_y_pi4(batch_data, generator=None):
    """A random multiple n * pi / 4, n in 1..7, about y per shape (provider.py:108-126; `--rotation_z_45`,
    pretrain_partseg_shapenet.py:335-337).  torch: n = one `torch.randint(1, 8, (B,))` from `generator`."""
    if _is_np(batch_data):
        return _rotate_np(batch_data, lambda k: _rot_y(np.random.randint(1, 8) * np.pi / 4))
    B = _host_draws(batch_data)
    n = torch.randint(1, 8, (B,), generator=generator).numpy()
    return apply_affine(batch_data, _affine_of(np.stack([_rot_y(v * np.pi / 4) for v in n])))


def rotate_point_cloud_y_by_angle(batch_data, rotation_angle):
    """Every shape rotated about y by `rotation_angle` radians (provider.py:129-147).  No draw."""
    if _is_np(batch_data):
        return _rotate_np(batch_data, lambda k: _rot_y(rotation_angle))
    B = _host_draws(batch_data)
    return apply_affine(batch_data, _affine_of(np.stack([_rot_y(rotation_angle)] * B)))


def rotate_point_cloud_by_angle(batch_data, rotation_angle):
    """provider.py:197-214: as rotate_point_cloud_y_by_angle on the first three channels of a [B,N,3+] batch; further channels of
    the result are ZERO, as upstream leaves them."""
    if _is_np(batch_data):
        return _rotate_np(batch_data, lambda k: _rot_y(rotation_angle), xyz_only=True)
    if not torch.is_tensor(batch_data) or batch_data.dim() != 3 or batch_data.shape[2] < 3:
        raise ValueError("expected a [B,N,3+] batch")
    B = batch_data.shape[0]
    xyz = apply_affine(batch_data[:, :, 0:3].contiguous(), _affine_of(np.stack([_rot_y(rotation_angle)] * B)))
    if batch_data.shape[2] == 3:
        return xyz
    rotated = torch.zeros_like(batch_data)
    rotated[:, :, 0:3] = xyz
    return rotated


def rotate_perturbation_point_cloud(batch_data, angle_sigma=0.06, angle_clip=0.18, generator=None):
    """A small random rotation per shape: three angles clip(angle_sigma * randn(3), +-angle_clip), R = Rz . Ry . Rx
    (provider.py:240-262).  torch: one float64 `torch.randn(B, 3)` from `generator`."""
    if _is_np(batch_data):
        return _rotate_np(batch_data, lambda k: _rot_perturbation(np.clip(angle_sigma * np.random.randn(3), -angle_clip, angle_clip)))
    B = _host_draws(batch_data)
    angles = np.clip(angle_sigma * torch.randn(B, 3, dtype=torch.float64, generator=generator).numpy(), -angle_clip, angle_clip)
    return apply_affine(batch_data, _affine_of(np.stack([_rot_perturbation(a) for a in angles])))


def random_anisotropic_scale_point_cloud(batch_data, scale_low=0.8, scale_high=1.25, generator=None):
    """One scale per shape AND channel, uniform in [scale_low, scale_high] (provider.py:306-317).  In place, the same object out.
    torch ([B,N,3]): one float64 `uniform_(scale_low, scale_high)` draw of shape [B,3] from `generator`."""
    if _is_np(batch_data):
        B, N, C = batch_data.shape
        scales = np.random.uniform(scale_low, scale_high, [B, 1, C])
        np.multiply(batch_data, scales, out=batch_data, casting="same_kind")
        return batch_data
    B = _host_draws(batch_data)
    scales = torch.empty(B, 3, dtype=torch.float64).uniform_(scale_low, scale_high, generator=generator).numpy()
    if batch_data.is_cuda and not batch_data.is_contiguous():
        raise ValueError("random_anisotropic_scale_point_cloud works in place: a device batch must be contiguous [B,N,3] "
                         "(for an xyz slice of a wider batch use compose_affine(aniso=...) + apply_affine on the whole batch)")
    return apply_affine(batch_data, compose_affine(aniso=scales), out=batch_data)


# ---------------------------------------------------------------------------------------------------------------------------
# The per-point family and the xyz + normal rotations (provider.py:3-44, :150-194, :216-236, :320-327)
# ---------------------------------------------------------------------------------------------------------------------------
# numpy batches go the reference's way.  A torch tensor gets its per-shape parameters (angles, dropout ratios) and ONE 64-bit seed
# from `generator` on the host; the per-point random numbers are a pure function of (seed, shape, point): Philox4x32-10 with the
# seed as key and (point, shape, stream, 0) as counter, stream 0 = jitter, 1 = dropout (the contract of prifit_perturb_points in
# include/prifit_hip.h).  On the GPU ONE launch of that kernel does the work; a host tensor takes `_perturb_host`, the same
# arithmetic in torch -- the same dropped set and the same rotated bits, the jitter to the rounding of log / sqrt / cos / sin.

_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_STREAM_JITTER, _STREAM_DROPOUT = 0, 1


def _philox4x32_10(c0, c1, c2, c3, seed):
    """Philox4x32-10 on arrays of counters (32-bit values held in uint64), key = (seed & 2^32 - 1, seed >> 32) -> four uint64
    arrays of 32-bit words."""
    mask = np.uint64(0xffffffff)
    c = [np.asarray(v, dtype=np.uint64) & mask for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c[0], np.uint64(_PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + _PHILOX_W0) & 0xffffffff, (k1 + _PHILOX_W1) & 0xffffffff
    return c


def _philox_words(B, M, stream, seed):
    """The four words of every (shape, point): [4][B,M] uint64."""
    return _philox4x32_10(np.arange(M).reshape(1, M), np.arange(B).reshape(B, 1), stream, 0, seed)


def _unit24(w, plus_one=False):
    """(w >> 8 [+ 1]) * 2^-24 as a float32 tensor: exact."""
    v = (w >> np.uint64(8)).astype(np.int64) + int(plus_one)
    return torch.from_numpy(v.astype(np.float32)) * 2.0 ** -24


def _perturb_host(points, affine, rotate_normals, sigma, clip, ratios, seed, out):
    B, M, C = points.shape
    res = points.clone()
    if affine is not None:
        res[:, :, 0:3] = _affine_torch(points, affine)
        if rotate_normals:
            A = affine.to(dtype=points.dtype)[:, :9].reshape(B, 1, 3, 3)
            n0, n1, n2 = points[:, :, 3:4], points[:, :, 4:5], points[:, :, 5:6]
            res[:, :, 3:6] = (n0 * A[:, :, 0] + n1 * A[:, :, 1]) + n2 * A[:, :, 2]
    if sigma > 0:
        w = _philox_words(B, M, _STREAM_JITTER, seed)
        two_pi = torch.tensor(2 * np.pi, dtype=torch.float32)
        r01, th01 = torch.sqrt(-2.0 * torch.log(_unit24(w[0], True))), two_pi * _unit24(w[1])
        r2, th2 = torch.sqrt(-2.0 * torch.log(_unit24(w[2], True))), two_pi * _unit24(w[3])
        z = torch.stack([r01 * torch.cos(th01), r01 * torch.sin(th01), r2 * torch.cos(th2)], dim=2)
        s, c = torch.tensor(sigma, dtype=torch.float32), torch.tensor(clip, dtype=torch.float32)
        res[:, :, 0:3] += (s * z).clamp_(-c, c).to(points.dtype)
    if ratios is not None:
        u = _unit24(_philox_words(B, M, _STREAM_DROPOUT, seed)[0])
        drop = u <= torch.from_numpy(np.asarray(ratios, dtype=np.float32)).reshape(B, 1)
        res = torch.where(drop.unsqueeze(2), res[:, 0:1, :], res)
    if out is None:
        return res
    return out.copy_(res)


def _perturb(points, affine, rotate_normals, sigma, clip, ratios, seed, out):
    """Steps 1-4 of prifit_perturb_points on a [B,N,3 | 6] torch tensor; out=None: a new tensor, out=points: in place."""
    if not torch.is_tensor(points):
        raise TypeError("expected a numpy array or a torch tensor, got %s" % type(points).__name__)
    if points.dim() != 3 or points.shape[2] not in (3, 6):
        raise ValueError("expected a [B,N,3] or [B,N,6] batch, got shape %s" % (tuple(points.shape),))
    if rotate_normals and (points.shape[2] != 6 or affine is None):
        raise ValueError("rotate_normals needs a [B,N,6] batch (xyz, normal) and an affine map")
    if not sigma >= 0 or (sigma > 0 and not clip > 0):
        raise ValueError("jitter needs sigma >= 0 and clip > 0, got %r, %r" % (sigma, clip))
    if affine is not None:
        affine = _check_affine_args(points, affine)
    if ratios is not None:
        ratios = np.asarray(ratios, dtype=np.float32)
        if ratios.shape != (points.shape[0],):
            raise ValueError("expected one dropout ratio per shape, got shape %s" % (ratios.shape,))
    if points.is_cuda:
        from . import ops
        if out is not None and not points.is_contiguous():
            raise ValueError("in place on the device needs a contiguous float32 batch")
        return ops.perturb_points(points if points.is_contiguous() and points.dtype == torch.float32 else ops.cf(points), affine,
                                  rotate_normals=rotate_normals, sigma=sigma, clip=clip, drop_ratio=ratios, seed=seed, out=out)[0]
    return _perturb_host(points, affine, rotate_normals, float(sigma), float(clip), ratios, seed, out)


def _draw_seed(generator):
    """The key of the per-point generator: one 63-bit draw from the host generator."""
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, generator=generator))


def perturb_batch(batch, *, affine=None, rotate_normals=False, jitter=None, dropout=None, generator=None):
    """Several augmentations of a [B,N,3 | 6] torch batch in ONE launch (on the host: one pass of torch arithmetic), a NEW tensor out:
      affine          [B,12] float32 as `compose_affine` returns it, applied to xyz;
      rotate_normals  its 3x3 part applied to channels 3..5 too ([B,N,6] batches);
      jitter          (sigma, clip): xyz += clamp(sigma * z, -clip, clip), z standard normal per point and channel;
      dropout         max_dropout_ratio: per shape a ratio uniform in [0, max) -- one float64 `torch.rand(B)` from `generator` --
                      and every point dropped with that probability becomes the (transformed, jittered) first point of its shape.
    With jitter or dropout one more draw from `generator` follows, the 63-bit seed of the per-point random numbers."""
    sigma, clip = (0.0, 0.0) if jitter is None else (float(jitter[0]), float(jitter[1]))
    if jitter is not None and not (sigma >= 0 and clip > 0):
        raise ValueError("jitter=(sigma, clip) needs sigma >= 0 and clip > 0")
    if not torch.is_tensor(batch):
        raise TypeError("perturb_batch takes a torch tensor, got %s" % type(batch).__name__)
    ratios = None
    if dropout is not None:
        ratios = torch.rand(batch.shape[0], dtype=torch.float64, generator=generator).numpy() * dropout
    seed = _draw_seed(generator) if (sigma > 0 or ratios is not None) else 0
    return _perturb(batch, affine, rotate_normals, sigma, clip, ratios, seed, None)


def random_point_dropout(batch_pc, max_dropout_ratio=0.875, generator=None):
    """Per shape a dropout ratio uniform in [0, max_dropout_ratio); every point whose own uniform draw is <= it is overwritten
    with the shape's first point (provider.py:320-327).  In place, the same object out.  torch ([B,N,3 | 6]): the ratios are one
    float64 `torch.rand(B)` from `generator`, then one seed draw; the per-point draws are Philox words (see above)."""
    if _is_np(batch_pc):
        for b in range(batch_pc.shape[0]):
            dropout_ratio = np.random.random() * max_dropout_ratio
            drop_idx = np.where(np.random.random((batch_pc.shape[1])) <= dropout_ratio)[0]
            if len(drop_idx) > 0:
                batch_pc[b, drop_idx, :] = batch_pc[b, 0, :]
        return batch_pc
    if not torch.is_tensor(batch_pc):
        raise TypeError("expected a numpy array or a torch tensor, got %s" % type(batch_pc).__name__)
    ratios = torch.rand(batch_pc.shape[0], dtype=torch.float64, generator=generator).numpy() * max_dropout_ratio
    return _perturb(batch_pc, None, False, 0.0, 0.0, ratios, _draw_seed(generator), batch_pc)


def _rotate_with_normal_np(batch_data, matrix_of, out):
    """The reference's loop over shapes: xyz and normal of shape k times matrix_of(k), formed in double and rounded on assignment
    into `out` (the batch itself for the in-place function: its normals are read after its xyz were written, as upstream)."""
    for k in range(batch_data.shape[0]):
        R = matrix_of(k)
        shape_pc = batch_data[k, :, 0:3]
        shape_normal = batch_data[k, :, 3:6]
        out[k, :, 0:3] = np.dot(shape_pc.reshape((-1, 3)), R)
        out[k, :, 3:6] = np.dot(shape_normal.reshape((-1, 3)), R)
    return out


def _check_xyz_normal(batch_data):
    if not torch.is_tensor(batch_data):
        raise TypeError("expected a numpy array or a torch tensor, got %s" % type(batch_data).__name__)
    if batch_data.dim() != 3 or batch_data.shape[2] != 6:
        raise ValueError("expected a [B,N,6] batch (xyz, normal), got %s" % (tuple(batch_data.shape),))
    return batch_data.shape[0]


def rotate_point_cloud_with_normal(batch_xyz_normal, generator=None):
    """One random rotation about y per shape, points and normals alike (provider.py:150-168).  [B,N,6], IN PLACE, the same object
    out.  torch: the draw of rotate_point_cloud."""
    if _is_np(batch_xyz_normal):
        return _rotate_with_normal_np(batch_xyz_normal, lambda k: _rot_y(np.random.uniform() * 2 * np.pi), batch_xyz_normal)
    B = _check_xyz_normal(batch_xyz_normal)
    aff = _affine_of(np.stack([_rot_y(a) for a in _uniform_angles(B, generator)]))
    return _perturb(batch_xyz_normal, aff, True, 0.0, 0.0, None, 0, batch_xyz_normal)


def rotate_perturbation_point_cloud_with_normal(batch_data, angle_sigma=0.06, angle_clip=0.18, generator=None):
    """rotate_perturbation_point_cloud for a [B,N,6] batch, normals rotated too (provider.py:170-194); a NEW float32 batch.
    torch: the draw of rotate_perturbation_point_cloud."""
    if _is_np(batch_data):
        return _rotate_with_normal_np(
            batch_data, lambda k: _rot_perturbation(np.clip(angle_sigma * np.random.randn(3), -angle_clip, angle_clip)),
            np.zeros(batch_data.shape, dtype=np.float32))
    B = _check_xyz_normal(batch_data)
    angles = np.clip(angle_sigma * torch.randn(B, 3, dtype=torch.float64, generator=generator).numpy(), -angle_clip, angle_clip)
    return _perturb(batch_data, _affine_of(np.stack([_rot_perturbation(a) for a in angles])), True, 0.0, 0.0, None, 0, None)


def rotate_point_cloud_by_angle_with_normal(batch_data, rotation_angle):
    """Every shape of a [B,N,6] batch rotated about y by `rotation_angle` radians, normals too (provider.py:216-236); a NEW
    float32 batch.  No draw."""
    if _is_np(batch_data):
        return _rotate_with_normal_np(batch_data, lambda k: _rot_y(rotation_angle), np.zeros(batch_data.shape, dtype=np.float32))
    B = _check_xyz_normal(batch_data)
    return _perturb(batch_data, _affine_of(np.stack([_rot_y(rotation_angle)] * B)), True, 0.0, 0.0, None, 0, None)


def shuffle_points(batch_data, generator=None):
    """One random order of the points for the whole batch (provider.py:34-44; it changes what farthest-point sampling picks).
    torch: one `torch.randperm(N)` from `generator`, the gather on the tensor's device."""
    if _is_np(batch_data):
        idx = np.arange(batch_data.shape[1])
        np.random.shuffle(idx)
        return batch_data[:, idx, :]
    idx = torch.randperm(batch_data.shape[1], generator=generator)
    return batch_data[:, idx.to(batch_data.device), :]


def shuffle_data(data, labels, generator=None):
    """Shapes and labels in one random order -> (data, labels, the order) (provider.py:22-32).  torch: one
    `torch.randperm(len(labels))` from `generator`."""
    if _is_np(data):
        idx = np.arange(len(labels))
        np.random.shuffle(idx)
        return data[idx, ...], labels[idx], idx
    idx = torch.randperm(len(labels), generator=generator)
    return data[idx.to(data.device), ...], labels[idx.to(labels.device)], idx


def normalize_data(batch_data):
    """Every shape centred on its per-channel mean and divided by its largest row norm, all C channels alike (provider.py:3-19).
    numpy: a new float64 batch, as upstream; torch: a new tensor of the batch's dtype on its device."""
    if _is_np(batch_data):
        B, N, C = batch_data.shape
        normal_data = np.zeros((B, N, C))
        for b in range(B):
            pc = batch_data[b]
            centroid = np.mean(pc, axis=0)
            pc = pc - centroid
            m = np.max(np.sqrt(np.sum(pc ** 2, axis=1)))
            pc = pc / m
            normal_data[b] = pc
        return normal_data
    pc = batch_data - batch_data.mean(dim=1, keepdim=True)
    return pc / pc.pow(2).sum(dim=2).sqrt().amax(dim=1).reshape(-1, 1, 1)

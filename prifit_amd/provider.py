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

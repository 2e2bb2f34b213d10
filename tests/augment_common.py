"""Restatement of the per-shape affine augmentation, written from the formulas (not from the package, not from the reference):
the kernel's fixed-order fp32 expression, its float64 counterpart, the composition of the pre-training script's chain, and the
error bound the comparisons use.

Bound.  out_j = ((p0*A0j + p1*A1j) + p2*A2j) + t_j in fp32 against the same map in float64, u = 2**-24:
  - four roundings lie on the longest chain of the fixed-order expression (the product p0*A0j, then three sums); every term
    passes through at most four, each relative to a partial sum no larger than |p|.|A| + |t|: 4u,
  - rounding the composed A, t to fp32 once moves every term by at most u of its size: 1u,
  - the reference stores fp32 between its stages, a rounding relative to a partial result of the same size: 1u.
Together 6u * (|p|.|A| + |t|) elementwise, to first order in u; |p|.|A| = sum_i |p_i| |A_ij|."""
import os

import numpy as np

U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_provider.npz")

NAMES = ("rotate_point_cloud", "rotate_point_cloud_z", "rotate_point_cloud_y", "rotate_point_cloud_y_pi4",
         "rotate_point_cloud_y_by_angle", "rotate_point_cloud_by_angle", "rotate_perturbation_point_cloud",
         "random_anisotropic_scale_point_cloud")
# the reference's parameter lists (provider.py), in order
REF_PARAMS = {
    "rotate_point_cloud": ["batch_data"],
    "rotate_point_cloud_z": ["batch_data"],
    "rotate_point_cloud_y": ["batch_data"],
    "rotate_point_cloud_y_pi4": ["batch_data"],
    "rotate_point_cloud_y_by_angle": ["batch_data", "rotation_angle"],
    "rotate_point_cloud_by_angle": ["batch_data", "rotation_angle"],
    "rotate_perturbation_point_cloud": ["batch_data", "angle_sigma", "angle_clip"],
    "random_anisotropic_scale_point_cloud": ["batch_data", "scale_low", "scale_high"],
}
REF_DEFAULTS = {"angle_sigma": 0.06, "angle_clip": 0.18, "scale_low": 0.8, "scale_high": 1.25}


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


def rot_perturbation(ax, ay, az):
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(ax), -np.sin(ax)], [0.0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0.0, np.sin(ay)], [0.0, 1.0, 0.0], [-np.sin(ay), 0.0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0.0], [np.sin(az), np.cos(az), 0.0], [0.0, 0.0, 1.0]])
    return Rz @ Ry @ Rx


def affine_ref32(src, affine):
    """The kernel's expression in float32 numpy, one rounding per operation: src [B,M,C] float32, affine [B,12] float32 ->
    [B,M,C] float32 (channels >= 3 copied)."""
    src, affine = np.asarray(src, np.float32), np.asarray(affine, np.float32)
    B = src.shape[0]
    A, t = affine[:, :9].reshape(B, 1, 3, 3), affine[:, 9:].reshape(B, 1, 3)
    p0, p1, p2 = src[:, :, 0:1], src[:, :, 1:2], src[:, :, 2:3]
    out = src.copy()
    xyz = ((p0 * A[:, :, 0] + p1 * A[:, :, 1]) + p2 * A[:, :, 2]) + t
    assert xyz.dtype == np.float32
    out[:, :, 0:3] = xyz
    return out


def affine_ref64(xyz, A, t=None):
    """xyz [B,M,3] . A [B,3,3] + t [B,3] in float64."""
    out = np.einsum("bni,bij->bnj", np.asarray(xyz, np.float64), np.asarray(A, np.float64))
    return out if t is None else out + np.asarray(t, np.float64)[:, None, :]


def bound(xyz, A, t=None):
    """6u (|p|.|A| + |t|) elementwise, [B,M,3] (see the module docstring)."""
    b = np.einsum("bni,bij->bnj", np.abs(np.asarray(xyz, np.float64)), np.abs(np.asarray(A, np.float64)))
    if t is not None:
        b = b + np.abs(np.asarray(t, np.float64))[:, None, :]
    return 6 * U * b


def sequence_At(scale, shift, aniso=None, angle=None, angle2=None):
    """p -> ((p * s + t) * a) . Ry(angle) . Ry(angle2) as (A [B,3,3], t [B,3]) in float64."""
    B = len(scale)
    A = np.zeros((B, 3, 3))
    t = np.zeros((B, 3))
    for b in range(B):
        Ab, tb = np.eye(3) * scale[b], np.asarray(shift[b], np.float64)
        if aniso is not None:
            D = np.diag(np.asarray(aniso, np.float64).reshape(B, 3)[b])
            Ab, tb = Ab @ D, tb @ D
        for ang in (angle, angle2):
            if ang is not None:
                Ab, tb = Ab @ rot_y(ang[b]), tb @ rot_y(ang[b])
        A[b], t[b] = Ab, tb
    return A, t


def split_affine(affine):
    """[B,12] -> (A [B,3,3], t [B,3]) float64."""
    a = np.asarray(affine, np.float64)
    return a[:, :9].reshape(-1, 3, 3), a[:, 9:]

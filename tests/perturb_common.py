"""Restatement of the per-point augmentation kernel (csrc/perturb.hip, contract: prifit_perturb_points in include/prifit_hip.h),
written from the formulas of the header -- not from the package:

  - Philox4x32-10 in integer arithmetic, twice: `philox4x32_10` on numpy arrays (what the tests use) and `philox4x32_10_scalar`
    on Python integers, written separately (the round as a function of a tuple, the key schedule precomputed); both are pinned
    against the known-answer vectors of the Random123 distribution (kat_vectors: philox4x32 10) in tests/test_perturb_names.py;
  - the Box-Muller normals of the header in float64 (`normals64`) and in numpy float32, operation by operation (`normals32`);
  - the whole kernel (`perturb_ref`): the bit-exact parts in float32 numpy, one rounding per operation in the stated order, the
    jitter in float64.

The jitter bar.  The kernel evaluates clamp(sigma * z) in fp32 with the device's logf / sqrtf / cosf / sinf.  The yardstick is the
SAME formula evaluated in numpy float32 on the same words against float64: `jitter_yardstick(sigma, clip)` = the largest absolute
difference over the 3 x 4096 x 3 offsets of YARD_SEED.  The bar is 4 x that, the budget for other implementations of the four
functions.  Measured on the CPU (numpy 2, x86-64): sigma 0.01 / clip 0.05: yardstick 1.19e-08, bar 4.77e-08; sigma 1.0 / clip 0.05
(97 % of the offsets on the clamp, the rest within 0.05 of zero, where the rounding of the angle weighs most): yardstick 7.96e-07,
bar 3.18e-06.  The kernel on an MI355X, a zero source: 1.07e-08 and 4.21e-07 (tests/test_gpu_perturb.py prints them).
The final `xyz + offset` is ONE correctly rounded fp32 addition, so an output may be another ulp(out) / 2 away from
xyz + offset64: the comparisons add exactly that (`half_ulp`), nothing else."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "perturb_provider.npz")
STREAM_JITTER, STREAM_DROPOUT = 0, 1
SEED = 0x0123456789ABCDEF            # the seed of the kernel tests
YARD_SEED, YARD_SHAPE = 0x5EED5EED5EED, (3, 4096)
MID_RATIO = 0.4

NAMES = ("random_point_dropout", "rotate_point_cloud_with_normal", "rotate_perturbation_point_cloud_with_normal",
         "rotate_point_cloud_by_angle_with_normal", "shuffle_points", "shuffle_data", "normalize_data")
REF_PARAMS = {
    "random_point_dropout": ["batch_pc", "max_dropout_ratio"],
    "rotate_point_cloud_with_normal": ["batch_xyz_normal"],
    "rotate_perturbation_point_cloud_with_normal": ["batch_data", "angle_sigma", "angle_clip"],
    "rotate_point_cloud_by_angle_with_normal": ["batch_data", "rotation_angle"],
    "shuffle_points": ["batch_data"],
    "shuffle_data": ["data", "labels"],
    "normalize_data": ["batch_data"],
}
REF_DEFAULTS = {"max_dropout_ratio": 0.875, "angle_sigma": 0.06, "angle_clip": 0.18}

# Random123 known-answer vectors, philox4x32 with 10 rounds: (counter, key, result)
PHILOX_KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

M0, M1 = 0xD2511F53, 0xCD9E8D57      # the two multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85      # the Weyl increments of the key
MASK = np.uint64(0xffffffff)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Arrays of 32-bit counters (any integer dtype, broadcast together), one key -> [4] uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(v).astype(np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        lo0, hi0 = (np.uint64(M0) * c0) & MASK, (np.uint64(M0) * c0) >> np.uint64(32)
        lo1, hi1 = (np.uint64(M1) * c2) & MASK, (np.uint64(M1) * c2) >> np.uint64(32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) % 2 ** 32, (k1 + W1) % 2 ** 32
    return [v.astype(np.uint32) for v in (c0, c1, c2, c3)]


def _round_scalar(ctr, key):
    prod0, prod1 = M0 * ctr[0], M1 * ctr[2]
    return ((prod1 // 2 ** 32) ^ ctr[1] ^ key[0], prod1 % 2 ** 32, (prod0 // 2 ** 32) ^ ctr[3] ^ key[1], prod0 % 2 ** 32)


def philox4x32_10_scalar(ctr, key):
    """The second implementation: Python integers, the ten round keys laid out first."""
    keys = [((key[0] + r * W0) % 2 ** 32, (key[1] + r * W1) % 2 ** 32) for r in range(10)]
    ctr = tuple(int(v) for v in ctr)
    for rk in keys:
        ctr = _round_scalar(ctr, rk)
    return ctr


def words(B, M, stream, seed):
    """[4][B, M] uint32: the words of counter (point, shape, stream, 0) under key (seed low, seed high)."""
    return philox4x32_10(np.arange(M, dtype=np.uint64).reshape(1, M), np.arange(B, dtype=np.uint64).reshape(B, 1), stream, 0,
                         seed & 0xffffffff, (seed >> 32) & 0xffffffff)


def normals64(w):
    """[B, M, 3] float64 standard normals of the header's Box-Muller on the four word arrays."""
    u1 = lambda x: ((x >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = lambda x: (x >> 8).astype(np.float64) * 2.0 ** -24
    r01, th01 = np.sqrt(-2.0 * np.log(u1(w[0]))), 2.0 * np.pi * u2(w[1])
    r2, th2 = np.sqrt(-2.0 * np.log(u1(w[2]))), 2.0 * np.pi * u2(w[3])
    return np.stack([r01 * np.cos(th01), r01 * np.sin(th01), r2 * np.cos(th2)], axis=2)


def normals32(w):
    """The same in numpy float32, one rounding per operation, fp32(2 pi) as the header states it."""
    f = np.float32
    u1 = lambda x: ((x >> 8).astype(np.int64) + 1).astype(f) * f(2.0 ** -24)
    u2 = lambda x: (x >> 8).astype(f) * f(2.0 ** -24)
    two_pi = np.array([0x40C90FDB], dtype=np.uint32).view(f)[0]
    r01, th01 = np.sqrt(f(-2.0) * np.log(u1(w[0]))), two_pi * u2(w[1])
    r2, th2 = np.sqrt(f(-2.0) * np.log(u1(w[2]))), two_pi * u2(w[3])
    z = np.stack([r01 * np.cos(th01), r01 * np.sin(th01), r2 * np.cos(th2)], axis=2)
    assert z.dtype == f
    return z


def offsets64(w, sigma, clip):
    """clamp(sigma * z, -clip, clip) in float64, sigma and clip the fp32 values the kernel receives."""
    s, c = float(np.float32(sigma)), float(np.float32(clip))
    return np.clip(s * normals64(w), -c, c)


def offsets32(w, sigma, clip):
    s, c = np.float32(sigma), np.float32(clip)
    out = np.clip(s * normals32(w), -c, c)
    assert out.dtype == np.float32
    return out


_yard = {}


def jitter_yardstick(sigma, clip):
    """max |numpy-float32 offsets - float64 offsets| over the words of (YARD_SEED, YARD_SHAPE): see the module docstring."""
    key = (float(sigma), float(clip))
    if key not in _yard:
        w = words(YARD_SHAPE[0], YARD_SHAPE[1], STREAM_JITTER, YARD_SEED)
        _yard[key] = float(np.abs(offsets32(w, sigma, clip).astype(np.float64) - offsets64(w, sigma, clip)).max())
    return _yard[key]


def jitter_bar(sigma, clip):
    return 4.0 * jitter_yardstick(sigma, clip)


def half_ulp(x):
    """ulp(x) / 2 of float32 values, as float64: the rounding of one fp32 addition whose result is x."""
    x = np.abs(np.asarray(x, dtype=np.float32))
    return 0.5 * (np.nextafter(x, np.float32(np.inf)).astype(np.float64) - x.astype(np.float64))


def drop_mask(B, M, ratios, seed):
    """bool [B, M]: u <= ratio in float32 (exact: u has 24 bits), u from the first word of the dropout stream."""
    u = (words(B, M, STREAM_DROPOUT, seed)[0] >> 8).astype(np.float32) * np.float32(2.0 ** -24)
    return u <= np.asarray(ratios, dtype=np.float32).reshape(B, 1)


def exact32(src, affine, rotate_normals):
    """Steps 1-2 in float32 numpy, the stated order, one rounding per operation: [B, M, C] float32."""
    src = np.asarray(src, np.float32)
    out = src.copy()
    if affine is None:
        return out
    affine = np.asarray(affine, np.float32)
    B = src.shape[0]
    A, t = affine[:, :9].reshape(B, 1, 3, 3), affine[:, 9:].reshape(B, 1, 3)
    p0, p1, p2 = src[:, :, 0:1], src[:, :, 1:2], src[:, :, 2:3]
    out[:, :, 0:3] = ((p0 * A[:, :, 0] + p1 * A[:, :, 1]) + p2 * A[:, :, 2]) + t
    if rotate_normals:
        n0, n1, n2 = src[:, :, 3:4], src[:, :, 4:5], src[:, :, 5:6]
        out[:, :, 3:6] = (n0 * A[:, :, 0] + n1 * A[:, :, 1]) + n2 * A[:, :, 2]
    assert out.dtype == np.float32
    return out


def perturb_ref(src, affine=None, rotate_normals=False, sigma=0.0, clip=0.0, ratios=None, seed=0):
    """The whole kernel -> dict:
      base    [B, M, C] float32: steps 1-2, bit-exact;
      want    [B, M, C] float64: base + the float64 offsets on xyz (== base without jitter), BEFORE dropout;
      drop    bool [B, M] (all False without ratios);
      words   the jitter stream's four word arrays (the debug output: the kernel has none), or None."""
    B, M, _ = src.shape
    base = exact32(src, affine, rotate_normals)
    want = base.astype(np.float64)
    w = None
    if sigma > 0:
        w = words(B, M, STREAM_JITTER, seed)
        want[:, :, 0:3] += offsets64(w, sigma, clip)
    drop = drop_mask(B, M, ratios, seed) if ratios is not None else np.zeros((B, M), dtype=bool)
    return dict(base=base, want=want, drop=drop, words=w)


def check_output(got, ref, sigma, clip):
    """`got` [B, M, C] float32 (channels-last) against perturb_ref's dict.  Dropped points: the bits of point 0's row of `got`.
    The others: without jitter the bits of `base`; with jitter |got - base| <= clip + ulp/2 and |got - want| <= bar + ulp/2 on
    xyz, the bits of `base` on the normals.  -> the largest |got - want| over the kept xyz values (0 without jitter)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref["base"].shape
    drop, keep = ref["drop"], ~ref["drop"]
    B = got.shape[0]
    first = np.broadcast_to(got[:, 0:1, :], got.shape)
    assert np.array_equal(got[drop].view(np.int32), first[drop].view(np.int32)), "a dropped point is not point 0's output"
    if not sigma > 0:
        assert np.array_equal(got[keep].view(np.int32), ref["base"][keep].view(np.int32))
        return 0.0
    assert np.array_equal(got[keep][:, 3:].view(np.int32), ref["base"][keep][:, 3:].view(np.int32))
    g, base, want = got[keep][:, :3].astype(np.float64), ref["base"][keep][:, :3].astype(np.float64), ref["want"][keep][:, :3]
    slack = half_ulp(got[keep][:, :3])
    assert (np.abs(g - base) <= float(np.float32(clip)) + slack).all(), "an offset beyond the clip"
    err = np.abs(g - want)
    assert (err <= jitter_bar(sigma, clip) + slack).all(), "jitter: %.3e over the bar %.3e" % (float((err - slack).max()),
                                                                                             jitter_bar(sigma, clip))
    return float(err.max()) if err.size else 0.0

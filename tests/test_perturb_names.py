"""CPU: the rest of the reference's provider.py under its names -- numpy paths bit for bit against arrays the reference wrote
(tests/golden/perturb_provider.npz, recipe: tools/make_golden_perturb.py), the names and signatures after `compat.install()`, the
host-tensor paths against the restatement of the kernel (tests/perturb_common.py), the restatement's generator against the
published known-answer vectors, the C entry point in the header and the library, and the argument errors."""
import inspect

import numpy as np
import pytest
import torch

import perturb_common as PC
from prifit_amd import _lib

FN_SEED = 13


@pytest.fixture(scope="module")
def gold():
    return np.load(PC.GOLDEN, allow_pickle=False)


# ------------------------------------------------------------------------------------------------------------ the generator
def test_philox_known_answers():
    """Both implementations of tests/perturb_common.py give the Random123 known-answer vectors of philox4x32 with 10 rounds."""
    for ctr, key, want in PC.PHILOX_KAT:
        got = PC.philox4x32_10(*[np.array([c], dtype=np.uint32) for c in ctr], *key)
        assert tuple(int(v[0]) for v in got) == want
        assert PC.philox4x32_10_scalar(ctr, key) == want


def test_philox_implementations_agree():
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 2 ** 32, (4, 64), dtype=np.uint64)
    k0, k1 = (int(v) for v in rng.integers(0, 2 ** 32, 2, dtype=np.uint64))
    got = np.stack(PC.philox4x32_10(*ctr, k0, k1), axis=1)
    want = np.array([PC.philox4x32_10_scalar(tuple(int(v) for v in ctr[:, i]), (k0, k1)) for i in range(64)], dtype=np.uint32)
    assert np.array_equal(got, want)


def test_package_generator_is_the_restatements():
    from prifit_amd import provider
    for stream in (PC.STREAM_JITTER, PC.STREAM_DROPOUT):
        got = provider._philox_words(3, 257, stream, PC.SEED)
        want = PC.words(3, 257, stream, PC.SEED)
        assert all(np.array_equal(g.astype(np.uint32), w) for g, w in zip(got, want))


def test_middle_ratio_drops_some_and_keeps_some():
    """The dropout cases of tests/test_gpu_perturb.py cannot pass vacuously: at their seed, M = 257 and the middle ratio every
    shape drops between 10 % and 90 % of its points; ratio 1 drops all; ratio 0 drops only a point whose 24-bit draw is zero."""
    frac = PC.drop_mask(3, 257, [PC.MID_RATIO] * 3, PC.SEED).mean(axis=1)
    assert ((frac > 0.1) & (frac < 0.9)).all(), frac
    assert PC.drop_mask(3, 257, [1.0] * 3, PC.SEED).all()
    assert not PC.drop_mask(3, 257, [0.0] * 3, PC.SEED).any()


def test_yardstick_is_what_the_docstring_records():
    for sigma, clip, recorded in ((0.01, 0.05, 1.19e-08), (1.0, 0.05, 7.96e-07)):
        y = PC.jitter_yardstick(sigma, clip)
        print("yardstick sigma %g clip %g: %.3e, bar %.3e" % (sigma, clip, y, PC.jitter_bar(sigma, clip)))
        assert 0.5 * recorded <= y <= 2 * recorded          # the host's logf / cosf may differ in the last bit, not in size
    z = PC.normals64(PC.words(*PC.YARD_SHAPE, PC.STREAM_JITTER, PC.YARD_SEED))
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02 and (np.abs(PC.offsets64(PC.words(2, 9, 0, 5), 1.0, 0.05)) <= 0.05 + 1e-9).all()


# --------------------------------------------------------------------------------------------------------------- numpy paths
def _inputs(gold, name):
    if name == "random_point_dropout":
        return (gold["in3"].copy(),)
    if name == "rotate_point_cloud_by_angle_with_normal":
        return (gold["in6"].copy(), float(gold["angle"]))
    if name == "shuffle_data":
        return (gold["in6"].copy(), gold["labels"].copy())
    return (gold["in6"].copy(),)


@pytest.mark.parametrize("name", PC.NAMES)
def test_numpy_path_reproduces_reference_bits(gold, name):
    from prifit_amd import provider
    args = _inputs(gold, name)
    before = args[0].copy()
    np.random.seed(FN_SEED)
    got = getattr(provider, name)(*args)
    if name == "shuffle_data":
        for g, key in zip(got, ("data", "labels", "idx")):
            want = gold["fn_shuffle_data_" + key]
            assert g.dtype == want.dtype and np.array_equal(g, want)
        return
    want = gold["fn_" + name]
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    if name in ("random_point_dropout", "rotate_point_cloud_with_normal"):
        assert got is args[0]                                       # in place, the same object out
    else:
        assert got is not args[0] and np.array_equal(args[0], before)       # a new batch, the input untouched
    assert not np.array_equal(got, before)


def test_names_resolve_after_compat_install():
    import importlib
    import sys
    from prifit_amd import compat
    saved = dict(sys.modules)
    try:
        compat.install()
        provider = importlib.import_module("provider")
        for name in PC.NAMES:
            params = inspect.signature(getattr(provider, name)).parameters
            want = PC.REF_PARAMS[name]
            assert list(params)[:len(want)] == want, name
            for p in want:
                if p in PC.REF_DEFAULTS:
                    assert params[p].default == PC.REF_DEFAULTS[p], (name, p)
            for extra in list(params)[len(want):]:                 # what this package adds is keyword-with-default only
                assert params[extra].default is None, (name, extra)
        params = inspect.signature(provider.perturb_batch).parameters
        assert list(params) == ["batch", "affine", "rotate_normals", "jitter", "dropout", "generator"]
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in params.items() if n != "batch")
        assert callable(provider.jitter_point_cloud)
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)


# --------------------------------------------------------------------------------------------------------- host tensor paths
def _batch(B=3, N=70, C=6, seed=4):
    x = np.random.default_rng(seed).uniform(-1, 1, (B, N, C)).astype(np.float32)
    if C == 6:
        x[:, :, 3:] /= np.linalg.norm(x[:, :, 3:], axis=2, keepdims=True)
    return x


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _aff(mats):
    B = len(mats)
    return np.concatenate([np.stack(mats).reshape(B, 9), np.zeros((B, 3))], axis=1).astype(np.float32)


def test_host_rotations_with_normal_follow_their_documented_draws():
    from prifit_amd import provider
    x = _batch()
    B = x.shape[0]
    t = torch.from_numpy(x.copy())
    got = provider.rotate_point_cloud_with_normal(t, generator=torch.Generator().manual_seed(3))
    ang = torch.rand(B, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).numpy() * 2 * np.pi
    aff = _aff([_rot_y(a) for a in ang])
    want = PC.exact32(x, aff, True)
    assert got is t and np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    # the same map through perturb_batch: a new tensor, the same bits
    t2 = torch.from_numpy(x.copy())
    again = provider.perturb_batch(t2, affine=aff, rotate_normals=True)
    assert again is not t2 and torch.equal(t2, torch.from_numpy(x)) and torch.equal(again.view(torch.int32), got.view(torch.int32))
    # normals stay unit vectors, and without rotate_normals they are copied
    assert np.abs(np.linalg.norm(got.numpy()[:, :, 3:].astype(np.float64), axis=2) - 1).max() < 1e-6
    plain = provider.perturb_batch(t2, affine=aff)
    assert torch.equal(plain[:, :, 3:], t2[:, :, 3:]) and torch.equal(plain[:, :, :3], got[:, :, :3])

    by = provider.rotate_point_cloud_by_angle_with_normal(t2, 0.7)
    assert by is not t2 and np.array_equal(by.numpy().view(np.int32), PC.exact32(x, _aff([_rot_y(0.7)] * B), True).view(np.int32))

    pert = provider.rotate_perturbation_point_cloud_with_normal(t2, generator=torch.Generator().manual_seed(5))
    plain3 = provider.rotate_perturbation_point_cloud(t2[:, :, :3].contiguous(), generator=torch.Generator().manual_seed(5))
    assert pert is not t2 and torch.equal(pert[:, :, :3], plain3) and not torch.equal(pert[:, :, 3:], t2[:, :, 3:])


def test_host_dropout_and_jitter_follow_the_restatement():
    from prifit_amd import provider
    x = _batch(B=3, N=257)
    B = x.shape[0]
    g = torch.Generator().manual_seed(9)
    t = torch.from_numpy(x.copy())
    got = provider.random_point_dropout(t, generator=g)
    g = torch.Generator().manual_seed(9)
    ratios = torch.rand(B, dtype=torch.float64, generator=g).numpy() * 0.875
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, generator=g))
    ref = PC.perturb_ref(x, ratios=ratios, seed=seed)
    assert got is t and 0 < ref["drop"].sum() < ref["drop"].size
    PC.check_output(got.numpy(), ref, 0.0, 0.0)
    assert np.array_equal(got.numpy()[:, 0], x[:, 0])               # point 0 keeps its own values, dropped or not

    ang = np.array([0.3, 1.1, 2.0])
    aff = _aff([_rot_y(a) for a in ang])
    for sigma, clip in ((0.01, 0.05), (1.0, 0.05)):
        g = torch.Generator().manual_seed(11)
        out = provider.perturb_batch(torch.from_numpy(x), affine=aff, rotate_normals=True, jitter=(sigma, clip), dropout=0.6,
                                     generator=g)
        g = torch.Generator().manual_seed(11)
        ratios = torch.rand(B, dtype=torch.float64, generator=g).numpy() * 0.6
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, generator=g))
        ref = PC.perturb_ref(x, aff, True, sigma, clip, ratios, seed)
        worst = PC.check_output(out.numpy(), ref, sigma, clip)
        print("host perturb_batch sigma %g: worst |out - float64| %.3e, bar %.3e" % (sigma, worst, PC.jitter_bar(sigma, clip)))


def test_host_index_and_reduction_functions():
    from prifit_amd import provider
    x = _batch()
    t = torch.from_numpy(x)
    got = provider.shuffle_points(t, generator=torch.Generator().manual_seed(2))
    idx = torch.randperm(x.shape[1], generator=torch.Generator().manual_seed(2))
    assert torch.equal(got, t[:, idx, :]) and not torch.equal(got, t)
    labels = torch.tensor([4, 0, 9])
    d, l, i = provider.shuffle_data(t, labels, generator=torch.Generator().manual_seed(6))
    assert torch.equal(i, torch.randperm(3, generator=torch.Generator().manual_seed(6)))
    assert torch.equal(d, t[i]) and torch.equal(l, labels[i])
    n = provider.normalize_data(t)
    want = provider.normalize_data(x)                               # the reference's float64 loop
    assert n.dtype == torch.float32 and np.abs(n.numpy() - want).max() < 1e-6


# ------------------------------------------------------------------------------------------------------------- C entry point
def test_header_declares_perturb_points():
    sigs = _lib._signatures()
    assert "prifit_perturb_points" in _lib.declared_symbols()
    # src, B, M, C, affine, rotate_normals, sigma, clip, drop_ratio, seed_lo, seed_hi, dst_cl, dst_cf, stream
    assert len(sigs["prifit_perturb_points"]) == 14
    import ctypes
    assert sigs["prifit_perturb_points"][9:11] == [ctypes.c_uint, ctypes.c_uint]
    assert sigs["prifit_perturb_points"][6:8] == [ctypes.c_float, ctypes.c_float]


def test_library_exports_perturb_points(hiplib):
    assert hasattr(hiplib, "prifit_perturb_points")
    assert _lib.abi_version() >= 803


# ------------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    from prifit_amd import ops, provider
    x6, x3, x4 = torch.zeros(2, 5, 6), torch.zeros(2, 5, 3), torch.zeros(2, 5, 4)
    aff = np.zeros((2, 12), np.float32)
    for fn in (provider.rotate_point_cloud_with_normal, provider.rotate_perturbation_point_cloud_with_normal):
        with pytest.raises(ValueError):
            fn(x3)
        with pytest.raises(TypeError):
            fn([1, 2, 3])
    with pytest.raises(ValueError):
        provider.rotate_point_cloud_by_angle_with_normal(x4, 0.1)
    with pytest.raises(ValueError):
        provider.random_point_dropout(x4)
    with pytest.raises(ValueError):
        provider.perturb_batch(x3, affine=aff, rotate_normals=True)             # no normals to rotate
    with pytest.raises(ValueError):
        provider.perturb_batch(x6, rotate_normals=True)                         # no map to rotate them with
    with pytest.raises(ValueError):
        provider.perturb_batch(x6, affine=np.zeros((3, 12), np.float32))
    with pytest.raises(ValueError):
        provider.perturb_batch(x6, jitter=(0.01, 0.0))
    with pytest.raises(ValueError):
        provider.perturb_batch(x6, jitter=(-1.0, 0.05))
    with pytest.raises(TypeError):
        provider.perturb_batch(np.zeros((2, 5, 3), np.float32))
    # the binding checks shapes before it asks for a device
    with pytest.raises(ValueError):
        ops.perturb_points(x4)
    with pytest.raises(ValueError):
        ops.perturb_points(x6.double())
    with pytest.raises(ValueError):
        ops.perturb_points(x6.transpose(1, 2))
    with pytest.raises(ValueError):
        ops.perturb_points(x3, aff, rotate_normals=True)
    with pytest.raises(ValueError):
        ops.perturb_points(x6, np.zeros((2, 9), np.float32))
    with pytest.raises(ValueError):
        ops.perturb_points(x6, drop_ratio=np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        ops.perturb_points(x6, sigma=0.01, clip=0.0)
    with pytest.raises(ValueError):
        ops.perturb_points(x6, sigma=float("nan"), clip=0.05)
    with pytest.raises(ValueError):
        ops.perturb_points(x6, out=torch.zeros(2, 5, 3))
    with pytest.raises(RuntimeError):
        ops.perturb_points(x6)                                                  # a host tensor: there is no CPU kernel

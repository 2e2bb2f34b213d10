"""GPU: the per-point augmentation kernel (csrc/perturb.hip prifit_perturb_points) through the C ABI, every tensor in guard bands
(tests/guard_common.py: the source in NaN guards, the outputs in sentinel guards), against the restatement of
tests/perturb_common.py; then the provider functions on device tensors against their host-tensor paths.

Everything is compared bit for bit except the jitter offsets.  Their bar (perturb_common): 4 x the largest error of the same
Box-Muller formula evaluated in numpy float32 against float64 -- sigma 0.01 / clip 0.05: yardstick 1.19e-08, bar 4.77e-08;
sigma 1.0 / clip 0.05: yardstick 7.96e-07, bar 3.18e-06 -- plus ulp(out) / 2 for the one correctly rounded fp32 addition
`xyz + offset` where xyz is not zero."""
import functools

import numpy as np
import pytest
import torch

import guard_common as G
import perturb_common as PC

pytestmark = pytest.mark.gpu

EINVAL = -1
LEAD = TAIL = 2048           # floats of guard around every tensor (a stray tile would move 256 * 6 floats at most)
# one point; two; a wave less one, a wave, a wave and one; a tile and one (two tiles, and in place with dropout one workgroup
# that takes both).  With C = 3 and M odd every shape but the first starts off a 16-byte boundary: the scalar staging path.
SHAPES = [(B, M, C) for B in (1, 3) for M in (1, 2, 63, 64, 65, 257) for C in (3, 6)]
MODES = ("out", "inplace", "cf")
JITTERS = ((0.01, 0.05), (1.0, 0.05))


@functools.lru_cache(maxsize=None)
def _case(B, M, C):
    rng = np.random.default_rng(1000 * B + 10 * M + C)
    src = rng.uniform(-2, 2, (B, M, C)).astype(np.float32)
    aff = rng.uniform(-1.5, 1.5, (B, 12)).astype(np.float32)
    src.setflags(write=False), aff.setflags(write=False)
    return src, aff


def _launch(hiplib, src, mode, affine=None, rotate_normals=False, sigma=0.0, clip=0.0, ratios=None, seed=PC.SEED):
    """One call; -> the output as a channels-last [B, M, C] float32 numpy array.  Guards and (out of place) the source are checked."""
    B, M, C = src.shape
    bufs = G.Bufs(lead=LEAD, tail=TAIL)
    d_aff = None if affine is None else bufs.fin(torch.from_numpy(np.array(affine)))
    d_ratio = None if ratios is None else bufs.fin(torch.from_numpy(np.asarray(ratios, dtype=np.float32)))
    t_src = torch.from_numpy(np.array(src))              # (a copy: the cached case arrays are read-only)
    if mode == "inplace":
        d_src = bufs.fout((B, M, C), init=t_src)
        d_cl, d_cf = d_src, None
    else:
        d_src = bufs.fin(t_src)
        d_cl = bufs.fout((B, M, C)) if mode == "out" else None
        d_cf = bufs.fout((B, C, M)) if mode == "cf" else None
    p = lambda t: None if t is None else t.data_ptr()
    rc = hiplib.prifit_perturb_points(d_src.data_ptr(), B, M, C, p(d_aff), int(rotate_normals), float(sigma), float(clip),
                                      p(d_ratio), seed & 0xffffffff, seed >> 32, p(d_cl), p(d_cf),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    bufs.intact()
    if mode != "inplace":
        assert np.array_equal(d_src.cpu().numpy().view(np.int32), np.asarray(src).view(np.int32))       # only read
    out = d_cl.cpu().numpy() if d_cl is not None else np.ascontiguousarray(d_cf.cpu().numpy().transpose(0, 2, 1))
    return out


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


@pytest.mark.parametrize("B,M,C", SHAPES)
def test_affine_only_is_affine_points(hiplib, B, M, C):
    """Without jitter and dropout: the xyz bits of prifit_affine_points on the same inputs, further channels copied; with
    rotate_normals the normals are the stated expression in float32, bit for bit; without a map a bit copy."""
    from prifit_amd import ops
    src, aff = _case(B, M, C)
    want = ops.affine_points(torch.from_numpy(src.copy()).cuda(), torch.from_numpy(aff.copy()).cuda(), want_cl=True)[0].cpu().numpy()
    assert _bits_equal(want, PC.exact32(src, aff, False))
    for mode in MODES:
        assert _bits_equal(_launch(hiplib, src, mode, affine=aff), want), mode
        assert _bits_equal(_launch(hiplib, src, mode), src), mode
        if C == 6:
            got = _launch(hiplib, src, mode, affine=aff, rotate_normals=True)
            assert _bits_equal(got[:, :, :3], want[:, :, :3]) and _bits_equal(got, PC.exact32(src, aff, True)), mode
            assert not _bits_equal(got[:, :, 3:], src[:, :, 3:])


def _ratio_sets(B):
    sets = [[0.0] * B, [PC.MID_RATIO] * B, [1.0] * B]
    if B == 3:
        sets.append([1.0, 0.0, PC.MID_RATIO])
    return sets


@pytest.mark.parametrize("B,M,C", SHAPES)
def test_dropout(hiplib, B, M, C):
    """The dropped set is the restatement's, bit for bit (u <= ratio is an exact fp32 comparison); a dropped point holds point 0's
    output bits -- in place too, where the workgroup must have read point 0 before it wrote -- and the others the transformed
    bits.  Ratios 0, 1 and one in between (tests/test_perturb_names.py shows that it drops 10-90 % at M = 257)."""
    src, aff = _case(B, M, C)
    for ratios in _ratio_sets(B):
        ref = PC.perturb_ref(src, aff, C == 6, ratios=ratios, seed=PC.SEED)
        if M == 257 and PC.MID_RATIO in ratios:
            frac = ref["drop"][ratios.index(PC.MID_RATIO)].mean()
            assert 0.1 < frac < 0.9
        if 1.0 in ratios:
            assert ref["drop"][ratios.index(1.0)].all()                 # point 0 itself is dropped here
        for mode in MODES:
            got = _launch(hiplib, src, mode, affine=aff, rotate_normals=C == 6, ratios=ratios)
            PC.check_output(got, ref, 0.0, 0.0)
            assert _bits_equal(got[:, 0], ref["base"][:, 0]), mode      # point 0: its own output, dropped or not
    # with jitter: a dropped point carries point 0's JITTERED output
    sigma, clip = JITTERS[0]
    ratios = _ratio_sets(B)[-1]
    ref = PC.perturb_ref(src, aff, C == 6, sigma, clip, ratios, PC.SEED)
    for mode in MODES:
        PC.check_output(_launch(hiplib, src, mode, affine=aff, rotate_normals=C == 6, sigma=sigma, clip=clip, ratios=ratios), ref,
                        sigma, clip)


@pytest.mark.parametrize("sigma,clip", JITTERS)
@pytest.mark.parametrize("B,M,C", SHAPES)
def test_jitter(hiplib, B, M, C, sigma, clip):
    """The offsets are the clipped Box-Muller normals of the restatement's Philox words: within the clip, and within the jitter bar
    of the float64 evaluation (a wrong word would miss by the size of sigma or of the clip)."""
    src, aff = _case(B, M, C)
    ref = PC.perturb_ref(src, aff, False, sigma, clip, None, PC.SEED)
    worst = 0.0
    for mode in MODES:
        worst = max(worst, PC.check_output(_launch(hiplib, src, mode, affine=aff, sigma=sigma, clip=clip), ref, sigma, clip))
    # a zero source without a map: the output IS the offset -- no addition rounds, so the bar alone and the clip exactly
    zero = np.zeros((B, M, C), dtype=np.float32)
    got = _launch(hiplib, zero, "out", sigma=sigma, clip=clip)
    want = PC.offsets64(PC.words(B, M, PC.STREAM_JITTER, PC.SEED), sigma, clip)
    err = float(np.abs(got[:, :, :3].astype(np.float64) - want).max())
    print("jitter sigma %g clip %g [%d,%d,%d]: |offset - float64| %.3e (bar %.3e, yardstick %.3e); with a source %.3e; on the clamp %.0f %%"
          % (sigma, clip, B, M, C, err, PC.jitter_bar(sigma, clip), PC.jitter_yardstick(sigma, clip), worst,
             100.0 * float((np.abs(want) == np.float32(clip)).mean())))
    assert (np.abs(got[:, :, :3]) <= np.float32(clip)).all() and not got[:, :, 3:].any()
    assert err <= PC.jitter_bar(sigma, clip)
    if sigma == 1.0 and M >= 63:
        assert (np.abs(got[:, :, :3]) == np.float32(clip)).mean() > 0.5     # most values sit on the clamp


def test_same_seed_same_bits(hiplib):
    B, M, C = 3, 257, 6
    src, aff = _case(B, M, C)
    kw = dict(affine=aff, rotate_normals=True, sigma=0.01, clip=0.05, ratios=[0.2, 0.4, 0.6])
    a = _launch(hiplib, src, "out", **kw)
    for mode in MODES:                           # another launch, another layout, in place another launch geometry: the same bits
        assert _bits_equal(_launch(hiplib, src, mode, **kw), a), mode
    other = _launch(hiplib, src, "out", seed=PC.SEED + 1, **kw)
    assert not _bits_equal(other, a)
    assert (other[:, :, :3] != a[:, :, :3]).mean() > 0.9
    hi = _launch(hiplib, src, "out", seed=PC.SEED ^ (1 << 40), **kw)          # the high word of the seed is part of the key
    assert (hi[:, :, :3] != a[:, :, :3]).mean() > 0.9


def test_rejects_bad_arguments(hiplib):
    B, M, C = 2, 40, 6
    src = torch.zeros(B, M, C, device="cuda")
    aff = torch.zeros(B, 12, device="cuda")
    ratio = torch.zeros(B, device="cuda")
    cl, cl_base = G.guarded((B, M, C), LEAD, TAIL, poison=G.SENTINEL)
    cf, cf_base = G.guarded((B, C, M), LEAD, TAIL, poison=G.SENTINEL)
    st = torch.cuda.current_stream().cuda_stream
    s, a, r, o, f = src.data_ptr(), aff.data_ptr(), ratio.data_ptr(), cl.data_ptr(), cf.data_ptr()
    nan = float("nan")
    bad = {
        "src NULL": (None, B, M, C, a, 0, 0.0, 0.0, r, 1, 2, o, f, st),
        "B = 0": (s, 0, M, C, a, 0, 0.0, 0.0, r, 1, 2, o, f, st),
        "B < 0": (s, -1, M, C, a, 0, 0.0, 0.0, r, 1, 2, o, f, st),
        "B > 65535": (s, 65536, M, C, a, 0, 0.0, 0.0, r, 1, 2, o, f, st),
        "M = 0": (s, B, 0, C, a, 0, 0.0, 0.0, r, 1, 2, o, f, st),
        "C = 4": (s, B, M, 4, a, 0, 0.0, 0.0, r, 1, 2, o, f, st),
        "C = 2": (s, B, M, 2, a, 0, 0.0, 0.0, r, 1, 2, o, f, st),
        "no output": (s, B, M, C, a, 0, 0.0, 0.0, r, 1, 2, None, None, st),
        "dst_cf == src": (s, B, M, C, a, 0, 0.0, 0.0, r, 1, 2, o, s, st),
        "dst_cf == dst_cl": (s, B, M, C, a, 0, 0.0, 0.0, r, 1, 2, o, o, st),
        "rotate_normals with C = 3": (s, B, 2 * M, 3, a, 1, 0.0, 0.0, r, 1, 2, o, f, st),
        "rotate_normals without affine": (s, B, M, C, None, 1, 0.0, 0.0, r, 1, 2, o, f, st),
        "sigma < 0": (s, B, M, C, a, 0, -0.01, 0.05, r, 1, 2, o, f, st),
        "sigma NaN": (s, B, M, C, a, 0, nan, 0.05, r, 1, 2, o, f, st),
        "sigma > 0, clip = 0": (s, B, M, C, a, 0, 0.01, 0.0, r, 1, 2, o, f, st),
        "sigma > 0, clip NaN": (s, B, M, C, a, 0, 0.01, nan, r, 1, 2, o, f, st),
    }
    for what, args in bad.items():
        assert hiplib.prifit_perturb_points(*args) == EINVAL, what
    torch.cuda.synchronize()
    for base in (cl_base, cf_base):
        assert (base.view(torch.int32) == G.poison_bits(G.SENTINEL)).all()       # nothing was launched: sentinel everywhere


def test_binding(hiplib):
    """ops.perturb_points: host tables in one upload or device tables, `out` in place, want_cf alone -- the bits of the C call."""
    from prifit_amd import ops
    B, M, C = 3, 65, 6
    src, aff = _case(B, M, C)
    ratios = np.array([1.0, 0.0, PC.MID_RATIO], dtype=np.float32)
    kw = dict(rotate_normals=True, sigma=0.01, clip=0.05, seed=PC.SEED)
    want = _launch(hiplib, src, "out", affine=aff, ratios=ratios, **kw)
    d = torch.from_numpy(src.copy()).cuda()
    aff = aff.copy()
    cl, cf = ops.perturb_points(d, aff, drop_ratio=ratios, **kw)
    assert cf is None and cl is not d and _bits_equal(cl.cpu().numpy(), want) and _bits_equal(d.cpu().numpy(), src)
    cl, cf = ops.perturb_points(d, torch.from_numpy(aff.copy()).cuda(), drop_ratio=torch.from_numpy(ratios).cuda(), want_cf=True, **kw)
    assert cl is None and _bits_equal(cf.cpu().numpy().transpose(0, 2, 1), want)
    out = torch.empty_like(d)
    cl, cf = ops.perturb_points(d, aff, drop_ratio=torch.from_numpy(ratios), want_cf=True, out=out, **kw)
    assert cl is out and _bits_equal(out.cpu().numpy(), want) and _bits_equal(cf.cpu().numpy().transpose(0, 2, 1), want)
    cl, _ = ops.perturb_points(d, aff, drop_ratio=ratios, out=d, **kw)
    assert cl is d and _bits_equal(d.cpu().numpy(), want)


# --------------------------------------------------------------------------------------------------------------- the provider
def _xyz_normal(B=3, N=300, C=6, seed=8):
    x = np.random.default_rng(seed).uniform(-1, 1, (B, N, C)).astype(np.float32)
    if C == 6:
        x[:, :, 3:] /= np.linalg.norm(x[:, :, 3:], axis=2, keepdims=True)
    return x


@pytest.mark.parametrize("name", ["random_point_dropout", "rotate_point_cloud_with_normal", "rotate_perturbation_point_cloud_with_normal",
                                  "rotate_point_cloud_by_angle_with_normal", "shuffle_points", "shuffle_data"])
def test_provider_on_device_is_the_host_path(hiplib, name):
    """No jitter involved: a device tensor and a host tensor given equally seeded generators come out bit for bit equal, and the
    in-place / new-tensor convention is the numpy path's."""
    from prifit_amd import provider
    x = _xyz_normal()
    fn = getattr(provider, name)
    outs = []
    for dev in ("cuda", "cpu"):
        t = torch.from_numpy(x.copy()).to(dev)
        if name == "rotate_point_cloud_by_angle_with_normal":
            got = fn(t, 0.7)
        elif name == "shuffle_data":
            labels = torch.tensor([4, 0, 9], device=dev)
            got, lab, idx = fn(t, labels, generator=torch.Generator().manual_seed(33))
            assert got.device.type == dev and torch.equal(lab.cpu(), torch.tensor([4, 0, 9])[idx])
        else:
            got = fn(t, generator=torch.Generator().manual_seed(33))
        assert got.device.type == dev and got.dtype == torch.float32 and tuple(got.shape) == x.shape
        if name in ("random_point_dropout", "rotate_point_cloud_with_normal"):
            assert got is t
        else:
            assert got is not t and _bits_equal(t.cpu().numpy(), x)
        outs.append(got.cpu().numpy())
    assert _bits_equal(outs[0], outs[1])
    if name != "shuffle_data":                          # (an order of three shapes may be the identity)
        assert not _bits_equal(outs[0], x)


def test_provider_normalize_data_on_device(hiplib):
    from prifit_amd import provider
    x = _xyz_normal()
    got = provider.normalize_data(torch.from_numpy(x).cuda())
    want = provider.normalize_data(x)                   # the reference's float64 loop
    assert got.is_cuda and got.dtype == torch.float32
    # float32 against float64, every value at most 1 in magnitude after the division: at most 9 roundings of a tree sum of 300
    # terms and one of the mean's division, the difference, 3 for the row norm, the quotient: 15 * 2**-24, and the centroid's
    # error enters twice, through the point and through the largest norm -- 32 * 2**-24 covers the worst case of each
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print("normalize_data on device: %.3e (bound %.3e)" % (err, 32 * 2.0 ** -24))
    assert err <= 32 * 2.0 ** -24


def test_rotate_with_normal_is_perturb_batch(hiplib):
    """rotate_point_cloud_with_normal(x) == perturb_batch(x, that rotation, rotate_normals=True), bit for bit, on the device."""
    from prifit_amd import provider
    x = _xyz_normal()
    t = torch.from_numpy(x.copy()).cuda()
    got = provider.rotate_point_cloud_with_normal(t, generator=torch.Generator().manual_seed(3))
    ang = torch.rand(x.shape[0], dtype=torch.float64, generator=torch.Generator().manual_seed(3)).numpy() * 2 * np.pi
    aff = provider.compose_affine(y_angle=ang)
    src = torch.from_numpy(x).cuda()
    again = provider.perturb_batch(src, affine=aff, rotate_normals=True)
    assert got is t and again is not src and torch.equal(again.view(torch.int32), got.view(torch.int32))
    assert _bits_equal(got.cpu().numpy(), PC.exact32(x, aff, True))


@pytest.mark.parametrize("sigma,clip", JITTERS)
def test_perturb_batch_on_device_is_the_host_path(hiplib, sigma, clip):
    """Everything at once.  The dropped set and the normals bit for bit; the jittered xyz of the kept points within the jitter bar
    plus the two sides' one addition each (ulp / 2 each)."""
    from prifit_amd import provider
    x = _xyz_normal()
    aff = provider.compose_affine(y_angle=np.array([0.3, 1.1, 2.0]), scale=np.array([0.9, 1.0, 1.2]))
    outs = [provider.perturb_batch(torch.from_numpy(x).to(dev), affine=aff, rotate_normals=True, jitter=(sigma, clip), dropout=0.6,
                                   generator=torch.Generator().manual_seed(11)).cpu().numpy() for dev in ("cuda", "cpu")]
    g = torch.Generator().manual_seed(11)
    ratios = torch.rand(3, dtype=torch.float64, generator=g).numpy() * 0.6
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, generator=g))
    ref = PC.perturb_ref(x, aff, True, sigma, clip, ratios, seed)
    assert 0 < ref["drop"].sum() < ref["drop"].size
    for o in outs:
        PC.check_output(o, ref, sigma, clip)
    assert _bits_equal(outs[0][:, :, 3:], outs[1][:, :, 3:])
    diff = np.abs(outs[0][:, :, :3].astype(np.float64) - outs[1][:, :, :3].astype(np.float64))
    print("perturb_batch sigma %g: device against host %.3e (bar %.3e)" % (sigma, float(diff.max()), PC.jitter_bar(sigma, clip)))
    assert (diff <= PC.jitter_bar(sigma, clip) + PC.half_ulp(outs[0][:, :, :3]) + PC.half_ulp(outs[1][:, :, :3])).all()

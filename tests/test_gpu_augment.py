"""GPU: the one-launch batch affine (csrc/augment.hip prifit_affine_points) through the C ABI in guard bands, bit for bit against
the float32 restatement of its fixed-order expression (tests/augment_common.py); the provider functions on device tensors; the
trainer's flagged batch preparation, its default path against the parent implementation, and `selfsup_validate`."""
import numpy as np
import pytest
import torch

import augment_common as AC
import guard_common as G
from prifit_amd import synth
from tests_helpers import fit_inputs

pytestmark = pytest.mark.gpu

EINVAL = -1
LEAD = TAIL = 1024           # floats of sentinel around every output (a stray block would write 256 * C floats at most)

# (B, M, C, n_subset, misaligned src): one point; under one block; one block + 1 with C = 6 and more subset columns than points;
# several blocks with C = 4 (every block 16-byte aligned) and exactly one subset block; C = 3 with M odd (shape 1 starts 12 bytes
# off a 16-byte boundary) and the source one float into its buffer, so no block takes the float4 path
CASES = [(1, 1, 3, 1, False), (3, 255, 3, 7, False), (2, 257, 6, 300, False), (2, 700, 4, 256, False), (2, 513, 3, 64, True)]


def _inputs(B, M, C, n_sub, misaligned, seed=0):
    rng = np.random.default_rng(seed + 17 * M + C)
    src = rng.uniform(-2, 2, (B, M, C)).astype(np.float32)
    aff = rng.uniform(-1.5, 1.5, (B, 12)).astype(np.float32)
    subset = rng.integers(0, M, n_sub).astype(np.int32)          # with replacement: repeated indices whenever n_sub > 1
    if n_sub > 1:
        subset[-1] = subset[0]
    want_cl = AC.affine_ref32(src, aff)
    want_cf = np.ascontiguousarray(want_cl.transpose(0, 2, 1))
    want_sub = np.ascontiguousarray(want_cf[:, :, subset])
    base = torch.full((B * M * C + 8,), float("nan"), device="cuda")
    off = 1 if misaligned else 0
    assert base.data_ptr() % 16 == 0
    d_src = base[off:off + B * M * C].view(B, M, C)
    d_src.copy_(torch.from_numpy(src))
    return dict(src=src, aff=aff, subset=subset, want=dict(cl=want_cl, cf=want_cf, sub=want_sub), d_src=d_src, base=base,
                d_aff=torch.from_numpy(aff).cuda(), d_subset=torch.from_numpy(subset).cuda())


def _out(shape):
    view, base = G.guarded(shape, LEAD, TAIL, poison=G.SENTINEL)
    return view, base


def _run(hiplib, d, which, B, M, C, n_sub, src=None):
    """One call with the outputs named in `which`; -> {name: (view, base)}."""
    shapes = dict(cl=(B, M, C), cf=(B, C, M), sub=(B, C, n_sub))
    outs = {k: _out(shapes[k]) for k in which}
    p = lambda k: outs[k][0].data_ptr() if k in outs else None
    src = d["d_src"] if src is None else src
    rc = hiplib.prifit_affine_points(src.data_ptr(), B, M, C, d["d_aff"].data_ptr(), d["d_subset"].data_ptr(), n_sub,
                                     p("cl"), p("cf"), p("sub"), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return outs


def _check(outs, want):
    for k, (view, base) in outs.items():
        assert np.array_equal(view.cpu().numpy().view(np.int32), want[k].view(np.int32)), k     # bits, NaN-safe
        G.assert_guards_intact(base, view)


@pytest.mark.parametrize("B,M,C,n_sub,misaligned", CASES)
def test_affine_points_bits(hiplib, B, M, C, n_sub, misaligned):
    d = _inputs(B, M, C, n_sub, misaligned)
    assert (d["d_src"].data_ptr() % 16 != 0) == misaligned
    for which in (("cl", "cf", "sub"), ("cl",), ("cf",), ("sub",)):
        _check(_run(hiplib, d, which, B, M, C, n_sub), d["want"])
    if C > 3:                                                            # channels >= 3: bit copies of the source
        cf = _run(hiplib, d, ("cf",), B, M, C, n_sub)["cf"][0].cpu().numpy()
        assert np.array_equal(cf[:, 3:, :].view(np.int32), d["src"].transpose(0, 2, 1)[:, 3:, :].view(np.int32))
    # the source was only read
    assert np.array_equal(d["d_src"].cpu().numpy(), d["src"]) and torch.isnan(d["base"][B * M * C + 1:]).all()
    # in place (dst_cl == src), with the other two outputs taken from the untouched source in the same call
    src_view, src_base = G.guarded((B, M, C), LEAD, TAIL, poison=G.SENTINEL)
    src_view.copy_(torch.from_numpy(d["src"]))
    outs = {k: _out(s) for k, s in dict(cf=(B, C, M), sub=(B, C, n_sub)).items()}
    rc = hiplib.prifit_affine_points(src_view.data_ptr(), B, M, C, d["d_aff"].data_ptr(), d["d_subset"].data_ptr(), n_sub,
                                     src_view.data_ptr(), outs["cf"][0].data_ptr(), outs["sub"][0].data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    outs["cl"] = (src_view, src_base)
    _check(outs, d["want"])


def test_affine_points_repeatable(hiplib):
    B, M, C, n_sub = 2, 700, 4, 256
    d = _inputs(B, M, C, n_sub, False, seed=1)
    a = _run(hiplib, d, ("cl", "cf", "sub"), B, M, C, n_sub)
    b = _run(hiplib, d, ("cl", "cf", "sub"), B, M, C, n_sub)
    for k in a:
        assert torch.equal(a[k][0].view(torch.int32), b[k][0].view(torch.int32))


def test_affine_points_rejects_bad_arguments(hiplib):
    B, M, C, n_sub = 2, 40, 3, 8
    d = _inputs(B, M, C, n_sub, False)
    outs = {k: _out(s) for k, s in dict(cl=(B, M, C), cf=(B, C, M), sub=(B, C, n_sub)).items()}
    st = torch.cuda.current_stream().cuda_stream
    src, aff, sub = d["d_src"].data_ptr(), d["d_aff"].data_ptr(), d["d_subset"].data_ptr()
    cl, cfp, sb = (outs[k][0].data_ptr() for k in ("cl", "cf", "sub"))
    bad = {
        "B = 0": (src, 0, M, C, aff, sub, n_sub, cl, cfp, sb, st),
        "B < 0": (src, -1, M, C, aff, sub, n_sub, cl, cfp, sb, st),
        "M = 0": (src, B, 0, C, aff, sub, n_sub, cl, cfp, sb, st),
        "C = 2": (src, B, M, 2, aff, sub, n_sub, cl, cfp, sb, st),
        "C = 9": (src, B, M, 9, aff, sub, n_sub, cl, cfp, sb, st),
        "no output": (src, B, M, C, aff, sub, n_sub, None, None, None, st),
        "dst_sub without subset": (src, B, M, C, aff, None, n_sub, cl, cfp, sb, st),
        "dst_sub with n_subset = 0": (src, B, M, C, aff, sub, 0, cl, cfp, sb, st),
        "dst_cf == src": (src, B, M, C, aff, sub, n_sub, cl, src, sb, st),
    }
    for what, args in bad.items():
        assert hiplib.prifit_affine_points(*args) == EINVAL, what
    torch.cuda.synchronize()
    for view, base in outs.values():
        assert (base.view(torch.int32) == G.poison_bits(G.SENTINEL)).all()       # nothing was launched: sentinel everywhere
    assert np.array_equal(d["d_src"].cpu().numpy(), d["src"])


def test_wrapper_checks_host_subset(hiplib):
    from prifit_amd import ops
    src = torch.zeros(1, 10, 3, device="cuda")
    aff = np.zeros((1, 12), np.float32)
    with pytest.raises(IndexError):
        ops.affine_points(src, aff, subset=np.array([0, 10]), want_cf=True)
    with pytest.raises(IndexError):
        ops.affine_points(src, aff, subset=np.array([-1]), want_cf=True)


@pytest.mark.parametrize("name", AC.NAMES)
def test_provider_on_device(hiplib, name):
    """Device tensor path: parameters from a seeded CPU generator, re-drawn here by the documented law after re-seeding, applied
    in float64; bound 6 * 2**-24 * (|p|.|A| + |t|) (augment_common: four roundings of the expression, one of A and t, one spare
    for the reference's fp32 stages, which this path does not have)."""
    from prifit_amd import provider
    B, N = 3, 300
    x = np.random.default_rng(8).uniform(-1, 1, (B, N, 3)).astype(np.float32)
    t = torch.from_numpy(x).cuda()
    g = torch.Generator().manual_seed(33)
    if name.endswith("by_angle"):
        got = getattr(provider, name)(t, 0.7)
        A = np.stack([AC.rot_y(0.7)] * B)
    else:
        got = getattr(provider, name)(t, generator=g)
        g = torch.Generator().manual_seed(33)
        if name == "random_anisotropic_scale_point_cloud":
            A = np.stack([np.diag(v) for v in torch.empty(B, 3, dtype=torch.float64).uniform_(0.8, 1.25, generator=g).numpy()])
        elif name == "rotate_perturbation_point_cloud":
            ang = np.clip(0.06 * torch.randn(B, 3, dtype=torch.float64, generator=g).numpy(), -0.18, 0.18)
            A = np.stack([AC.rot_perturbation(*v) for v in ang])
        elif name == "rotate_point_cloud_y_pi4":
            A = np.stack([AC.rot_y(int(n) * np.pi / 4) for n in torch.randint(1, 8, (B,), generator=g)])
        else:
            ang = torch.rand(B, dtype=torch.float64, generator=g).numpy() * 2 * np.pi
            A = np.stack([(AC.rot_z if name.endswith("_z") else AC.rot_y)(v) for v in ang])
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (B, N, 3)
    if name == "random_anisotropic_scale_point_cloud":
        assert got is t                                                     # in place, as the numpy path
    else:
        assert got is not t and np.array_equal(t.cpu().numpy(), x)          # a new batch
    err = np.abs(got.cpu().numpy().astype(np.float64) - AC.affine_ref64(x, A))
    lim = AC.bound(x, A)
    print("%s on device: worst error / bound = %.3f" % (name, float((err / lim).max())))
    assert (err <= lim).all()


# ----------------------------------------------------------------------------------------------------------------- trainer
B_T, N_T, M_T = 2, 1024, 2500      # the smallest self-supervised step shape of tests/test_gpu_train_step.py
STEP_KW = dict(npoint=N_T, quantile=0.05, msc_iterations=5, max_num_clusters=25)


@pytest.fixture(scope="module")
def cham_batches():
    return [fit_inputs(B_T, N_T, 128, seed, M=M_T)[1] for seed in (8, 9)]


@pytest.fixture(scope="module")
def trainer(hiplib):
    from prifit_amd.models import pointnet2_part_seg_msg as MSG
    from prifit_amd.train_step import Trainer
    torch.manual_seed(4)
    net = MSG.get_model(50)
    synth.xavier_like_trainer(net)
    return Trainer(net.cuda(), lmbda=1.0)


def test_prefetch_with_flags_follows_the_scripts_draws(trainer, cham_batches):
    x = cham_batches[0].cpu().numpy()
    np.random.seed(3)
    trainer.prefetch_selfsup(cham_batches[0].cuda(), npoint=N_T, rotation_z=True, rotation_z_45=True, random_anisotropic_scale=True)
    nxt, trainer._next = trainer._next, None
    trainer.model.after_backbone = None
    np.random.seed(3)
    scale, shift = np.random.uniform(0.8, 1.25, B_T), np.random.uniform(-0.1, 0.1, (B_T, 3))
    aniso = np.random.uniform(0.8, 1.25, [B_T, 1, 3])
    a1 = [np.random.uniform() * 2 * np.pi for _ in range(B_T)]
    a2 = [np.random.randint(1, 8) * np.pi / 4 for _ in range(B_T)]
    subset = np.random.choice(M_T, N_T, replace=False)
    A, t = AC.sequence_At(scale, shift, aniso, a1, a2)
    cham, points = nxt["cham"], nxt["points"]
    assert tuple(cham.shape) == (B_T, 3, M_T) and tuple(points.shape) == (B_T, 3, N_T) and cham.is_contiguous() and points.is_contiguous()
    err = np.abs(cham.cpu().numpy().transpose(0, 2, 1).astype(np.float64) - AC.affine_ref64(x, A, t))
    lim = AC.bound(x, A, t)
    print("prefetch_selfsup(flags): worst error / bound = %.3f" % float((err / lim).max()))
    assert (err <= lim).all()
    assert torch.equal(points.view(torch.int32), cham[:, :, torch.from_numpy(subset).cuda()].view(torch.int32))


def _parent_selfsup_batch(chamfer_points, npoint, augment, subset):
    """`Trainer._selfsup_batch` and `random_scale_shift` as they stood before the augmentation flags."""
    B, M, _ = chamfer_points.shape
    if augment:
        dev = chamfer_points.device
        scales = torch.empty(B, 1, 1, device=dev).uniform_(0.8, 1.25, generator=None)
        shifts = torch.empty(B, 1, 3, device=dev).uniform_(-0.1, 0.1, generator=None)
        out = chamfer_points.clone()
        out[:, :, 0:3] = out[:, :, 0:3] * scales + shifts
        chamfer_points = out
    cham = chamfer_points.transpose(2, 1).contiguous()
    if subset is None:
        subset = torch.from_numpy(np.random.choice(M, npoint, replace=False)).to(cham.device)
    return cham, cham[:, :, subset].contiguous()


def test_default_batch_path_is_the_parents(trainer, cham_batches):
    c = cham_batches[0].cuda()
    for augment in (True, False):
        torch.manual_seed(11), np.random.seed(12)
        want = _parent_selfsup_batch(c, N_T, augment, None)
        torch.manual_seed(11), np.random.seed(12)
        got = trainer._selfsup_batch(c, N_T, augment, None)
        state = np.random.get_state()[1].copy()
        for a, b in zip(got, want):
            assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
        np.random.seed(12)
        np.random.choice(M_T, N_T, replace=False)
        assert np.array_equal(state, np.random.get_state()[1])              # one choice() and nothing else was drawn


def test_selfsup_validate(trainer, cham_batches):
    """The mean of the per-batch losses of direct eval-mode / no_grad model calls with the same subset, sampling starts and
    device random stream.  Bar: 1e-4 relative, what tests/test_gpu_train_step.py asks of two runs of the same forward (the fit
    path sums with float atomics, so two runs differ in the last bits).  Nothing of the model's state moves."""
    net = trainer.model
    subset = torch.from_numpy(np.random.default_rng(3).choice(M_T, N_T, replace=False)).cuda()
    starts = (torch.from_numpy(synth.fps_start(B_T, N_T, 5)).cuda(), torch.from_numpy(synth.fps_start(B_T, 512, 6)).cuda())
    kw = dict(quantile=0.05, msc_iterations=5, max_num_clusters=25, fps_start=starts)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    assert any(k.endswith("num_batches_tracked") for k in before) and any(k.endswith("running_mean") for k in before)
    beta = net.beta
    want = []
    net.eval()
    torch.manual_seed(12)
    with torch.no_grad():
        for c in cham_batches:
            cham = c.cuda().transpose(2, 1).contiguous()
            out = net(cham[:, :, subset].contiguous(), torch.zeros(B_T, 1, 16, device="cuda"), chamfer_points=cham,
                      include_convex_loss=True, **kw)
            want.append(float(torch.mean(out[3])))
    for mode in (True, False):
        net.train(mode)
        net.beta = beta
        torch.manual_seed(12)
        got = trainer.selfsup_validate([c.cuda() for c in cham_batches], npoint=N_T, subset=subset, **kw)
        assert isinstance(got, float) and net.training is mode
        print("selfsup_validate %.9g, direct %.9g %.9g" % (got, want[0], want[1]))
        assert got == pytest.approx((want[0] + want[1]) / 2, rel=1e-4, abs=0)
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k
    net.train()


def test_selfsup_step_with_flags_trains(trainer, cham_batches):
    net = trainer.model
    w0 = net.extra_conv_emb.weight.detach().clone()
    np.random.seed(5)
    ss = trainer.selfsup_step(cham_batches[1].cuda(), rotation_z=True, random_anisotropic_scale=True, **STEP_KW)
    assert torch.isfinite(ss) and not torch.equal(net.extra_conv_emb.weight.detach(), w0)

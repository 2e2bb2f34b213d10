"""The chart-batched AtlasNet decoder (csrc/atlas.hip, models/reconstruction.py) and reconstruct=True of the part-seg net.

Tolerance, per tensor: the restatement of tests/atlas_common.py evaluated in fp32 on the CPU differs from its fp64 evaluation
by some maximum error e32; the kernels get 4 * e32 against the same fp64 values.  Both are fp32 evaluations of one fp64
quantity that differ in summation order only, and the maximum runs over thousands of elements.  Every test prints e32, the
kernels' error and their ratio for every tensor (largest ratios: DESIGN.md 3.5).  The comparison presumes that fp32 and fp64
pick the same nearest neighbours, which is asserted on the restatement."""
import numpy as np
import pytest
import torch

import atlas_common as ac
from guard_common import SENTINEL, assert_guards_intact, guarded

pytestmark = pytest.mark.gpu

# (B, num_charts, num_points, seed, training, constant columns)
CASES = {
    "2x3x128": (2, 3, 128, 11, True, False),
    "3x2x9": (3, 2, 9, 12, True, False),
    "5x25x128": (5, 25, 128, 13, True, False),
    "1x1x16": (1, 1, 16, 14, True, False),
    "eval": (2, 3, 128, 11, False, False),
    "constant": (2, 2, 128, 15, True, True),
}
_ref = {}


def reference(name):
    """fp64 and fp32 restatement of a case, computed once"""
    if name not in _ref:
        B, C, npts, seed, training, const = CASES[name]
        sd = ac.make_state(seed, C, constant_columns=const)
        z, target = ac.make_inputs(seed, B)
        r64 = ac.evaluate(sd, z, target, npts, C, torch.float64, training)
        r32 = ac.evaluate(sd, z, target, npts, C, torch.float32, training)
        _ref[name] = (sd, z, target, r64, r32)
    return _ref[name]


def build(sd, C, npts, training):
    from prifit_amd.models.reconstruction import AtlasNet
    net = AtlasNet(num_charts=C, num_points=npts)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    net = net.cuda()
    return net.train() if training else net.eval()


def run(name):
    """the module on the GPU -> dict shaped like atlas_common.evaluate's"""
    from prifit_amd.models.reconstruction import ChamferDistance
    B, C, npts, seed, training, const = CASES[name]
    sd, z, target = reference(name)[:3]
    net = build(sd, C, npts, training)
    zt = torch.from_numpy(z).cuda().requires_grad_(True)
    out = net(zt)
    loss = ChamferDistance()(out, torch.from_numpy(target).cuda())
    loss.backward()
    res = {"out": out.detach().cpu().numpy(), "loss": loss.detach().cpu().numpy(), "gz": zt.grad.cpu().numpy()}
    for k, p in net.named_parameters():
        res["g:" + k] = p.grad.cpu().numpy()
    for k, b in net.named_buffers():
        res[k] = b.cpu().numpy()
    return res


def check(tag, got, r64, r32, keys):
    """prints every tensor's figures first, then asserts"""
    rows = []
    for k in keys:
        e32 = float(np.abs(r32[k].astype(np.float64) - r64[k]).max())
        e = float(np.abs(got[k].astype(np.float64).reshape(r64[k].shape) - r64[k]).max())
        ratio = e / e32 if e32 > 0 else (0.0 if e == 0 else float("inf"))
        print("%-10s %-34s e32 %.3e  kernel %.3e  ratio %.2f" % (tag, k, e32, e, ratio))
        rows.append((k, e32, e))
    for k, e32, e in rows:
        assert np.isfinite(got[k]).all(), k
        assert e <= 4.0 * e32, "%s %s: kernel error %.3e above 4 x %.3e" % (tag, k, e, e32)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_neighbours_agree(name):
    _, _, _, r64, r32 = reference(name)
    assert np.array_equal(r64["idx_ot"], r32["idx_ot"]) and np.array_equal(r64["idx_to"], r32["idx_to"])


@pytest.mark.parametrize("name", list(CASES))
def test_against_restatement(hiplib, name):
    B, C, npts, seed, training, const = CASES[name]
    sd, z, target, r64, r32 = reference(name)
    got = run(name)
    keys = ["out", "loss", "gz"] + [k for k in r64 if k.startswith("g:")] + [k for k in r64 if "running" in k]
    check(name, got, r64, r32, keys)
    for i in range(C):
        for l in (1, 2, 3):
            k = "decoder.%d.bn%d.num_batches_tracked" % (i, l)
            assert int(got[k]) == int(sd[k]) + (1 if training else 0), k
    if not training:
        for k in sd:
            if "running" in k:
                assert np.array_equal(got[k], sd[k]), k


def test_golden_reference_values(hiplib, golden):
    """the recorded reference outputs themselves (not only through the restatement) at the two recorded shapes"""
    G = golden("atlas_decoder")
    for name in ("2x3x128", "3x2x9"):
        B, C, npts = CASES[name][:3]
        _, _, _, r64, r32 = reference(name)
        got = run(name)
        tag = "%d_%d_%d|" % (B, C, npts)
        ref = {"out": G[tag + "out"], "loss": G[tag + "loss"], "gz": G[tag + "gz"]}
        for k in ref:
            e32 = float(np.abs(r32[k].astype(np.float64) - ref[k]).max())
            e = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
            print("%-10s %-6s e32 %.3e kernel %.3e" % (name, k, e32, e))
            assert e <= 4.0 * e32, (name, k, e, e32)


def test_same_bits_from_two_runs(hiplib):
    a, b = run("5x25x128"), run("5x25x128")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def _direct(L, name):
    """the entry points called directly on guarded buffers -> (views, bases)"""
    B, C, npts, seed, training, const = CASES[name]
    sd, z, target = reference(name)[:3]
    net = build(sd, C, npts, training)
    P = net.grid_size ** 2
    table, grid = net._table(torch.device("cuda", torch.cuda.current_device())), net._grid(torch.device("cuda", torch.cuda.current_device()))
    nf, nb = L.query("prifit_atlas_workspace_floats", C, B, P, 0), L.query("prifit_atlas_workspace_floats", C, B, P, 1)
    out, out_b = guarded((B, C * P, 3), 4096, 4096, SENTINEL)
    ws, ws_b = guarded((nf,), 4096, 4096, SENTINEL)
    sc, sc_b = guarded((nb,), 4096, 4096, SENTINEL)
    gz, gz_b = guarded((B, 128), 4096, 4096, SENTINEL)
    gp, gp_b = guarded((C, 28210), 4096, 4096, SENTINEL)
    zt = torch.from_numpy(z).cuda()
    L.call("prifit_atlas_fwd", L.ptr(table), L.ptr(zt), L.ptr(grid), C, B, P, int(training), 1e-5, 0.1, L.ptr(out), L.ptr(ws), L.cur_stream())
    gout = torch.from_numpy(np.random.default_rng(seed).standard_normal((B, C * P, 3)).astype(np.float32)).cuda()
    L.call("prifit_atlas_bwd", L.ptr(table), L.ptr(zt), L.ptr(grid), C, B, P, int(training), L.ptr(gout), L.ptr(out), L.ptr(ws), L.ptr(sc),
           L.ptr(gz), L.ptr(gp), L.cur_stream())
    torch.cuda.synchronize()
    return net, dict(out=(out, out_b), ws=(ws, ws_b), scratch=(sc, sc_b), gz=(gz, gz_b), gparams=(gp, gp_b))


@pytest.mark.parametrize("name", ["3x2x9", "2x3x128"])
def test_guard_bands(hiplib, name):
    """buffers that start as NaN inside and around: a read of a word the call chain has not written shows as a non-finite
    result, a write outside the extent as a changed guard word"""
    from prifit_amd import _lib as L
    net, bufs = _direct(L, name)
    for k, (view, base) in bufs.items():
        assert_guards_intact(base, view)
        if k in ("out", "gz", "gparams"):
            assert torch.isfinite(view).all(), k
    _, _, _, r64, r32 = reference(name)
    e32 = float(np.abs(r32["out"].astype(np.float64) - r64["out"]).max())
    assert float(np.abs(bufs["out"][0].cpu().numpy().astype(np.float64) - r64["out"]).max()) <= 4.0 * e32


def test_flat_adam_adopts_the_parameters(hiplib):
    """FlatAdam moves every parameter into its flat buffer: the pointer table is uploaded again with the new addresses, the
    output keeps its bits, the gradients land where the optimizer reads them and a step changes the output"""
    from prifit_amd.optim import FlatAdam
    B, C, npts, seed, training, const = CASES["3x2x9"]
    sd, z, target = reference("3x2x9")[:3]
    net = build(sd, C, npts, True)
    dev = torch.device("cuda", torch.cuda.current_device())
    zt = torch.from_numpy(z).cuda()
    before = net(zt).detach().clone()
    old = net._table(dev).clone()
    opt = FlatAdam(net.parameters(), lr=1e-2)
    new = net._table(dev)
    w = net.decoder[1].conv2.weight
    lo, hi = opt.flat.data_ptr(), opt.flat.data_ptr() + opt.flat.numel() * 4
    assert not torch.equal(old, new) and int(new[24 + 2]) == w.data_ptr() and lo <= w.data_ptr() < hi
    assert int(new[24 + 10]) == net.decoder[1].bn1.running_mean.data_ptr() == int(old[24 + 10])     # buffers stay
    out = net(zt)
    assert torch.equal(out, before)
    out.square().sum().backward()
    assert all(p.grad is not None and p.grad.is_contiguous() and p.grad.shape == p.shape for p in net.parameters())
    opt.step()
    assert net._table(dev) is new                  # nothing moved: no new upload
    assert not torch.equal(net(zt), before)


def test_bad_arguments(hiplib):
    from prifit_amd import _lib as L
    lib = L.dll()
    t = torch.zeros(4096, device="cuda")
    p, s = L.ptr(t), L.cur_stream()
    ok = (p, p, p, 1, 1, 4, 1, 1e-5, 0.1, p, p, s)
    bad = [(None,) + ok[1:], ok[:1] + (None,) + ok[2:], ok[:2] + (None,) + ok[3:], ok[:3] + (0,) + ok[4:],
           ok[:4] + (0,) + ok[5:], ok[:5] + (0,) + ok[6:], ok[:5] + (1,) + ok[6:], ok[:7] + (0.0,) + ok[8:],
           ok[:8] + (1.5,) + ok[9:], ok[:9] + (None,) + ok[10:], ok[:10] + (None,) + ok[11:], ok[:3] + (70000,) + ok[4:]]
    for args in bad:
        assert lib.prifit_atlas_fwd(*args) == -1, args
    okb = (p, p, p, 1, 1, 4, 1, p, p, p, p, p, p, s)
    for i in (0, 1, 2, 7, 8, 9, 10, 11, 12):
        assert lib.prifit_atlas_bwd(*(okb[:i] + (None,) + okb[i + 1:])) == -1, i
    assert lib.prifit_atlas_bwd(*(okb[:3] + (-1,) + okb[4:])) == -1
    assert lib.prifit_atlas_workspace_floats(0, 1, 4, 0) == 0 and lib.prifit_atlas_workspace_floats(1, 1, 4, 0) > 0


# ---------------------------------------------------------------------------------------------------------- whole model

def _model(reconstruct, seed=ac.MODEL_CASE["seed"]):
    from prifit_amd.models.pointnet2_part_seg_msg import get_model
    torch.manual_seed(seed)
    net = get_model(50, reconstruct=reconstruct)
    if reconstruct:
        net.atlasnet.load_state_dict({k: torch.from_numpy(np.array(v))
                                      for k, v in ac.make_state(ac.MODEL_CASE["decoder_seed"], 25).items()})
    return net.cuda().train()


def test_model_decoder_against_reference(hiplib, golden):
    """the net's own decoder and loss modules on the latent the reference's backbone produced (atlas_model.npz)"""
    G = golden("atlas_model")
    net = _model(True)
    xyz, _ = ac.model_inputs()
    z = torch.from_numpy(G["z"].astype(np.float32)).cuda()
    with torch.no_grad():
        out = net.atlasnet(z)
        rec = net.chamferdistance(out, torch.from_numpy(xyz).cuda().permute(0, 2, 1))
    sd = ac.make_state(ac.MODEL_CASE["decoder_seed"], 25)
    tgt = np.ascontiguousarray(xyz.transpose(0, 2, 1))
    res = {}
    for dt in (torch.float64, torch.float32):
        with torch.no_grad():
            o, _ = ac.decoder(ac.leaves(sd, dt), torch.from_numpy(G["z"]).to(dt), 128, 25, True)
            l, i1, i2 = ac.rec_loss(o, torch.from_numpy(tgt).to(dt))
        res[dt] = (o.numpy(), l.numpy(), i1.numpy(), i2.numpy())
    assert np.array_equal(res[torch.float64][2], res[torch.float32][2]) and np.array_equal(res[torch.float64][3], res[torch.float32][3])
    for k, got, ref, r32 in (("output_points", out.cpu().numpy(), G["output_points"], res[torch.float32][0]),
                             ("rec", rec.cpu().numpy(), G["rec"], res[torch.float32][1])):
        e32 = float(np.abs(r32.astype(np.float64) - ref).max())
        e = float(np.abs(got.astype(np.float64) - ref).max())
        print("model %-14s e32 %.3e kernel %.3e ratio %.2f" % (k, e32, e, e / e32))
        assert e <= 4.0 * e32, (k, e, e32)


def test_model_six_tuple_and_gradients(hiplib):
    net = _model(True)
    xyz, cls = ac.model_inputs()
    x, c = torch.from_numpy(xyz).cuda(), torch.from_numpy(cls).cuda()
    torch.manual_seed(7)                # the farthest-point sampling starts at random points
    out = net(x, c)
    B, N = xyz.shape[0], xyz.shape[2]
    assert len(out) == 6
    # the latent is the mean over the points of the fp1 output, not of feat (training-mode outputs do not depend on the
    # running statistics, so the second pass gives the same bits)
    with torch.no_grad():
        torch.manual_seed(7)
        l0 = net._embed_with_l0(x, c)[4]
        assert tuple(l0.shape) == (B, N, 128)
        assert torch.equal(net.atlasnet(l0.mean(dim=1)), out[5])
        assert not torch.equal(net.atlasnet(out[2].mean(dim=2).contiguous()), out[5])
    assert tuple(out[0].shape) == (B, N, 50) and tuple(out[2].shape) == (B, 128, N) and tuple(out[5].shape) == (B, 25 * 121, 3)
    assert tuple(out[3].shape) == (1,) and tuple(out[4].shape) == (1,) and float(out[4]) == 0.0
    with torch.no_grad():
        rec = net.chamferdistance(out[5], torch.from_numpy(xyz).cuda().permute(0, 2, 1))
    assert torch.equal(out[3], torch.zeros(1, device="cuda") + rec)
    out[3].backward()
    for p in (net.atlasnet.decoder[24].conv1.weight, net.sa1.conv_blocks[0][0].weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0.0


def test_model_without_reconstruct_is_unchanged(hiplib):
    """the backbone outputs do not depend on the flag: a reconstruct=False net and a reconstruct=True net of the same seed give
    the same bits in every output they share"""
    xyz, cls = ac.model_inputs()
    x, c = torch.from_numpy(xyz).cuda(), torch.from_numpy(cls).cuda()
    a, b = _model(False), _model(True)
    b.load_state_dict(a.state_dict(), strict=False)
    a.drop1.eval(); b.drop1.eval()
    torch.manual_seed(7)            # the farthest-point sampling starts at random points
    oa = a(x, c)
    torch.manual_seed(7)
    ob = b(x, c)
    assert len(oa) == 5 and float(oa[3]) == 0.0 and float(oa[4]) == 0.0
    assert torch.equal(oa[0], ob[0]) and torch.equal(oa[2], ob[2])
    for u, v in zip(oa[1], ob[1]):
        assert torch.equal(u, v)


def _sha(t):
    import hashlib
    return np.frombuffer(hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).digest(), np.uint8)


def test_model_without_reconstruct_matches_recorded_bits(hiplib, golden):
    """seg and feat of the reconstruct=False net at the seeded whole-model case, against SHA-256 digests recorded on an MI355X
    (tests/golden/atlas_model_digest.npz).  First recorded from the revision before reconstruct=True existed; recorded again,
    by this test's own recipe, when the streaming forward began to sum its column statistics per accumulator tile (DESIGN.md,
    the streaming kernels' tests): the library before that change still gives the first digests, the one after it gives
    these in two separate processes."""
    G = golden("atlas_model_digest")
    xyz, cls = ac.model_inputs()
    a = _model(False)
    a.drop1.eval()
    torch.manual_seed(7)
    oa = a(torch.from_numpy(xyz).cuda(), torch.from_numpy(cls).cuda())
    assert np.array_equal(_sha(oa[0]), G["seg"]) and np.array_equal(_sha(oa[2]), G["feat"])


def test_model_with_convex_loss(hiplib):
    """out[3] = the convex loss of the reconstruct=False net with the same backbone weights + rec; still the 6-tuple"""
    from prifit_amd import synth
    from tests_helpers import fit_inputs
    _, cham, _ = fit_inputs(2, 1024, 128, 8)
    x = cham[:, :1024].transpose(1, 2).contiguous().cuda()
    ch = cham.transpose(1, 2).contiguous().cuda()
    R = torch.from_numpy(synth.uniform01((3, 3), 3)).cuda()
    a, b = _model(False, 32), _model(True, 32)
    b.load_state_dict(a.state_dict(), strict=False)
    kw = dict(chamfer_points=ch, include_convex_loss=True, quantile=0.05, msc_iterations=5, max_num_clusters=25,
              fit_inputs=dict(rand_table=R))
    cls = torch.zeros(2, 1, 16, device="cuda")
    with torch.no_grad():
        torch.manual_seed(7)        # the farthest-point sampling starts at random points
        oa = a(x, cls, **kw)
        torch.manual_seed(7)
        ob = b(x, cls, **kw)
        rec = b.chamferdistance(ob[5], x.permute(0, 2, 1))
    assert len(ob) == 6 and float(ob[4].abs().sum()) == 0.0 and tuple(ob[4].shape) == (1,)
    want = float(oa[3].sum()) + float(rec)
    print("convex %.6f rec %.6f total %.6f" % (float(oa[3].sum()), float(rec), float(ob[3].sum())))
    assert abs(float(ob[3].sum()) - want) <= 1e-5 * abs(want) + 1e-7

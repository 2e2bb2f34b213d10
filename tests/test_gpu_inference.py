"""GPU: frozen inference (prifit_amd/inference.py, csrc/infer.hip) -- the one-launch BatchNorm fold against an fp64 numpy fold
inside guard bands, the chain kernel against an fp64 numpy restatement with the existing eval route as the yardstick of its
error, and the frozen network end to end against the live model in eval mode."""
import ctypes

import numpy as np
import pytest
import torch

import guard_common as GC

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
CHAIN_SHAPES = [(32, 32, 64, 32), (64, 64, 128, 64), (64, 96, 128, 128), (128, 128, 256, 64), (128, 196, 256, 128)]


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _ptrs(ts):
    return _arr(ctypes.c_void_p, [None if t is None else t.data_ptr() for t in ts])


# ---------------------------------------------------------------------------------------------- fold
def test_fold_bn_against_fp64_in_guard_bands():
    """5 jobs: widths 1, 3, 64, 196, one NULL bias, one NULL gamma (a copy), running variances with 0 and 1e-12.
    |W' - ref| <= 4 u |ref|, u = 2^-23: the sqrt, the divide and the multiply round once each (half an ulp), the sum var + eps
    once more -- derived, not measured; |b' - ref| <= 4 u (|b - mean| |s| + |beta|)."""
    from prifit_amd._lib import call, cur_stream
    rng = np.random.default_rng(7)
    eps = float(np.float32(1e-5))
    jobs = []        # (cout, kin, has_bias, has_bn)
    for cout, kin, has_bias, has_bn in ((1, 5, False, True), (3, 9, True, True), (64, 64, True, True), (196, 128, True, True),
                                        (64, 6, True, False)):
        j = {"W": rng.standard_normal((cout, kin)).astype(np.float32),
             "b": rng.standard_normal(cout).astype(np.float32) if has_bias else None}
        if has_bn:
            var = rng.uniform(0.1, 2.0, cout).astype(np.float32)
            var[0] = 0.0
            if cout > 2:
                var[2] = 1e-12
            j.update(gamma=rng.uniform(-1.5, 1.5, cout).astype(np.float32), beta=rng.standard_normal(cout).astype(np.float32),
                     mean=rng.standard_normal(cout).astype(np.float32), var=var)
        jobs.append(j)
    off, place = 0, []
    for j in jobs:
        cout, kin = j["W"].shape
        ldw = (kin + 3) // 4 * 4
        place.append((off, ldw, off + cout * ldw + 12))          # 12 floats between a job's W' and its b': not the kernel's
        off += cout * ldw + 12 + cout + 20                       # and 20 behind
        off = (off + 3) // 4 * 4
    flat, base = GC.guarded((off,), 4096, 4096, poison=GC.SENTINEL)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    t = {k: [dev(j.get(k)) for j in jobs] for k in ("W", "b", "gamma", "beta", "mean", "var")}
    n = len(jobs)
    call("prifit_fold_bn", n, _ptrs(t["W"]), _arr(ctypes.c_int32, [j["W"].shape[0] for j in jobs]),
         _arr(ctypes.c_int32, [j["W"].shape[1] for j in jobs]), _ptrs(t["b"]), _ptrs(t["gamma"]), _ptrs(t["beta"]), _ptrs(t["mean"]),
         _ptrs(t["var"]), _arr(ctypes.c_float, [eps] * n), _arr(ctypes.c_longlong, [p[0] for p in place]),
         _arr(ctypes.c_int32, [p[1] for p in place]), _arr(ctypes.c_longlong, [p[2] for p in place]), flat.data_ptr(),
         ctypes.c_longlong(flat.numel()), cur_stream())
    torch.cuda.synchronize()
    GC.assert_guards_intact(base, flat)
    got = flat.cpu().numpy()
    owned = np.zeros(off, dtype=bool)
    for j, (w_off, ldw, b_off) in zip(jobs, place):
        cout, kin = j["W"].shape
        Wg = got[w_off:w_off + cout * ldw].reshape(cout, ldw)
        bg = got[b_off:b_off + cout]
        owned[w_off:w_off + cout * ldw] = True
        owned[b_off:b_off + cout] = True
        assert np.all(Wg[:, kin:] == 0.0)                                    # the padding to a 16-byte row
        W64 = j["W"].astype(np.float64)
        b64 = np.zeros(cout) if j["b"] is None else j["b"].astype(np.float64)
        if "gamma" not in j:
            assert np.array_equal(Wg[:, :kin].view(np.int32), j["W"].view(np.int32))      # the copy job: bit for bit
            assert np.array_equal(bg.view(np.int32), j["b"].view(np.int32))
            continue
        s = j["gamma"].astype(np.float64) / np.sqrt(j["var"].astype(np.float64) + np.float64(np.float32(eps)))
        Wr = W64 * s[:, None]
        br = (b64 - j["mean"]) * s + j["beta"]
        ew = np.abs(Wg[:, :kin] - Wr)
        print("fold job cout=%d: max |W' - ref| / |ref| = %.3g u" % (cout, float(np.max(ew / np.maximum(np.abs(Wr), 1e-300))) / U))
        assert np.all(ew <= 4 * U * np.abs(Wr))
        bound = 4 * U * (np.abs(b64 - j["mean"]) * np.abs(s) + np.abs(j["beta"].astype(np.float64)))
        print("fold job cout=%d: max |b' - ref| / bound = %.3g" % (cout, float(np.max(np.abs(bg - br) / bound))))
        assert np.all(np.abs(bg - br) <= bound)
    # the words between the jobs' regions are not the kernel's either
    assert np.all(flat.view(torch.int32).cpu().numpy()[~owned] == GC.poison_bits(GC.SENTINEL))


# ---------------------------------------------------------------------------------------------- chain kernel
def _chain_inputs(C0, C1, C2, K, G, seed, dead_group=None):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((G * K, C0)).astype(np.float32)
    W1 = (rng.standard_normal((C1, C0)) / np.sqrt(C0)).astype(np.float32)
    W2 = (rng.standard_normal((C2, C1)) / np.sqrt(C1)).astype(np.float32)
    b1 = (0.1 * rng.standard_normal(C1)).astype(np.float32)
    b2 = (0.1 * rng.standard_normal(C2)).astype(np.float32)
    if dead_group is not None:
        # every output of that group negative before the last ReLU: its inputs are <= 0 and no layer-1 bias is positive, so
        # layer 1 gives exactly 0 and layer 2 its bias, which is negative
        b1, b2 = -np.abs(b1), -np.abs(b2) - np.float32(0.01)
        X[dead_group * K:(dead_group + 1) * K] = -np.abs(X[dead_group * K:(dead_group + 1) * K])
    return X, W1, b1, W2, b2


def _chain_ref(X, W1, b1, W2, b2, K):
    """fp64 restatement -> (pooled [G, C2], scale [G, C2]): scale = the largest sum_k |a_k| |w_k| (+ |bias|) of the last
    product among the group's rows -- what one rounding of that product is relative to."""
    X, W1, b1, W2, b2 = (a.astype(np.float64) for a in (X, W1, b1, W2, b2))
    h = np.maximum(np.maximum(X, 0.0) @ W1.T + b1, 0.0)
    y = np.maximum(h @ W2.T + b2, 0.0)
    mag = np.abs(h) @ np.abs(W2).T + np.abs(b2)
    G = X.shape[0] // K
    return y.reshape(G, K, -1).max(axis=1), mag.reshape(G, K, -1).max(axis=1)


def _eval_route(X, W1, b1, W2, b2, K):
    """The existing eval route on the same weights and (identity) statistics: SharedMLPFn, training=False."""
    from prifit_amd.nn_ops import FrontEnd, SharedMLPFn
    ident = lambda c: [torch.ones(c, device="cuda"), torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda"),
                       torch.ones(c, device="cuda")]
    ts = [None, None] + ident(X.shape[1]) + [W1, b1] + ident(W1.shape[0]) + [W2, b2] + ident(W2.shape[0])
    cfg = {"pool_K": K, "training": False, "eps": 0.0, "momentum": [0.1] * 3, "front": FrontEnd("preact", True)}
    with torch.no_grad():
        return SharedMLPFn.apply(X, cfg, *ts)


@pytest.mark.parametrize("C0,C1,C2,K,G,dead,ld_gap", [
    (32, 32, 64, 32, 3, None, 0), (64, 64, 128, 64, 3, 1, 0), (64, 96, 128, 128, 3, None, 24), (128, 128, 256, 64, 3, None, 0),
    (128, 196, 256, 128, 3, None, 0), (32, 32, 64, 32, 5, 4, 8)])
def test_chain_kernel_against_fp64_and_the_eval_route(C0, C1, C2, K, G, dead, ld_gap):
    """G odd: the last 128-row tile is partial; K = 32: a tile spans four groups.  The kernel's error against fp64, in
    units of sum |a_k| |w_k| of the last product, is at most twice the existing eval route's on the same inputs (another
    summation order over the same fp32 MFMA arithmetic).  NaN guards around every input, sentinel guards around the output
    window (and in its row gap where ld_out > C2)."""
    from prifit_amd._lib import call, cur_stream, query
    if not query("prifit_mlp_chain_pool_supported", C0, C1, C2, K):
        pytest.fail("the chain kernel does not take (%d, %d, %d, %d)" % (C0, C1, C2, K))
    Xn, W1n, b1n, W2n, b2n = _chain_inputs(C0, C1, C2, K, G, 100 + C1 + G, dead)
    ref, scale = _chain_ref(Xn, W1n, b1n, W2n, b2n, K)
    tail = 1 << 14
    X, W1, b1, W2, b2 = (GC.guarded_like(torch.from_numpy(a).cuda(), tail, tail)[0] for a in (Xn, W1n, b1n, W2n, b2n))
    out, base = GC.guarded_matrix(G, C2, C2 + ld_gap, 4096, 4096, poison=GC.SENTINEL)
    call("prifit_mlp_chain_pool_f32", X.data_ptr(), ctypes.c_longlong(C0), G, K, C0, C1, C2, W1.data_ptr(), ctypes.c_longlong(C0),
         b1.data_ptr(), W2.data_ptr(), ctypes.c_longlong(C1), b2.data_ptr(), out.data_ptr(), ctypes.c_longlong(out.stride(0)), None,
         cur_stream())
    torch.cuda.synchronize()
    GC.assert_guards_intact(base, out)
    got = out.cpu().numpy().astype(np.float64)
    live = _eval_route(X, W1, b1, W2, b2, K).cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
    e_chain = float(np.max(np.abs(got - ref) / scale))
    e_live = float(np.max(np.abs(live - ref) / scale))
    print("chain (%d, %d, %d) K=%d G=%d: chain %.3g u, eval route %.3g u" % (C0, C1, C2, K, G, e_chain / U, e_live / U))
    if dead is not None:
        assert np.all(ref[dead] == 0.0) and np.all(got[dead] == 0.0)
        assert np.any(got[:dead] > 0.0)
    assert e_chain <= 2.0 * e_live


def test_chain_supported_rejects_other_shapes():
    from prifit_amd._lib import query
    assert query("prifit_mlp_chain_pool_supported", 256, 512, 1024, 128) == 0
    for C0, C1, C2, _ in CHAIN_SHAPES:
        assert query("prifit_mlp_chain_pool_supported", C0, C1, C2, 0) == 0


# ---------------------------------------------------------------------------------------------- end to end
def _gather(table, idx):
    B = table.shape[0]
    flat = idx.reshape(B, -1).long()
    return torch.gather(table, 1, flat.unsqueeze(-1).expand(-1, -1, table.shape[-1])).reshape(*idx.shape, table.shape[-1])


def _ref64(frozen, xyz, onehot, fps_start):
    """fp64 torch run of the folded network on the CPU.  The index lists (sampling, ball query, 3-NN and its weights) are
    the GPU entry points' own: what is measured is the arithmetic of the layers, not a tie in a distance comparison."""
    from prifit_amd import ops
    cpu = lambda t: t.detach().double().cpu()
    Wb = lambda ly: (cpu(ly.W[:, :ly.kin]), cpu(ly.b))
    B, _, N = xyz.shape
    pts_g = xyz.permute(0, 2, 1).contiguous()
    xyz_g = pts_g[:, :, :3].contiguous()
    pts, l0_xyz = cpu(pts_g), cpu(xyz_g)

    def mlp(x, layers):
        for ly in layers:
            W, b = Wb(ly)
            x = torch.relu(x @ W.t() + b)
        return x

    def sa(lv, xyz_gpu, xyz_c, feats, start):
        S = lv["npoint"]
        _, nx_gpu = ops.farthest_point_sample(xyz_gpu, S, start, return_xyz=True)
        lists = ops.ball_query_multi(lv["radii"], lv["nsamples"], xyz_gpu, nx_gpu)
        centres = cpu(nx_gpu)
        outs = []
        for (st, _), gi, K in zip(lv["scales"], lists, lv["nsamples"]):
            gi = gi.cpu()
            g = torch.cat([_gather(feats, gi), _gather(xyz_c, gi) - centres.unsqueeze(2)], dim=-1)
            outs.append(mlp(g.reshape(B * S * K, -1), st).reshape(B, S, K, -1).amax(dim=2))
        return nx_gpu, centres, torch.cat(outs, dim=-1)

    def fp(name, x1_gpu, x2_gpu, p1, p2):
        st = frozen._fp[name][0]
        if p2.shape[1] == 1:
            interp = p2.expand(B, p1.shape[1], -1)
        else:
            idx, w = ops.three_nn(x1_gpu, x2_gpu)
            interp = (_gather(p2, idx.cpu()) * cpu(w).unsqueeze(-1)).sum(dim=2)
        x = torch.cat([p1, interp], dim=-1)                                     # upstream's order
        return mlp(x.reshape(-1, x.shape[-1]), st).reshape(B, p1.shape[1], -1)

    l1_gpu, l1_xyz, l1_points = sa(frozen._sa[0], xyz_g, l0_xyz, pts, fps_start[0])
    l2_gpu, l2_xyz, l2_points = sa(frozen._sa[1], l1_gpu, l1_xyz, l1_points, fps_start[1])
    g = torch.cat([l2_xyz, l2_points], dim=-1)
    l3_points = mlp(g.reshape(-1, g.shape[-1]), frozen._sa3[0]).reshape(B, l2_xyz.shape[1], -1).amax(dim=1, keepdim=True)
    l2_up = fp("fp3", None, None, l2_points, l3_points)
    l1_up = fp("fp2", l1_gpu, l2_gpu, l1_points, l2_up)
    skip = torch.cat([cpu(onehot).reshape(B, 1, 16).expand(B, N, 16), l0_xyz, pts], dim=-1)
    l0_up = fp("fp1", xyz_g, l1_gpu, skip, l1_up)
    feat = mlp(l0_up.reshape(B * N, -1), frozen._head)
    W, b = Wb(frozen._conv2)
    seg = torch.log_softmax(feat @ W.t() + b, dim=1).reshape(B, N, -1)
    return seg, feat.reshape(B, N, -1).permute(0, 2, 1)


def _trained_model(normal, seed):
    """get_model(50) with random gamma / beta and running statistics moved by three training-mode forwards."""
    from prifit_amd.models import pointnet2_part_seg_msg as M
    torch.manual_seed(seed)
    net = M.get_model(50, normal_channel=normal).cuda()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.1)
    net.train()
    C = 6 if normal else 3
    for _ in range(3):
        _train_forward(net, C)
    return net.eval()


def _train_forward(net, C, B=2, N=1024):
    net.train()
    with torch.no_grad():
        net(torch.rand(B, C, N, device="cuda") * 2 - 1, torch.eye(16, device="cuda")[torch.randint(0, 16, (B,))].reshape(B, 1, 16))
    net.eval()


def _inputs(B, C, N, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(B, C, N, generator=g) * 2 - 1).cuda()
    onehot = torch.eye(16)[torch.randint(0, 16, (B,), generator=g)].reshape(B, 1, 16).cuda()
    start = (torch.randint(0, N, (B,), generator=g).cuda(), torch.randint(0, 512, (B,), generator=g).cuda())
    return xyz, onehot, start


@pytest.fixture(scope="module", params=[(False, 2), (True, 1)], ids=["xyz_B2", "normals_B1"])
def e2e(request):
    """One live / frozen / fp64 triple per configuration, shared by the tests below and left unchanged by them."""
    from prifit_amd import inference
    normal, B = request.param
    net = _trained_model(normal, 3 + B)
    frozen = inference.freeze(net)
    xyz, onehot, start = _inputs(B, 6 if normal else 3, 1024, 11)
    with torch.no_grad():
        live = net(xyz, onehot, fps_start=start)
    got = frozen(xyz, onehot, fps_start=start)
    ref_seg, ref_feat = _ref64(frozen, xyz, onehot, start)
    torch.cuda.synchronize()
    return dict(net=net, frozen=frozen, xyz=xyz, onehot=onehot, start=start, live=live, got=got, ref_seg=ref_seg, ref_feat=ref_feat,
                C=6 if normal else 3)


def test_frozen_forward_matches_the_live_eval_forward(e2e):
    live, got = e2e["live"], e2e["got"]
    assert len(got) == len(live) == 5
    for a, b in zip(got[1], live[1]):
        assert a.shape == b.shape
    assert got[0].shape == live[0].shape and got[2].shape == live[2].shape
    for k in (3, 4):
        assert got[k].shape == live[k].shape and float(got[k].abs().sum()) == 0.0
    for name, k, ref in (("seg", 0, e2e["ref_seg"]), ("feat", 2, e2e["ref_feat"])):
        bar = 2.0 * float((live[k].double().cpu() - ref).abs().max())
        diff = float((got[k] - live[k]).abs().max())
        own = float((got[k].double().cpu() - ref).abs().max())
        print("%s: |frozen - live| %.3g, bar %.3g (2 x the live route's error against fp64); frozen against fp64 %.3g"
              % (name, diff, bar, own))
        assert diff <= bar, name
        if name == "seg":
            top2 = live[0].topk(2, dim=-1).values
            sure = (top2[..., 0] - top2[..., 1]) > bar
            assert bool(sure.any())
            assert torch.equal(got[0].argmax(-1)[sure], live[0].argmax(-1)[sure])


def test_snapshot_and_refresh(e2e):
    net, frozen = e2e["net"], e2e["frozen"]
    args = (e2e["xyz"], e2e["onehot"])
    state = {k: v.clone() for k, v in net.state_dict().items()}
    try:
        _train_forward(net, e2e["C"])                                   # the live statistics move ...
        again = frozen(*args, fps_start=e2e["start"])
        assert torch.equal(again[0], e2e["got"][0]) and torch.equal(again[2], e2e["got"][2])   # ... the snapshot does not
        frozen.refresh()
        moved = frozen.predict(*args, fps_start=e2e["start"])
        assert moved.shape == again[0].shape and not torch.equal(moved, again[0])
    finally:
        net.load_state_dict(state)
        frozen.refresh()
    back = frozen(*args, fps_start=e2e["start"])
    assert torch.equal(back[0], e2e["got"][0])


def test_frozen_module_protocol(e2e):
    frozen = e2e["frozen"]
    with pytest.raises(ValueError):
        frozen(e2e["xyz"], e2e["onehot"], include_convex_loss=True)
    with pytest.raises(RuntimeError):
        frozen.train()
    assert frozen.eval() is frozen and not frozen.training
    ps = list(frozen.parameters())
    assert len(ps) == 1 and ps[0].dim() == 1 and not ps[0].requires_grad and ps[0].dtype == torch.float32 and ps[0].is_cuda
    assert not list(frozen.buffers())
    out = frozen(e2e["xyz"], e2e["onehot"], fps_start=e2e["start"], evaluation=True, quantile=0.05, msc_iterations=3, alpha=1)
    assert len(out) == 5 and torch.equal(out[0], e2e["got"][0])


def test_frozen_forward_launches(e2e, monkeypatch):
    """No statistics kernels, one chain launch per SA1 / SA2 scale."""
    import prifit_amd.inference as I
    import prifit_amd.models.pointnet_util as PU
    import prifit_amd.nn_ops as NN
    import prifit_amd.ops as O
    from prifit_amd import _lib
    seen = []

    def spy(name, *args):
        seen.append(name)
        return _lib.call(name, *args)

    for mod in (I, PU, NN, O):
        monkeypatch.setattr(mod, "call", spy)
    e2e["frozen"](e2e["xyz"], e2e["onehot"], fps_start=e2e["start"])
    assert "prifit_bn_finalize" not in seen and "prifit_col_stats" not in seen
    assert not any("bwd" in n or "stats" in n for n in seen)
    assert seen.count("prifit_mlp_chain_pool_f32") == 5
    assert seen.count("prifit_sa_group_linear_fwd") == 2 and seen.count("prifit_fps") == 2


def test_evaluate_loader_runs_unchanged_on_the_frozen_model(e2e):
    from prifit_amd import testing as T
    rng = np.random.default_rng(5)
    batches = []
    for _ in range(2):
        cats = rng.integers(0, 16, 2)
        target = np.stack([rng.choice(T.seg_classes[T.classes[c]], 1024) for c in cats]).astype(np.int64)
        batches.append((rng.uniform(-1, 1, (2, 1024, e2e["C"])).astype(np.float32), cats.reshape(2, 1).astype(np.int64), target))
    preds = {}
    for name, model in (("live", e2e["net"]), ("frozen", e2e["frozen"])):
        torch.manual_seed(21)                                          # the random sampling starts of both runs
        ev = T.SegmentationEvaluator()
        with torch.no_grad():
            preds[name] = [ev.predict(model(torch.from_numpy(p).cuda().transpose(2, 1).contiguous(),
                                            T.to_categorical(torch.from_numpy(l).cuda(), 16))[0], torch.from_numpy(t).cuda())[0]
                           for p, l, t in batches]
    agreed = all(torch.equal(a, b) for a, b in zip(preds["live"], preds["frozen"]))
    torch.manual_seed(21)
    m_live = T.evaluate_loader(e2e["net"], batches)
    torch.manual_seed(21)
    m_frozen = T.evaluate_loader(e2e["frozen"], batches)
    assert set(m_frozen) == set(m_live) and set(m_frozen["category_iou"]) == set(m_live["category_iou"])
    assert not e2e["net"].training and not e2e["frozen"].training
    print("evaluate_loader: predictions agree everywhere: %s" % agreed)
    if agreed:
        for k in ("accuracy", "class_avg_accuracy", "class_avg_iou", "instance_avg_iou", "chamfer_loss"):
            assert m_frozen[k] == m_live[k] or (np.isnan(m_frozen[k]) and np.isnan(m_live[k])), k

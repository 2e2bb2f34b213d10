"""GPU: classifier-layer pre-training on the frozen network (csrc/probe_head.hip prifit_probe_head_f32, FrozenPartSeg.probe_step,
Trainer.init_classifier) -- loss, conv2 gradient and accuracy count of the fused head against the fp64 restatement of
tests/probe_common.py with the existing separate launches as the yardstick of its error, the label rules, guard bands round
every operand, determinism, and three iterations end to end against the live eval-mode route."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import guard_common as GC
import probe_common as PC

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
G = PC.GRID


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _workspace(P, K0, CL):
    from prifit_amd._lib import dll
    return dll().prifit_probe_head_workspace(P, K0, 4, _arr(ctypes.c_int32, [128, 128, 128, CL]))


def _launch(X, Ws, bs, target, dW, db, loss, ws):
    from prifit_amd._lib import call, cur_stream
    P, K0 = X.shape
    call("prifit_probe_head_f32", X.data_ptr(), X.stride(0), P, K0, 4, _arr(ctypes.c_int32, [W.shape[0] for W in Ws]),
         _arr(ctypes.c_void_p, [W.data_ptr() for W in Ws]), _arr(ctypes.c_longlong, [W.stride(0) for W in Ws]),
         _arr(ctypes.c_void_p, [b.data_ptr() for b in bs]), target.data_ptr(), dW.data_ptr(), dW.stride(0), db.data_ptr(),
         loss.data_ptr(), ws.data_ptr(), cur_stream())
    torch.cuda.synchronize()


def _run(Xn, Wn, bn, tn):
    """The entry point on host arrays -> (loss [4], dW [CL, 128], db [CL]) as float64 numpy, every output pre-filled with NaN."""
    P, K0 = Xn.shape
    CL = Wn[3].shape[0]
    X, target = torch.from_numpy(Xn).cuda(), torch.from_numpy(tn).cuda()
    Ws, bs = [torch.from_numpy(w).cuda() for w in Wn], [torch.from_numpy(b).cuda() for b in bn]
    dW, db = torch.full((CL, 128), float("nan"), device="cuda"), torch.full((CL,), float("nan"), device="cuda")
    loss = torch.full((4,), float("nan"), device="cuda")
    ws = torch.full((_workspace(P, K0, CL),), float("nan"), device="cuda")
    _launch(X, Ws, bs, target, dW, db, loss, ws)
    return loss.cpu().numpy().astype(np.float64), dW.cpu().numpy().astype(np.float64), db.cpu().numpy().astype(np.float64)


def _separate_route(Xn, Wn, bn, tn):
    """Route (b), the launches the fused head replaces: the row chain's scores (prifit_mlp_chain_rows_f32), a3 from the
    products and ReLU launches of FrozenPartSeg._stack, torch's log_softmax, prifit_cross_entropy_fwd / _bwd and the TN
    product of the training path; db = torch's column sum.  -> (loss, dW, db) as float64 numpy."""
    from prifit_amd import nn_ops
    from prifit_amd._lib import call, cur_stream
    P, K0 = Xn.shape
    CL = Wn[3].shape[0]
    X, target = torch.from_numpy(Xn).cuda(), torch.from_numpy(tn).cuda()
    Ws, bs = [torch.from_numpy(w).cuda() for w in Wn], [torch.from_numpy(b).cuda() for b in bn]
    ones, zeros = torch.ones(128, device="cuda"), torch.zeros(128, device="cuda")

    def product(x, W, b, unit):
        y = torch.empty(P, W.shape[0], dtype=torch.float32, device="cuda")
        nn_ops.gemm(nn_ops.NT, P, W.shape[0], W.shape[1], x, x.stride(0), W, W.stride(0), y, W.shape[0],
                    a_affine=(ones, zeros) if unit else None, bias=b)
        return y

    h = product(X, Ws[0], bs[0], False)
    h = torch.relu(product(h, Ws[1], bs[1], True))
    a3 = torch.relu(product(h, Ws[2], bs[2], False))
    scores = torch.empty(P, CL, device="cuda")
    call("prifit_mlp_chain_rows_f32", X.data_ptr(), X.stride(0), P, K0, 4, _arr(ctypes.c_int32, [W.shape[0] for W in Ws]),
         _arr(ctypes.c_void_p, [W.data_ptr() for W in Ws]), _arr(ctypes.c_longlong, [W.stride(0) for W in Ws]),
         _arr(ctypes.c_void_p, [b.data_ptr() for b in bs]), scores.data_ptr(), CL, None, None, None, P, None, cur_stream())
    y = torch.log_softmax(scores, dim=1).requires_grad_()
    loss = nn_ops.CrossEntropyFn.apply(y, target)
    loss.backward()                                       # prifit_cross_entropy_bwd: d loss / d y = softmax(y) - onehot
    dy = y.grad
    dz = dy - torch.exp(y.detach()) * dy.sum(dim=1, keepdim=True)      # log_softmax's backward, as autograd forms it
    dW = nn_ops._weight_grad(dz.contiguous(), P, CL, a3, 128, None, out=torch.zeros(CL, 128, device="cuda"))
    db = dz.sum(dim=0)
    torch.cuda.synchronize()
    return float(loss.detach()), dW.cpu().numpy().astype(np.float64), db.cpu().numpy().astype(np.float64)


def _err(got, ref, scale):
    """Largest error in units of the sum |.| |.| scale; where the reference is identically zero the result must be too."""
    got, ref, scale = np.atleast_1d(got), np.atleast_1d(ref), np.atleast_1d(scale)
    zero = scale == 0
    assert np.all(got[zero] == 0), "a non-zero where the reference is identically zero"
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got - ref)[~zero] / scale[~zero]))


@pytest.mark.parametrize("K0,CL", [(152, 50), (160, 64), (8, 50), (64, 33), (152, 1)])
@pytest.mark.parametrize("P", [1, 33, 129, 128 * G + 40])
def test_against_fp64_and_the_separate_launches(P, K0, CL):
    """P = 1: one live row; 33: the second lane half of a wave partly live; 129: a second workgroup with one row; 128 G + 40:
    every workgroup of the fixed grid takes a tile, the first a second, ragged one.  The errors of loss, dW and db against the fp64
    restatement, in units of their sum |.| |.| scales, are at most twice those of the separate launches on the same inputs;
    kept and correct are exact; C_L = 1 gives dz = 0 and exact zeros.
    Measured on an MI355X (fused / separate, in u = 2^-23 of the scale; the whole table is in DESIGN.md 3.9.3): K0 = 152, C_L = 50:
    P = 1 loss 0.068 / 0.89, dW 89.3 / 90.6, db 2.68 / 4.29; P = 32808 loss 0.164 / 0.164, dW 9.58 / 9.45, db 0.128 / 0.178.  The
    largest ratio of the 60 is db at K0 = 152, P = 129: 1.1 / 0.707 = 1.56."""
    Xn, Wn, bn, tn = PC.net(P, K0, CL, 2000 + 7 * K0 + CL + P % 1000)
    ref = PC.probe(Xn, Wn, bn, tn)
    loss, dW, db = _run(Xn, Wn, bn, tn)
    s_loss, s_dW, s_db = _separate_route(Xn, Wn, bn, tn)
    assert np.all(np.isfinite(loss)) and np.all(np.isfinite(dW)) and np.all(np.isfinite(db))
    assert loss[1] == ref["kept"] == P and loss[2] == ref["correct"] and loss[3] == 0
    for name, got, sep, want, scale in (("loss", loss[0], s_loss, ref["loss"], ref["loss_scale"]),
                                        ("dW", dW, s_dW, ref["dW"], ref["dW_scale"]), ("db", db, s_db, ref["db"], ref["db_scale"])):
        e_fused, e_sep = _err(got, want, scale), _err(sep, want, scale)
        print("probe head K0=%d C_L=%d P=%d %s: fused %.3g u, separate launches %.3g u" % (K0, CL, P, name, e_fused / U, e_sep / U))
        assert e_fused <= 2.0 * e_sep, name


def test_label_rules():
    """P = 200 with 37 rows labelled -100: the restatement on the kept rows.  Every row ignored: a NaN loss, zero gradients (what
    torch gives on the CPU, tests/test_probe_restatement.py).  One out-of-range label: a NaN loss."""
    P, K0, CL = 200, 152, 50
    Xn, Wn, bn, tn = PC.net(P, K0, CL, 91)
    tn[np.random.default_rng(92).choice(P, 37, replace=False)] = PC.IGNORE
    ref = PC.probe(Xn, Wn, bn, tn)
    loss, dW, db = _run(Xn, Wn, bn, tn)
    assert loss[1] == 163 == ref["kept"] and loss[2] == ref["correct"]
    # the data arrived (precision is the first test's subject): an fp32 sum of K <= 160 terms is within K u = 2e-5 of its
    # scale in the worst case, four layers and the head on top of each other stay below 1e-4
    assert abs(loss[0] - ref["loss"]) <= 1e-4 * ref["loss_scale"]
    assert np.all(np.abs(dW - ref["dW"]) <= 1e-4 * ref["dW_scale"]) and np.all(np.abs(db - ref["db"]) <= 1e-4 * ref["db_scale"])
    # the gradient does not see the dropped rows at all: the same bits without them
    keep = tn != PC.IGNORE
    tn2 = tn.copy()
    Xn2 = Xn.copy()
    Xn2[~keep] = 7.0
    loss2, dW2, db2 = _run(Xn2, Wn, bn, tn2)
    assert np.array_equal(loss2, loss) and np.array_equal(dW2, dW) and np.array_equal(db2, db)
    tn[:] = PC.IGNORE
    loss, dW, db = _run(Xn, Wn, bn, tn)
    assert np.isnan(loss[0]) and loss[1] == 0 and loss[2] == 0 and not dW.any() and not db.any()
    Xn, Wn, bn, tn = PC.net(P, K0, CL, 93)
    tn[150] = CL
    loss, dW, db = _run(Xn, Wn, bn, tn)
    assert np.isnan(loss[0]) and loss[1] == P and np.isnan(dW).all() and np.isnan(db).all()
    tn[150] = -1
    assert np.isnan(_run(Xn, Wn, bn, tn)[0][0])


def test_correct_count_ties_and_nan():
    """Channels 3 and 4 share a row of W_4 / b_4 with a bias that makes them the maximum: the first wins, so rows labelled 3 count
    and rows labelled 4 do not.  A NaN input row makes every score NaN: the first channel is its arg-max (and its loss NaN)."""
    P, K0, CL = 70, 152, 50
    Xn, Wn, bn, tn = PC.net(P, K0, CL, 94)
    Wn[3][4] = Wn[3][3]
    bn[3][3] = bn[3][4] = 100.0
    tn[:35], tn[35:] = 3, 4
    loss, _, _ = _run(Xn, Wn, bn, tn)
    assert loss[1] == P and loss[2] == 35 and np.isfinite(loss[0])
    Xn[5] = np.nan
    tn[5] = 0
    loss, _, _ = _run(Xn, Wn, bn, tn)
    assert loss[2] == 35 and np.isnan(loss[0])            # row 5 now counts (label 0 = the first NaN), row 5 no longer as a 3


def test_guard_bands():
    """X, every W, b and the labels in NaN (the labels: out-of-range) guards, dW [50, 128] with a row stride of 132, db, loss and
    the workspace in sentinel guards: finite results equal to the unguarded run bit for bit, every guard word and pad column intact."""
    P, K0, CL, lddw = 200, 152, 50, 132
    Xn, Wn, bn, tn = PC.net(P, K0, CL, 95)
    plain = _run(Xn, Wn, bn, tn)
    tail = 1 << 14
    X = GC.guarded_like(torch.from_numpy(Xn).cuda(), tail, tail)[0]
    Ws = [GC.guarded_like(torch.from_numpy(w).cuda(), tail, tail)[0] for w in Wn]
    bs = [GC.guarded_like(torch.from_numpy(b).cuda(), tail, tail)[0] for b in bn]
    bufs = GC.Bufs(lead=4096, tail=4096)
    target = bufs.lin(torch.from_numpy(tn), CL + 7)         # a stray label read is out of range: a NaN loss
    dW = bufs.mout(CL, 128, lddw)
    db, loss = bufs.fout((CL,)), bufs.fout((4,))
    ws = bufs.fout((_workspace(P, K0, CL),))
    _launch(X, Ws, bs, target, dW, db, loss, ws)
    bufs.intact()
    got = (loss.cpu().numpy().astype(np.float64), dW.cpu().numpy().astype(np.float64), db.cpu().numpy().astype(np.float64))
    for a, b in zip(got, plain):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)


def test_two_launches_give_the_same_bits():
    P, K0, CL = 128 * G + 40, 152, 50
    Xn, Wn, bn, tn = PC.net(P, K0, CL, 96)
    X, target = torch.from_numpy(Xn).cuda(), torch.from_numpy(tn).cuda()
    Ws, bs = [torch.from_numpy(w).cuda() for w in Wn], [torch.from_numpy(b).cuda() for b in bn]
    outs = []
    for fill in (0.0, float("nan")):
        dW, db, loss = torch.full((CL, 128), fill, device="cuda"), torch.full((CL,), fill, device="cuda"), torch.full((4,), fill, device="cuda")
        ws = torch.full((_workspace(P, K0, CL),), fill, device="cuda")
        _launch(X, Ws, bs, target, dW, db, loss, ws)
        outs.append((dW.view(torch.int32).clone(), db.view(torch.int32).clone(), loss.view(torch.int32).clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][0].view(torch.float32)).all())


# ---------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module", params=[False, True], ids=["xyz", "normals"])
def e2e(request):
    """The seeded model and inputs of test_gpu_infer_labels' e2e fixture at B = 2, N = 1024, part labels uniform in [0, 50)."""
    from test_gpu_infer_labels import E2E_SEED, _seeded_model
    from test_gpu_inference import _inputs
    normal = request.param
    net = _seeded_model(normal, E2E_SEED[normal])
    xyz, onehot, start = _inputs(2, 6 if normal else 3, 1024, 11)
    target = torch.randint(0, 50, (2, 1024), generator=torch.Generator().manual_seed(12)).cuda()
    return dict(net=net, xyz=xyz, onehot=onehot, start=start, target=target, normal=normal)


def test_init_classifier_against_the_live_route(e2e):
    """Three init_classifier iterations (augment=False) against three of the live route on a deep copy -- model.eval(), get_loss,
    autograd, torch.optim.SGD(conv2.parameters(), 0.1, momentum=0.5) -- and both against an fp64 trajectory (the frozen
    network's fp64 features of test_gpu_inference._ref64, then tests/probe_common.py).  The bar is the frozen-vs-live bar of
    tests/test_gpu_inference.py for `seg`: |frozen - live| <= 2.0 x the live route's own error against fp64, here on
    conv2.weight / conv2.bias after step 3 (in units of the largest update, max |p_3 - p_0|) and on the three losses.
    Nothing but conv2 moves: every other parameter, every BatchNorm buffer and the trainer's optimizer state keep their bits;
    the frozen form was refreshed at the end.
    The existing constant is the 2.0 of `bar = 2.0 * float((live[k].double().cpu() - ref).abs().max())`.  Measured on an MI355X
    (xyz / normals): conv2.weight 4.7e-6 / 5.07e-6 of the largest update against bars of 1.25e-5 / 1.44e-5; conv2.bias 4.71e-7 /
    1.13e-6 against 2.42e-6 / 4.0e-6; the losses 2.38e-7 / 2.38e-7 (one ulp at 3.9) against 3.6e-7 / 5.71e-7."""
    from prifit_amd import inference
    from prifit_amd.models import pointnet2_part_seg_msg as M
    from prifit_amd.train_step import Trainer
    from test_gpu_inference import _ref64 as net_ref64
    net, xyz, onehot, start, target = (e2e[k] for k in ("net", "xyz", "onehot", "start", "target"))
    live = copy.deepcopy(net)
    p0 = [net.conv2.weight.detach().clone(), net.conv2.bias.detach().clone()]

    tr = Trainer(net)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt_before = copy.deepcopy(tr.optimizer.state_dict())
    home = (net.conv2.weight.data_ptr(), net.conv2.bias.data_ptr())
    # the fourth element pins the sampling: the comparison needs the same start points on both routes
    batch = [(xyz.permute(0, 2, 1).contiguous(), onehot, target, start)]
    hist = tr.init_classifier(batch, epochs=3, augment=False)
    frozen = tr.frozen
    losses = hist["loss"]
    after = net.state_dict()
    for k, v in before.items():
        if k.startswith("conv2."):
            assert not torch.equal(after[k], v), k
        else:
            assert torch.equal(after[k], v), k
    opt_after = tr.optimizer.state_dict()
    assert opt_after["param_groups"] == opt_before["param_groups"] and opt_after["state"].keys() == opt_before["state"].keys()
    for i, st in opt_before["state"].items():
        for name, v in st.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(opt_after["state"][i][name])), (i, name)
    # conv2 still lives in the storage the trainer's optimizer steps
    assert (net.conv2.weight.data_ptr(), net.conv2.bias.data_ptr()) == home
    tr.optimizer._check_storage()
    # the final refresh() happened
    fresh = inference.freeze(net).predict(xyz, onehot, fps_start=start)
    assert torch.equal(frozen.predict(xyz, onehot, fps_start=start), fresh)
    # the accuracy: the count of the arg-max of the LAST iteration's scores is between 0 and 1 and the loss went down
    assert 0.0 <= hist["acc"][-1] <= 1.0 and losses[2] < losses[0]

    # the live route on the copy
    live.eval()
    crit = M.get_loss()
    opt = torch.optim.SGD(live.conv2.parameters(), 0.1, momentum=0.5)
    live_losses = []
    for _ in range(3):
        opt.zero_grad()
        seg = live(xyz, onehot, fps_start=start)[0]
        loss = crit(seg.contiguous().view(-1, 50), target.view(-1))
        loss.backward()
        opt.step()
        live_losses.append(float(loss.detach()))

    # the fp64 trajectory
    a3 = net_ref64(frozen, xyz, onehot, start)[1].permute(0, 2, 1).reshape(-1, 128).numpy()
    sgd = PC.SGD([p0[0].reshape(50, 128).cpu().numpy(), p0[1].cpu().numpy()], 0.1, 0.5)
    ref_losses = []
    tn = target.reshape(-1).cpu().numpy()
    for _ in range(3):
        h = PC.head(a3, sgd.params[0], sgd.params[1], tn)
        ref_losses.append(h["loss"])
        sgd.step([h["dW"], h["db"]])

    for name, mine, theirs, ref, start_p in (("conv2.weight", net.conv2.weight, live.conv2.weight, sgd.params[0], p0[0]),
                                             ("conv2.bias", net.conv2.bias, live.conv2.bias, sgd.params[1], p0[1])):
        mine, theirs = mine.detach().double().cpu().reshape(ref.shape).numpy(), theirs.detach().double().cpu().reshape(ref.shape).numpy()
        upd = float(np.max(np.abs(ref - start_p.double().cpu().reshape(ref.shape).numpy())))
        diff, bar = float(np.max(np.abs(mine - theirs))) / upd, 2.0 * float(np.max(np.abs(theirs - ref))) / upd
        print("init_classifier %s after 3 steps: |frozen - live| %.3g, bar %.3g (2 x the live route's error against fp64), both "
              "relative to the largest update %.3g" % (name, diff, bar, upd))
        assert diff <= bar, name
    diff = max(abs(a - b) for a, b in zip(losses, live_losses))
    bar = 2.0 * max(abs(a - b) for a, b in zip(live_losses, ref_losses))
    print("init_classifier losses %s, live %s: |frozen - live| %.3g, bar %.3g" % (losses, live_losses, diff, bar))
    assert diff <= bar


def test_refusals(e2e):
    from prifit_amd import inference
    net, xyz, onehot, target = e2e["net"], e2e["xyz"], e2e["onehot"], e2e["target"]
    with pytest.raises(NotImplementedError):
        inference.freeze(net, "bf16").probe_step(xyz, onehot, target)
    frozen = inference.freeze(net)
    with pytest.raises(ValueError):
        frozen.probe_step(xyz, onehot, target[:, :1000])
    with pytest.raises(ValueError):
        frozen.probe_step(xyz, onehot, target.int())
    with pytest.raises(ValueError):
        frozen.probe_step(xyz, onehot, target.float())
    with pytest.raises(ValueError):
        frozen.probe_step(xyz[0], onehot, target)

"""GPU: momentum SGD in one launch over the flat parameter buffer (csrc/optim.hip prifit_sgd_flat, prifit_amd/optim.py FlatSGD)
against torch.optim.SGD -- the reference's other optimizer, train_partseg_shapenet.py:260-261 -- and through the trainer."""
import os
import tempfile

import numpy as np
import pytest
import torch

from prifit_amd import synth
from tests_helpers import fit_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(64, 9), (50,), (1,), (128, 64, 1, 1), (7, 3), (33,), (256, 131)]
LATE, NEVER = 4, 5           # first gradient at step 3 / never a gradient

ARMS = {
    "trainer": dict(momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False),
    "nesterov_wd": dict(momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=True),
    "dampening_wd": dict(momentum=0.5, dampening=0.3, weight_decay=1e-4, nesterov=False),     # pins the first-step rule
    "no_momentum_wd": dict(momentum=0.0, dampening=0.0, weight_decay=1e-4, nesterov=False),   # no buffer
    "from_torch_state": dict(momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False),  # continues a torch checkpoint
}


def _params(dt, d):
    return [torch.nn.Parameter(torch.randn(*s, dtype=dt, device=d)) for s in SHAPES]


@pytest.mark.parametrize("arm", list(ARMS))
def test_flat_sgd_matches_torch_sgd(hiplib, arm):
    """The recipe of test_flat_adam_matches_torch_adam: ragged tensor sizes (a length that is no multiple of four, a scalar), a
    parameter that gets its first gradient at step 3 and one that never does, a learning-rate change at step 5, misaligned
    gradient views on odd steps (scalar loads), a step discarded through the device `skip` flag before step 6.  References:
    torch.optim.SGD on the CPU in fp32 and in fp64 on the same gradients; the bar is the fp32 reference's own rounding error."""
    from prifit_amd.optim import FlatSGD
    dev = torch.device("cuda", 0)
    kw = dict(lr=1e-3, **ARMS[arm])
    torch.manual_seed(3)
    ref32 = _params(torch.float32, "cpu")
    ref64 = [torch.nn.Parameter(p.detach().double()) for p in ref32]
    o32, o64 = torch.optim.SGD(ref32, **kw), torch.optim.SGD(ref64, **kw)
    if arm == "from_torch_state":
        # two steps taken by torch (the late parameter has none yet: it comes back with no buffer, so its first step here is a
        # first step), then the flat optimizer continues from torch's state dict
        for _ in range(2):
            gs = [torch.randn(*s) * (0.1 + i) for i, s in enumerate(SHAPES)]
            for i in range(len(SHAPES)):
                has = i not in (NEVER, LATE)
                ref32[i].grad = gs[i].clone() if has else None
                ref64[i].grad = gs[i].double() if has else None
            o32.step()
            o64.step()
    start = [p.detach().clone() for p in ref32]
    mine = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ref32]
    opt = FlatSGD(mine, **kw)
    if arm == "from_torch_state":
        opt.load_state_dict(o32.state_dict())
        assert opt._steps[opt._cur].cpu().tolist() == [0 if i in (NEVER, LATE) else 1 for i in range(len(SHAPES))]
    assert all(p.data_ptr() % 512 == 0 for p in mine)           # every tensor keeps an allocator-like alignment
    assert (opt.momentum_buf is None) == (kw["momentum"] == 0)  # one state buffer, none without momentum
    assert not hasattr(opt, "exp_avg")
    skip = torch.zeros(1, dtype=torch.int32, device=dev)
    for step in range(8):
        if step == 5:
            for o in (o32, o64, opt):
                o.param_groups[0]["lr"] = 2.5e-4
        gs = [torch.randn(*s) * (0.1 + i) for i, s in enumerate(SHAPES)]
        for i in range(len(SHAPES)):
            has = i != NEVER and (i != LATE or step >= 3)
            ref32[i].grad = gs[i].clone() if has else None
            ref64[i].grad = gs[i].double() if has else None
            # odd steps: a gradient that is a misaligned view (scalar loads in the kernel); even steps: its own tensor
            if has and step % 2 == 1 and gs[i].numel() > 1:
                buf = torch.zeros(gs[i].numel() + 1, device=dev)
                buf[1:].copy_(gs[i].reshape(-1))
                mine[i].grad = buf[1:].view(SHAPES[i])
            else:
                mine[i].grad = gs[i].to(dev) if has else None
        if step == 6:       # a discarded step: nothing may change, the buffer and the counters included
            before = [p.detach().clone() for p in mine]
            buf0 = None if opt.momentum_buf is None else opt.momentum_buf.clone()
            cnt0 = opt._steps[opt._cur].clone()
            skip.fill_(1)
            opt.step(skip=skip)
            skip.zero_()
            assert all(torch.equal(a, b) for a, b in zip(before, mine))
            assert buf0 is None or torch.equal(buf0, opt.momentum_buf)
            assert torch.equal(cnt0, opt._steps[opt._cur])
        o32.step()
        o64.step()
        opt.step()
    torch.cuda.synchronize()
    for i, (a, b, c) in enumerate(zip(mine, ref32, ref64)):
        noise = float((b.detach().double() - c.detach()).abs().max())
        err = float((a.detach().cpu().double() - c.detach()).abs().max())
        print("%s tensor %d: err %.3e noise %.3e" % (arm, i, err, noise))
        assert err <= 4 * noise + 1e-7, (i, err, noise)
    assert torch.equal(mine[NEVER].detach().cpu(), start[NEVER])                    # untouched
    sd = opt.state_dict()
    assert NEVER not in sd["state"]
    if kw["momentum"] != 0:
        assert set(sd["state"]) == set(range(len(SHAPES))) - {NEVER}
        ref_state = o32.state_dict()["state"]
        for i, st in sd["state"].items():
            assert set(st) == {"momentum_buffer"} and st["momentum_buffer"].shape == ref32[i].shape
            noise = float((ref_state[i]["momentum_buffer"].double() - o64.state_dict()["state"][i]["momentum_buffer"]).abs().max())
            err = float((st["momentum_buffer"].cpu().double() - o64.state_dict()["state"][i]["momentum_buffer"]).abs().max())
            assert err <= 4 * noise + 1e-7, (i, err, noise)
    else:
        assert sd["state"] == o32.state_dict()["state"]             # what torch writes without momentum
    assert opt.uploads <= 9


def test_flat_sgd_checkpoint_both_ways(hiplib):
    """FlatSGD -> torch.optim.SGD and back through state_dict(): one more step on identical gradients agrees in all three, the
    group's key set is the installed torch's, and a state dict of the other optimizer is refused by name in both classes."""
    from prifit_amd.optim import FlatAdam, FlatSGD
    dev = torch.device("cuda", 0)
    kw = dict(lr=1e-3, momentum=0.9)
    torch.manual_seed(5)
    ref32 = _params(torch.float32, "cpu")
    mine = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ref32]
    o32, opt = torch.optim.SGD(ref32, **kw), FlatSGD(mine, **kw)
    for step in range(3):
        gs = [torch.randn(*s) * (0.1 + i) for i, s in enumerate(SHAPES)]
        for i in range(len(SHAPES)):
            ref32[i].grad = gs[i].clone() if i != NEVER else None
            mine[i].grad = gs[i].to(dev) if i != NEVER else None
        o32.step()
        opt.step()
    sd = opt.state_dict()
    assert set(sd["param_groups"][0]) == set(o32.state_dict()["param_groups"][0])
    assert sd["param_groups"][0]["params"] == list(range(len(SHAPES)))
    for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize", "foreach", "differentiable"):
        assert sd["param_groups"][0][k] == o32.state_dict()["param_groups"][0][k], k
    t2 = torch.optim.SGD([torch.nn.Parameter(p.detach().clone().cpu()) for p in mine], lr=0.5)      # flat -> torch
    t2.load_state_dict(sd)
    fresh = [torch.nn.Parameter(p.detach().clone()) for p in mine]                                  # torch -> flat
    opt2 = FlatSGD(fresh, lr=0.5)
    opt2.load_state_dict(o32.state_dict())
    assert opt2.param_groups[0]["lr"] == 1e-3 and opt2.param_groups[0]["momentum"] == 0.9
    g = [torch.randn(*s) for s in SHAPES]
    for i in range(len(SHAPES)):
        for plist in (fresh, mine):
            plist[i].grad = g[i].to(dev) if i != NEVER else None
        t2.param_groups[0]["params"][i].grad = g[i].clone() if i != NEVER else None
        ref32[i].grad = g[i].clone() if i != NEVER else None
    opt2.step(); opt.step(); t2.step(); o32.step()
    for i in range(len(SHAPES)):
        for other in (fresh[i].detach().cpu(), mine[i].detach().cpu(), t2.param_groups[0]["params"][i].detach()):
            assert torch.allclose(other, ref32[i].detach(), rtol=0, atol=2e-6), i
    # the other optimizer's format: refused up front, the message names both
    adam_sd = torch.optim.Adam([torch.nn.Parameter(torch.zeros(*s)) for s in SHAPES]).state_dict()
    with pytest.raises(ValueError, match=r"torch\.optim\.SGD.*torch\.optim\.Adam"):
        opt2.load_state_dict(adam_sd)
    adam = FlatAdam([torch.nn.Parameter(p.detach().clone()) for p in mine])
    with pytest.raises(ValueError, match=r"torch\.optim\.Adam.*torch\.optim\.SGD"):
        adam.load_state_dict(o32.state_dict())
    with pytest.raises(AssertionError):                     # a gradient list of another length than the parameter list
        opt.step(grads=[None] * (len(SHAPES) - 1))
    with pytest.raises(AssertionError):
        adam.step(grads=[None] * (len(SHAPES) + 1))


def test_sgd_flat_rejects_bad_arguments(hiplib):
    """The entry point itself returns PRIFIT_EINVAL and launches nothing: the parameters stay as they are."""
    from prifit_amd._lib import cur_stream, dll
    dev = torch.device("cuda", 0)
    total = 128
    P = torch.ones(total, device=dev)
    M = torch.zeros(total, device=dev)
    g = torch.ones(8, device=dev)
    G = torch.tensor([g.data_ptr()], dtype=torch.int64, device=dev)
    off = torch.zeros(1, dtype=torch.int32, device=dev)
    ln = torch.full((1,), 8, dtype=torch.int32, device=dev)
    s0, s1 = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    fn = dll().prifit_sgd_flat

    def rc(buf=M, total=total, src=s0, dst=s1, lr=0.1, momentum=0.9, dampening=0.0, wd=0.0, nesterov=0):
        return fn(P.data_ptr(), None if buf is None else buf.data_ptr(), G.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, total,
                  src.data_ptr(), dst.data_ptr(), lr, momentum, dampening, wd, nesterov, None, cur_stream())

    einval = -1                                              # PRIFIT_EINVAL (include/prifit_hip.h)
    assert rc(buf=None, momentum=0.0, nesterov=1) == einval
    assert rc(dampening=0.1, nesterov=1) == einval
    assert rc(dst=s0) == einval
    assert rc(total=6) == einval
    assert rc(buf=None, momentum=0.9) == einval
    assert rc(lr=-0.1) == einval and rc(momentum=-0.5) == einval and rc(wd=-1e-4) == einval
    torch.cuda.synchronize()
    assert torch.equal(P, torch.ones_like(P)) and int(s1.item()) == 0
    # and the same arguments with the fault taken out run: one plain step, p = 1 - 0.1 * 1 on the 8 live floats
    assert rc(buf=None, momentum=0.0) == 0
    torch.cuda.synchronize()
    expect = torch.ones(total)
    expect[:8] = torch.tensor(1.0) - torch.tensor(0.1) * torch.tensor(1.0)
    assert torch.allclose(P.cpu(), expect, rtol=0, atol=1e-7) and torch.equal(P[8:].cpu(), torch.ones(total - 8))
    assert int(s1.item()) == 1


def test_trainer_sgd_steps(hiplib):
    """Trainer(net, optimizer="SGD") (train_partseg_shapenet.py:260-261): the flat optimizer, a supervised and a self-supervised
    step through it, the first step's update p - lr * grad (momentum's fresh buffer IS the gradient), the checkpoint."""
    from prifit_amd.models import pointnet2_part_seg_msg as M
    from prifit_amd.train_step import Trainer
    B, N, lr = 2, 512, 0.001
    torch.manual_seed(4)
    np.random.seed(4)                                        # the trainer draws the model's subset of the cloud from numpy
    net = M.get_model(50)
    synth.xavier_like_trainer(net)
    net.cuda()
    tr = Trainer(net, learning_rate=lr, optimizer="SGD")
    assert type(tr.optimizer).__name__ == "FlatSGD" and tr.optimizer.takes_grads
    g0 = tr.optimizer.param_groups[0]
    assert g0["momentum"] == 0.9 and g0["weight_decay"] == 0 and g0["dampening"] == 0 and not g0["nesterov"]
    captured = []
    real_step = tr.optimizer.step

    def step(*a, **k):
        grads = k["grads"]                                   # the hand-over from FlatGradBucket
        captured.append(([p.detach().clone() for p in tr.optimizer.params],
                         [None if g is None else g.detach().clone() for g in grads]))
        return real_step(*a, **k)

    tr.optimizer.step = step
    pts = torch.from_numpy(synth.cloud("surface", B, N, 5)).cuda()
    target = torch.from_numpy(synth.labels(B, N, 50, 5)).cuda()
    loss, acc = tr.supervised_step(pts, target)
    after = [p.detach().clone() for p in tr.optimizer.params]
    before, grads = captured[0]
    lr32 = float(np.float32(lr))
    stepped = 0
    for i, (p0, g, p1) in enumerate(zip(before, grads, after)):
        if g is None:
            assert torch.equal(p0, p1), i
            continue
        stepped += 1
        # exactly p - lr * grad, rounded once: within half a unit in the last place of the result, measured in fp64 (where the
        # product of two fp32 numbers is exact)
        exact = p0.double() - lr32 * g.double()
        half_ulp = torch.ldexp(torch.ones_like(exact), torch.frexp(p1.double())[1] - 25)
        assert bool(((p1.double() - exact).abs() <= half_ulp * (1 + 1e-9)).all()), i
        assert torch.equal(tr.optimizer._slice(tr.optimizer.momentum_buf, i), g), i        # the fresh buffer is the gradient
    assert stepped >= 100 and torch.isfinite(loss)
    _, cham, _ = fit_inputs(B, N, 128, 4)
    ss = tr.selfsup_step(cham.cuda(), npoint=N, quantile=0.05, msc_iterations=5, max_num_clusters=25)
    tr.finish()
    assert torch.isfinite(ss) and len(captured) == 2
    assert all(torch.isfinite(p).all() for p in net.parameters())
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "model_001.pth")
        tr.save(path)
        net2 = M.get_model(50).cuda()
        tr2 = Trainer(net2, optimizer="SGD")
        tr2.load(path)
        assert type(tr2.optimizer).__name__ == "FlatSGD"
        assert torch.equal(tr2.optimizer.momentum_buf, tr.optimizer.momentum_buf)
        sd, sd2 = tr.optimizer.state_dict()["state"], tr2.optimizer.state_dict()["state"]
        assert set(sd) == set(sd2) and len(sd) >= stepped
        for i in sd:
            assert torch.equal(sd[i]["momentum_buffer"], sd2[i]["momentum_buffer"]), i
        for a, b in zip(net.state_dict().values(), net2.state_dict().values()):
            assert torch.equal(a.cpu(), b.cpu())
    assert type(Trainer(M.get_model(50).cuda()).optimizer).__name__ == "FlatAdam"

"""CPU: the fp64 restatement the probe-head tests measure against (tests/probe_common.py) is pinned to torch -- fp64 autograd
through F.cross_entropy(F.log_softmax(z, 1), t), the reference's get_loss on its network's output, and three steps of
torch.optim.SGD(lr=0.1, momentum=0.5) on the last layer."""
import numpy as np
import torch
import torch.nn.functional as F

import probe_common as PC

REL = 1e-12


def _torch_head(a3, W4, b4, target):
    a3 = torch.from_numpy(a3)
    W = torch.from_numpy(np.asarray(W4, dtype=np.float64)).requires_grad_()
    b = torch.from_numpy(np.asarray(b4, dtype=np.float64)).requires_grad_()
    z = a3 @ W.t() + b
    loss = F.cross_entropy(F.log_softmax(z, dim=1), torch.from_numpy(target))
    loss.backward()
    return float(loss.detach()), W.grad.numpy(), b.grad.numpy(), z.detach()


def _close(got, want, what):
    scale = np.max(np.abs(want))
    assert np.max(np.abs(got - want)) <= REL * scale, (what, float(np.max(np.abs(got - want))), float(scale))


def test_head_against_torch_autograd():
    """P = 200 rows, 37 of them labelled -100; (K0, C_L) = (152, 50) and (64, 33)."""
    for K0, CL, seed in ((152, 50, 1), (64, 33, 2)):
        X, Ws, bs, target = PC.net(200, K0, CL, seed)
        target[np.random.default_rng(seed).choice(200, 37, replace=False)] = PC.IGNORE
        a3 = PC.hidden(X, Ws, bs)
        got = PC.head(a3, Ws[3], bs[3], target)
        loss, dW, db, z = _torch_head(a3, Ws[3], bs[3], target)
        assert got["kept"] == 163
        assert abs(got["loss"] - loss) <= REL * abs(loss)
        _close(got["dW"], dW, "dW")
        _close(got["db"], db, "db")
        keep = target != PC.IGNORE
        assert got["correct"] == int((z.argmax(dim=1).numpy()[keep] == target[keep]).sum())
        # the hidden layers against torch
        a = torch.from_numpy(X.astype(np.float64))
        for W, b in zip(Ws[:3], bs[:3]):
            a = torch.relu(a @ torch.from_numpy(W.astype(np.float64)).t() + torch.from_numpy(b.astype(np.float64)))
        _close(a3, a.numpy(), "a3")


def test_every_row_ignored_is_what_torch_gives():
    """No kept row: torch's loss is NaN (0 / 0) and its gradient all zeros; so is the restatement's."""
    X, Ws, bs, target = PC.net(40, 8, 50, 3)
    target[:] = PC.IGNORE
    a3 = PC.hidden(X, Ws, bs)
    loss, dW, db, _ = _torch_head(a3, Ws[3], bs[3], target)
    assert np.isnan(loss) and not dW.any() and not db.any()
    got = PC.head(a3, Ws[3], bs[3], target)
    assert np.isnan(got["loss"]) and got["kept"] == 0 and got["correct"] == 0
    assert not got["dW"].any() and not got["db"].any()


def test_out_of_range_label_is_nan():
    X, Ws, bs, target = PC.net(40, 8, 50, 4)
    target[7] = 50
    got = PC.probe(X, Ws, bs, target)
    assert np.isnan(got["loss"]) and got["kept"] == 40 and np.isnan(got["dW"]).all() and np.isnan(got["db"]).all()


def test_c_l_one_has_a_zero_gradient():
    X, Ws, bs, target = PC.net(33, 152, 1, 5)
    got = PC.probe(X, Ws, bs, target)
    assert got["loss"] == 0.0 and not got["dW"].any() and not got["db"].any() and got["correct"] == 33


def test_three_sgd_steps_against_torch():
    X, Ws, bs, target = PC.net(129, 64, 33, 6)
    a3 = PC.hidden(X, Ws, bs)
    W = torch.from_numpy(Ws[3].astype(np.float64)).requires_grad_()
    b = torch.from_numpy(bs[3].astype(np.float64)).requires_grad_()
    opt = torch.optim.SGD([W, b], lr=0.1, momentum=0.5)
    sgd = PC.SGD([Ws[3], bs[3]], lr=0.1, momentum=0.5)
    for step in range(3):
        opt.zero_grad()
        loss = F.cross_entropy(F.log_softmax(torch.from_numpy(a3) @ W.t() + b, dim=1), torch.from_numpy(target))
        loss.backward()
        opt.step()
        got = PC.head(a3, sgd.params[0], sgd.params[1], target)
        assert abs(got["loss"] - float(loss.detach())) <= REL * abs(float(loss.detach())), step
        sgd.step([got["dW"], got["db"]])
        _close(sgd.params[0], W.detach().numpy(), "W after step %d" % step)
        _close(sgd.params[1], b.detach().numpy(), "b after step %d" % step)

"""fp64 numpy restatement of the classifier-layer pre-training head (prifit_probe_head_f32, FrozenPartSeg.probe_step): the four
layers of the per-point tail, log_softmax, the cross-entropy on the log-probabilities with torch's label rules, the gradient
of the last layer, the accuracy count and the momentum-SGD update.  Shared by the CPU test that pins it to torch and by the
GPU tests that use it as the reference."""
import numpy as np

IGNORE = -100
GRID = 256          # the kernel's fixed grid: workgroups at most (csrc/probe_head.hip PROBE_GRID)
TILE = 128          # rows of a tile


def hidden(X, Ws, bs):
    """a3 [P, 128]: the first three layers, z_l = W_l a + b_l, a = relu(z_l) (np.maximum: a NaN stays)."""
    a = np.asarray(X, dtype=np.float64)
    for W, b in zip(Ws[:3], bs[:3]):
        a = np.maximum(a @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64), 0.0)
    return a


def log_softmax(z):
    m = np.max(z, axis=1, keepdims=True)
    return z - m - np.log(np.sum(np.exp(z - m), axis=1, keepdims=True))


def first_argmax(z):
    """numpy's order: the first maximum, a NaN beats every number and the first NaN wins."""
    return np.argmax(z, axis=1)


def head(a3, W4, b4, target):
    """The head on a3 [P, 128] -> dict(loss, kept, correct, dW [CL, 128], db [CL], and the sum |.| |.| scales of each:
    loss_scale = mean over the kept rows of |logsumexp(y)| + |y[t]|, dW_scale = |dz|^T |a3|, db_scale = sum |dz|).
    target int64 [P]: -100 drops a row from numerator and denominator; any other label outside [0, CL) makes the loss and that
    row's contribution NaN; no kept row: loss NaN (0 / 0), dW and db zeros (as torch on the CPU)."""
    a3 = np.asarray(a3, dtype=np.float64)
    W4, b4 = np.asarray(W4, dtype=np.float64), np.asarray(b4, dtype=np.float64)
    target = np.asarray(target, dtype=np.int64)
    P, CL = a3.shape[0], W4.shape[0]
    z = a3 @ W4.T + b4
    y = log_softmax(z)
    kept_rows = target != IGNORE
    bad = kept_rows & ((target < 0) | (target >= CL))
    ok = kept_rows & ~bad
    kept = int(kept_rows.sum())
    my = np.max(y, axis=1)
    lse2 = my + np.log(np.sum(np.exp(y - my[:, None]), axis=1))
    tc = np.where(ok, target, 0)
    yt = y[np.arange(P), tc]
    row = np.where(bad, np.nan, lse2 - yt)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float64(row[kept_rows].sum()) / kept
        loss_scale = np.float64((np.abs(lse2) + np.abs(yt))[kept_rows].sum()) / kept
    onehot = np.zeros((P, CL))
    onehot[np.arange(P)[ok], target[ok]] = 1.0
    dz = np.exp(y - lse2[:, None]) - onehot
    dz[bad] = np.nan
    dz[~kept_rows] = 0.0
    den = kept if kept else 1
    dz = dz / den
    correct = int(np.sum(first_argmax(z)[ok] == target[ok]))
    return dict(loss=float(loss), kept=kept, correct=correct, dW=dz.T @ a3, db=dz.sum(axis=0), loss_scale=float(loss_scale),
                dW_scale=np.abs(dz).T @ np.abs(a3), db_scale=np.abs(dz).sum(axis=0), z=z)


def probe(X, Ws, bs, target):
    """The whole entry point on raw rows X [P, K0]."""
    return head(hidden(X, Ws, bs), Ws[3], bs[3], target)


class SGD:
    """torch.optim.SGD(lr, momentum) restated: the first step sets the buffer to the gradient, then buf = momentum buf + g;
    p -= lr buf."""

    def __init__(self, params, lr=0.1, momentum=0.5):
        self.params = [np.array(p, dtype=np.float64) for p in params]
        self.lr, self.momentum = lr, momentum
        self.bufs = None

    def step(self, grads):
        grads = [np.asarray(g, dtype=np.float64) for g in grads]
        self.bufs = [g.copy() for g in grads] if self.bufs is None else [self.momentum * b + g for b, g in zip(self.bufs, grads)]
        self.params = [p - self.lr * b for p, b in zip(self.params, self.bufs)]
        return self.params


def net(P, K0, CL, seed):
    """Seeded normal rows and weights of the tail, drawn as test_gpu_infer_labels._net draws them, plus labels uniform in
    [0, CL): X [P, K0], W (128, 128, 128, CL) rows, b, target int64 [P]."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((P, K0)).astype(np.float32)
    Ws, bs, kin = [], [], K0
    for cout in (128, 128, 128, CL):
        Ws.append((rng.standard_normal((cout, kin)) / np.sqrt(kin)).astype(np.float32))
        bs.append((0.1 * rng.standard_normal(cout)).astype(np.float32))
        kin = cout
    target = rng.integers(0, CL, size=P).astype(np.int64)
    return X, Ws, bs, target

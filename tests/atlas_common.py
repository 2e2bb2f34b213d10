"""Shared by the AtlasNet decoder tests and tools/make_golden_reconstruct.py: the seeded input recipes and an independent
restatement of decoder + reconstruction loss in functional torch (any dtype, CPU), written from the formulas:

  per chart c, shape b, grid point p:   x0 = [u_p, v_p | z_b]                                   (130 values)
    x1 = relu(bn1(W1 x0 + b1)),  x2 = relu(bn2(W2 x1 + b2)),  x3 = relu(bn3(W3 x2 + b3)),  out = tanh(W4 x3 + b4)
  bn in training mode: statistics over the B * P rows of the chart, biased variance to normalise, unbiased variance into
  the running statistics with momentum 0.1; in eval mode the running statistics
  output_points [B, C * P, 3]: chart-major within a shape, grid order within a chart; grid point n = (n % g, n // g) / (g - 1)
  rec = mean over all B * C * P of min_j |o_i - t_j|^2 + mean over all B * N of min_i |o_i - t_j|^2

Nothing here is stored: weights, z and targets come from np.random.default_rng(seed)."""
import numpy as np
import torch

EPS, MOMENTUM = 1e-5, 0.1
WIDTHS = ((130, 130), (65, 130), (32, 65), (3, 32))     # (out, in) of conv1 .. conv4
# (B, num_charts, num_points, seed) of the recorded cases
GOLDEN_CASES = ((2, 3, 128, 11), (3, 2, 9, 12))
GOLDEN_EVAL = (2, 3, 128, 11)
TARGET_N = 70
PARAM_ORDER = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias", "conv4.weight",
               "conv4.bias", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias", "bn3.weight", "bn3.bias")
MODEL_CASE = dict(B=2, N=512, seed=5, decoder_seed=21)


def make_state(seed, C, constant_columns=False):
    """-> {name: float32 array} with AtlasNet's state_dict names (decoder.{i}. ...), every tensor of it"""
    rng = np.random.default_rng(seed)
    sd = {}
    for i in range(C):
        pre = "decoder.%d." % i
        for l, (o, k) in enumerate(WIDTHS, 1):
            sd[pre + "conv%d.weight" % l] = (rng.standard_normal((o, k, 1)) * (1.5 / np.sqrt(k))).astype(np.float32)
            sd[pre + "conv%d.bias" % l] = (0.1 * rng.standard_normal(o)).astype(np.float32)
        for l, (o, _) in enumerate(WIDTHS[:3], 1):
            sd[pre + "bn%d.weight" % l] = (1.0 + 0.2 * rng.standard_normal(o)).astype(np.float32)
            sd[pre + "bn%d.bias" % l] = (0.2 * rng.standard_normal(o)).astype(np.float32)
            sd[pre + "bn%d.running_mean" % l] = (0.3 * rng.standard_normal(o)).astype(np.float32)
            sd[pre + "bn%d.running_var" % l] = (0.5 + rng.random(o)).astype(np.float32)
            sd[pre + "bn%d.num_batches_tracked" % l] = np.array(3 + i + l, np.int64)
        if constant_columns:
            # rows of zeros in a weight + an exactly representable bias: the column entering bn is the same value in every row,
            # its sums are exact in fp32, the variance is exactly 0 and eps alone normalises
            for l, rows in ((1, (0, 7, 129)), (2, (3, 64)), (3, (0, 31))):
                for r in rows:
                    sd[pre + "conv%d.weight" % l][r] = 0.0
                    sd[pre + "conv%d.bias" % l][r] = 0.5 if r % 2 else -0.25
    return sd


def make_inputs(seed, B, N=TARGET_N):
    """-> z [B,128], target [B,N,3] float32"""
    rng = np.random.default_rng(1000 + seed)
    z = rng.standard_normal((B, 128)).astype(np.float32)
    target = (rng.random((B, N, 3)) * 2.0 - 1.0).astype(np.float32)
    return z, target


def grid_of(num_points):
    g = int(np.sqrt(num_points))
    n = np.arange(g * g)
    return np.stack([(n % g).astype(np.float32) / np.float32(g - 1), (n // g).astype(np.float32) / np.float32(g - 1)]), g


def leaves(sd, dtype):
    """-> {name: torch leaf (requires_grad for the trainable ones)}"""
    out = {}
    for k, v in sd.items():
        t = torch.from_numpy(np.array(v))
        if t.dtype == torch.float32:
            t = t.to(dtype)
        if "running" not in k and "num_batches" not in k:
            t.requires_grad_(True)
        out[k] = t
    return out


def _bn(y, w, b, rm, rv, training):
    """y [rows, ch] -> (normalised, new running_mean, new running_var)"""
    if not training:
        return (y - rm) / torch.sqrt(rv + EPS) * w + b, rm, rv
    n = y.shape[0]
    mean = y.mean(dim=0)
    var = ((y - mean) ** 2).mean(dim=0)
    out = (y - mean) / torch.sqrt(var + EPS) * w + b
    with torch.no_grad():
        new_rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
        new_rv = (1 - MOMENTUM) * rv + MOMENTUM * var * n / (n - 1)
    return out, new_rm, new_rv


def decoder(L, z, num_points, C, training=True):
    """L: leaves(...); z [B,128] tensor of the same dtype -> (output_points [B, C * P, 3], {running name: new value})"""
    grid, g = grid_of(num_points)
    P = g * g
    B = z.shape[0]
    uv = torch.from_numpy(grid).to(z.dtype).T                                        # [P,2]
    x0 = torch.cat([uv.unsqueeze(0).expand(B, P, 2), z.unsqueeze(1).expand(B, P, 128)], dim=2).reshape(B * P, 130)
    outs, running = [], {}
    for i in range(C):
        pre = "decoder.%d." % i
        x = x0
        for l in (1, 2, 3):
            y = x @ L[pre + "conv%d.weight" % l][:, :, 0].T + L[pre + "conv%d.bias" % l]
            y, rm, rv = _bn(y, L[pre + "bn%d.weight" % l], L[pre + "bn%d.bias" % l], L[pre + "bn%d.running_mean" % l],
                            L[pre + "bn%d.running_var" % l], training)
            running[pre + "bn%d.running_mean" % l], running[pre + "bn%d.running_var" % l] = rm, rv
            x = torch.relu(y)
        o = torch.tanh(x @ L[pre + "conv4.weight"][:, :, 0].T + L[pre + "conv4.bias"])
        outs.append(o.reshape(B, P, 3))
    return torch.cat(outs, dim=1), running


def rec_loss(out, target):
    """-> (rec, idx_ot [B, C P], idx_to [B, N]): direct differences, nearest neighbours of both sides"""
    d = ((out.unsqueeze(2) - target.unsqueeze(1)) ** 2).sum(dim=3)                  # [B, CP, N]
    m1, i1 = d.min(dim=2)
    m2, i2 = d.min(dim=1)
    return m1.mean() + m2.mean(), i1, i2


def evaluate(sd, z, target, num_points, C, dtype, training=True):
    """One forward + backward of the restatement in `dtype` -> dict of numpy arrays: out, loss, gz, g:<param name>, the new
    running statistics, idx_ot / idx_to."""
    L = leaves(sd, dtype)
    zt = torch.from_numpy(z).to(dtype).requires_grad_(True)
    out, running = decoder(L, zt, num_points, C, training)
    loss, i1, i2 = rec_loss(out, torch.from_numpy(target).to(dtype))
    loss.backward()
    res = {"out": out.detach().numpy(), "loss": loss.detach().numpy(), "gz": zt.grad.numpy(), "idx_ot": i1.numpy(),
           "idx_to": i2.numpy()}
    for k, t in L.items():
        if t.requires_grad:
            res["g:" + k] = t.grad.numpy()
    for k, t in running.items():
        res[k] = t.detach().numpy()
    return res


def grad_moments(res, C):
    """per tensor kind (PARAM_ORDER) and chart: (sum, sum of squares) of the gradient -> [14, C, 2] float64"""
    m = np.zeros((len(PARAM_ORDER), C, 2))
    for a, name in enumerate(PARAM_ORDER):
        for i in range(C):
            g = res["g:decoder.%d.%s" % (i, name)].astype(np.float64)
            m[a, i] = g.sum(), (g * g).sum()
    return m


def model_inputs():
    """The whole-model case: xyz [B,3,N], cls one-hot [B,16] float32"""
    rng = np.random.default_rng(MODEL_CASE["seed"])
    B, N = MODEL_CASE["B"], MODEL_CASE["N"]
    xyz = (rng.random((B, 3, N)) * 2.0 - 1.0).astype(np.float32)
    cls = np.zeros((B, 16), np.float32)
    cls[np.arange(B), rng.integers(0, 16, B)] = 1.0
    return xyz, cls

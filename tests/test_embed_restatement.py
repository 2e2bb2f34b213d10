"""CPU: the fp64 restatement the embedding-chain tests measure against (embed_common.embed64 on folded weights) is the network's
own arithmetic -- F.conv1d + eval-mode F.batch_norm + ReLU for fp1's two layers and conv1 + bn1, extra_conv_emb as a plain
F.conv1d, F.normalize over the channels -- evaluated in float64 on the CPU, folded against unfolded."""
import numpy as np
import torch
import torch.nn.functional as F

import embed_common as EC


def _unfolded(rng, K0):
    """Three (conv, BatchNorm) layers K0 -> 128 -> 128 -> 128 with statistics away from (1, 0, 0, 1), then a plain conv."""
    layers, kin = [], K0
    for _ in range(3):
        layers.append(dict(W=rng.standard_normal((128, kin)) / np.sqrt(kin), b=0.1 * rng.standard_normal(128),
                           gamma=rng.uniform(0.5, 1.5, 128), beta=0.1 * rng.standard_normal(128),
                           mean=0.1 * rng.standard_normal(128), var=rng.uniform(0.5, 1.5, 128), eps=1e-5))
        kin = 128
    We, be = rng.standard_normal((128, 128)) / np.sqrt(128), 0.1 * rng.standard_normal(128)
    return layers, We, be


def _torch_route(X, layers, We, be, normalize):
    """[B, K0, N] channels-first, as the live model runs it."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    x = t(X).t().unsqueeze(0)
    for ly in layers:
        x = F.conv1d(x, t(ly["W"]).unsqueeze(-1), t(ly["b"]))
        x = F.relu(F.batch_norm(x, t(ly["mean"]), t(ly["var"]), t(ly["gamma"]), t(ly["beta"]), training=False, eps=ly["eps"]))
    e = F.conv1d(x, t(We).unsqueeze(-1), t(be))
    if normalize:
        e = F.normalize(e, p=2, dim=1)
    return e[0].t().numpy()


def _folded(layers, We, be):
    Ws, bs = [], []
    for ly in layers:
        W, b = EC.fold64(ly["W"], ly["b"], ly["gamma"], ly["beta"], ly["mean"], ly["var"], ly["eps"])
        Ws.append(W)
        bs.append(b)
    return Ws + [We], bs + [be]


def test_folded_restatement_equals_the_unfolded_network():
    rng = np.random.default_rng(3)
    for K0 in (152, 8):
        layers, We, be = _unfolded(rng, K0)
        X = rng.standard_normal((37, K0))
        Ws, bs = _folded(layers, We, be)
        for normalize in (False, True):
            got, scale = EC.embed64(X, Ws, bs, normalize)
            want = _torch_route(X, layers, We, be, normalize)
            assert got.shape == want.shape == (37, 128) and scale.shape == got.shape and np.all(scale > 0)
            # fp64 on both sides, two orders of the same sums: a few hundred roundings of 1.1e-16 on values of order 1
            assert np.max(np.abs(got - want)) <= 1e-12
            if normalize:
                assert np.max(np.abs(np.sqrt(np.sum(got * got, axis=1)) - 1.0)) <= 1e-14


def test_an_all_zero_row_keeps_eps():
    """Zero weights and biases in the last product: e = 0, and F.normalize divides by max(0, 1e-12) -- zeros, not NaN."""
    rng = np.random.default_rng(4)
    layers, We, be = _unfolded(rng, 16)
    X = rng.standard_normal((5, 16))
    We0, be0 = np.zeros_like(We), np.zeros_like(be)
    Ws, bs = _folded(layers, We0, be0)
    got, scale = EC.embed64(X, Ws, bs, True)
    want = _torch_route(X, layers, We0, be0, True)
    assert np.array_equal(got, np.zeros((5, 128))) and np.array_equal(want, got) and np.all(np.isfinite(scale))
    # a row of norm 1e-13, below eps, is divided by eps and not by its norm
    be1 = np.zeros(128)
    be1[7] = 1e-13
    Ws, bs = _folded(layers, We0, be1)
    got = EC.embed64(X, Ws, bs, True)[0]
    want = _torch_route(X, layers, We0, be1, True)
    assert np.allclose(got[:, 7], 0.1, rtol=1e-12, atol=0) and np.max(np.abs(got - want)) <= 1e-15
    e, n = EC.normalize64(np.array([[3.0, 4.0]]))
    assert np.array_equal(n, [[5.0]]) and np.allclose(e, [[0.6, 0.8]], rtol=1e-15, atol=0)


def test_the_integer_net_and_the_bound_helpers():
    """The helpers the GPU tests lean on: the integer net's stated magnitudes and a bound that is positive and grows with E."""
    for K0, CL in EC.CASES:
        X, Ws, bs, a3, z, e = EC.int_net(7, K0, CL)
        assert a3.max() <= 31 and np.abs(e).max() <= 63 and (z is None) == (CL == 0)
        assert int(np.sum(e.astype(np.int64) ** 2, axis=1).max()) < 2 ** 24
    Xn, Wn, bn = EC.seeded_net(9, 24, 5, 1)
    assert [None if w is None else w.shape for w in Wn] == [(128, 24), (128, 128), (128, 128), (5, 128), (128, 128)]
    assert EC.seeded_net(9, 24, 0, 1)[1][3] is None
    main = [Wn[i] for i in (0, 1, 2, 4)], [bn[i] for i in (0, 1, 2, 4)]
    z, E = EC.chain64(Xn, *main)
    ref = EC.embed64(Xn, *main, False)[0]
    assert np.max(np.abs(z - ref)) <= 1e-13 and np.all(E > 0)
    e32 = z.astype(np.float32)
    en, bound = EC.normalize_f32_bound(e32.astype(np.float64))
    s = np.sum(e32 * e32, axis=1, keepdims=True, dtype=np.float32)
    assert np.all(np.abs((e32 / np.maximum(np.sqrt(s), np.float32(1e-12))).astype(np.float64) - en) <= bound)

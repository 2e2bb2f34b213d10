"""The mean-shift kernels with every input inside NaN guard bands and every output inside sentinel guards
(tests/guard_common.py), against a plain float64 computation of src/mean_shift.py:61-82 and :138-160.

Each case asserts, in this order:
  1. every output is finite (a read past the extent a kernel owns returns NaN, and `fma(0, NaN, acc)` is NaN);
  2. every guard word still holds its pattern (no stray write, inputs not written);
  3. every output is within a bar of the fp64 result.
Finiteness, guard integrity and the documented fallback of the row-sparse backward (modes 1 and 2 run mode 0 above 16
iterations: the same bits) are exact.  The bars are relative to the largest magnitude of the fp64 quantity, set at a small
multiple of the fp32 error measured on non-ragged control shapes (BAR below, the measured value next to each)."""
import ctypes

import numpy as np
import pytest
import torch

from guard_common import SENTINEL, assert_guards_intact, guarded, guarded_like, padded_stream, x_tail
from prifit_amd import synth

pytestmark = pytest.mark.gpu

LL = ctypes.c_longlong
NAN = float("nan")

# max |fp32 - fp64| / max |fp64| per quantity: 4x the error measured on an MI355X on the non-ragged control (rounded up), the
# measurement in the comment.  Controls: rows -- test_row_sparse_backward_control_finite_guards (N = 2048, T = 10); dense --
# N = 2048, D = 128; fused -- N = 576 (whole 64-query blocks), first update -- N = 2048; q = 0.01 -- its own N = 2048 case.
BAR = {
    "centres": 3e-6,       # 7.2e-7 (all cases: <= 1.4e-6)
    "dX_rows": 6e-6,       # 1.36e-6 (<= 2.5e-6)
    "Z_dense": 6e-6,       # 1.46e-6 (<= 2.0e-6)
    "dX_dense": 1.1e-5,    # 2.59e-6 (<= 2.7e-6)
    "KT": 8e-6,            # 1.84e-6 (<= 1.9e-6)
    "O": 5e-6,             # 6.2e-7; first update 1.08e-6 (<= 1.1e-6)
    "rowsum": 3e-6,        # 3.5e-7; first update 6.0e-7 (<= 6.7e-7)
    "Zn": 6e-6,            # 6.1e-7; first update 1.30e-6 (<= 1.3e-6)
    "nrm": 6e-6,           # 1.22e-6; first update 1.27e-6 (<= 1.3e-6)
    "gST": 8e-6,           # 1.83e-6 (<= 1.8e-6)
    "dZ": 2e-6,            # 3.9e-7 (<= 6.6e-7)
    "dX_fused": 4e-6,      # 8.9e-7 (<= 1.7e-6)
    "bw": 9e-7,            # 2.2e-7
    "centres_q01": 1.8e-5,  # 4.3e-6 (20 iterations, b = 0.145, 87 % of the kernel values on the exp(-13) floor)
    "dX_q01": 5e-5,        # 1.18e-5
}


@pytest.fixture(scope="module")
def F(hiplib):
    assert torch.cuda.is_available()
    from prifit_amd import fit_ops
    return fit_ops


def rel(a, ref):
    """max |a - ref| / max |ref|"""
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


def check(name, a, ref, report):
    report[name] = rel(a, ref)
    print("%-12s %.3e  (bar %.1e)" % (name, report[name], BAR[name.split(":")[0]]))


def assert_bars(report):
    bad = {k: v for k, v in report.items() if not v <= BAR[k.split(":")[0]]}
    assert not bad, bad


def clustered(B, N, D, seed, nproto=6, noise=0.15):
    """Unit rows around a few prototypes, so that kernel values span the clamp."""
    gen = torch.Generator().manual_seed(seed)
    proto = torch.nn.functional.normalize(torch.randn(nproto, D, generator=gen), dim=1)
    X = proto[torch.randint(0, nproto, (B, N), generator=gen)] + noise * torch.randn(B, N, D, generator=gen)
    return torch.nn.functional.normalize(X, dim=2)


def ms64(X, bw, T):
    """src/mean_shift.py:61-82 (gaussian kernel, delta = 1) in float64: Z_0 = X, Z <- normalize(Z + (K X / rowsum - Z)),
    K = exp(clamp((Z X^T - 1) / b^2, -13, 75)).  X [B,N,D] float64; autograd through it when X requires grad."""
    b2 = (bw.double() ** 2).view(-1, 1, 1)
    Z = X
    for _ in range(T):
        K = torch.exp(torch.clamp((Z @ X.transpose(1, 2) - 1.0) / b2, -13.0, 75.0))
        new = Z + (K @ X / K.sum(-1, keepdim=True) - Z)
        Z = new / new.norm(dim=-1, keepdim=True)
    return Z


def bandwidth64(X, quantile):
    """src/mean_shift.py:138-160 over all rows in float64: mean over rows of sqrt(max(k-th smallest chord, 1e-6))."""
    X = X.double()
    k = int(quantile * X.shape[1])
    dist = 2.0 - 2.0 * X @ X.transpose(1, 2)
    kth = torch.topk(dist, k, dim=2, largest=False)[0][..., -1]
    return torch.sqrt(kth.clamp(min=1e-6)).mean(1)


def gather_rows(Z, ids):
    return torch.gather(Z, 1, ids.unsqueeze(-1).expand(-1, -1, Z.shape[2]))


def guarded_x(X, poison=NAN):
    D = X.shape[-1]
    return guarded_like(X.cuda(), x_tail(D), x_tail(D), poison)


def rows_problem(B, N, D, R, nrows, seed):
    gen = torch.Generator().manual_seed(seed)
    X = clustered(B, N, D, seed)
    bw = torch.tensor([0.35, 0.5, 0.8][:B]).cuda() if B <= 3 else torch.linspace(0.35, 0.8, B).cuda()
    ids = torch.stack([torch.randperm(N, generator=gen)[:R] for _ in range(B)]).cuda()
    nr = torch.tensor(nrows, dtype=torch.int32).cuda()
    G = torch.randn(B, R, D, generator=gen).cuda()
    live = (torch.arange(R, device="cuda").view(1, R) < nr.view(B, 1).long()).unsqueeze(-1).float()
    return X, bw, ids, nr, G, live


def rows_ref64(X, bw, ids, G, live, T):
    X64 = X.cuda().double().requires_grad_(True)
    c64 = gather_rows(ms64(X64, bw, T), ids)
    (c64 * (G * live).double()).sum().backward()
    return c64.detach(), X64.grad


def rows_run(F, X, bw, ids, nr, G, T, mode, monkeypatch, poison=NAN):
    """MeanShiftRowsFn with X inside guards, the mode forced -> (centres, dX); X's guards checked."""
    Xg, base = guarded_x(X, poison)
    Xg = Xg.detach().requires_grad_(True)
    monkeypatch.setattr(F, "MS_ROWS_MODE", str(mode))
    with torch.no_grad():
        _, traj = F.mean_shift_trajectory(Xg.detach(), bw, T, keep_kernel=False)
    c = F.MeanShiftRowsFn.apply(Xg, bw, ids, nr, traj)
    (c * G).sum().backward()
    torch.cuda.synchronize()
    assert_guards_intact(base, Xg, poison)
    return c.detach(), Xg.grad


# (N, D, T, R, live rows per shape): each axis covered -- N 2048 / 2088 = 2048 + 40 / 300 / 1500, D 128 / 64 / 32, T 1 / 10 / 16 /
# 17 / 20, 32 and 64 slots, live counts 0 and full, the ragged shape last in a batch of three (its X ends at the guard), B = 1
ROWS_CASES = [
    (2048, 128, 10, 32, (8, 1, 32)),
    (2088, 128, 10, 32, (32, 0, 5)),
    (300, 128, 16, 32, (4, 7, 3)),
    (1500, 64, 1, 32, (0, 32, 2)),
    (2088, 64, 10, 32, (3, 6, 0)),
    (300, 32, 10, 32, (2, 2, 32)),
    (2088, 32, 17, 32, (3, 3, 3)),
    (2048, 128, 20, 32, (5, 2, 8)),
    (300, 64, 20, 64, (40, 0, 64)),
    (1500, 32, 10, 64, (64, 2, 33)),
    (2088, 128, 4, 64, (1, 64, 9)),
    (2088, 128, 3, 32, (6,)),
]


@pytest.mark.parametrize("N,D,T,R,nrows", ROWS_CASES)
def test_row_sparse_backward_in_guards_against_fp64(F, N, D, T, R, nrows, monkeypatch):
    """MeanShiftRowsFn in all three modes (prifit_meanshift_rows_bwd `mode`), X in NaN guards: centres and dX against fp64
    autograd of the dense iteration followed by the gather.  Modes 0 and 1 give the same bits; above TCAP = 16 iterations
    modes 1 and 2 ARE mode 0 (the documented fallback): the same bits."""
    B = len(nrows)
    X, bw, ids, nr, G, live = rows_problem(B, N, D, R, nrows, N + D + T + R)
    c64, dX64 = rows_ref64(X, bw, ids, G, live, T)
    got, report = {}, {}
    for mode in (0, 1, 2):
        c, dX = rows_run(F, X, bw, ids, nr, G, T, mode, monkeypatch)
        got[mode] = dX
        check("centres:%d" % mode, c * live, c64 * live, report)
        check("dX_rows:%d" % mode, dX, dX64, report)
        assert torch.isfinite(c).all() and torch.isfinite(dX).all(), "mode %d: non-finite output" % mode
    assert torch.equal(got[0], got[1])
    if T > 16:
        assert torch.equal(got[1], got[0]) and torch.equal(got[2], got[0])
    assert_bars(report)


def test_row_sparse_backward_control_finite_guards(F, monkeypatch):
    """The control of the bars above: N = 2048, D = 128, T = 10, guards holding a finite value (zeros), every mode."""
    X, bw, ids, nr, G, live = rows_problem(3, 2048, 128, 32, (8, 1, 32), 77)
    c64, dX64 = rows_ref64(X, bw, ids, G, live, 10)
    report = {}
    for mode in (0, 1, 2):
        c, dX = rows_run(F, X, bw, ids, nr, G, 10, mode, monkeypatch, poison=0.0)
        check("centres:%d" % mode, c * live, c64 * live, report)
        check("dX_rows:%d" % mode, dX, dX64, report)
    assert_bars(report)


def test_row_sparse_backward_abi_output_guards(F):
    """prifit_meanshift_rows_bwd called directly, dX and the workspace inside sentinel guards: no word outside them written,
    dX (accumulated onto zeros) finite and equal to the autograd path's, in every mode."""
    from prifit_amd._lib import call, cur_stream, ptr, query
    B, N, D, T, R = 3, 2088, 128, 10, 32
    X, bw, ids, nr, G, live = rows_problem(B, N, D, R, (4, 9, 32), 5)
    Xg, xbase = guarded_x(X)
    with torch.no_grad():
        _, traj = F.mean_shift_trajectory(Xg, bw, T, keep_kernel=False)
    arr = lambda k: (ctypes.c_void_p * T)(*[it[k].data_ptr() for it in traj])
    nws = query("prifit_meanshift_rows_bwd_workspace", B, N, D, R, T)
    c64, dX64 = rows_ref64(X, bw, ids, G, live, T)
    report = {}
    for mode in (0, 1, 2):
        ws, wbase = guarded((nws,), 4096, 65536, SENTINEL)
        dX, dbase = guarded((B, N, D), 4096, x_tail(D), SENTINEL)
        dX.zero_()
        call("prifit_meanshift_rows_bwd", ptr(Xg), ptr(bw), B, N, D, T, arr(0), arr(4), arr(2), arr(3), arr(5), ptr(ids), ptr(nr),
             R, ptr(G.contiguous()), ptr(ws), ptr(dX), mode, cur_stream())
        torch.cuda.synchronize()
        assert_guards_intact(wbase, ws)
        assert_guards_intact(dbase, dX)
        check("dX_rows:%d" % mode, dX, dX64, report)
        assert torch.isfinite(dX).all(), "mode %d: non-finite dX" % mode
    assert_guards_intact(xbase, Xg, NAN)
    assert_bars(report)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(200, 128), (333, 128), (2080, 128), (2088, 128), (333, 64), (2088, 64), (200, 32), (2088, 32),
                                 (2048, 128)])
def test_dense_engine_in_guards_against_fp64(F, N, D):
    """MeanShiftFn forward + backward (D = 128: the fused kernels, the hybrid backward where N % 32 == 0, the GEMM chain
    otherwise; D = 32 / 64: the GEMM chain), X in NaN guards, a gradient on every row: end points and dX against fp64."""
    B, T = 3, 3
    X = clustered(B, N, D, N + D)
    bw = torch.tensor([0.35, 0.5, 0.8]).cuda()
    G = torch.randn(B, N, D, generator=torch.Generator().manual_seed(N)).cuda()
    X64 = X.cuda().double().requires_grad_(True)
    Z64 = ms64(X64, bw, T)
    (Z64 * G.double()).sum().backward()
    Xg, base = guarded_x(X)
    Xg = Xg.detach().requires_grad_(True)
    Z = F.MeanShiftFn.apply(Xg, bw, T)
    (Z * G).sum().backward()
    torch.cuda.synchronize()
    report = {}
    check("Z_dense", Z.detach(), Z64.detach(), report)
    check("dX_dense", Xg.grad, X64.grad, report)
    assert torch.isfinite(Z).all() and torch.isfinite(Xg.grad).all()
    assert_guards_intact(base, Xg, NAN)
    assert_bars(report)


# ---------------------------------------------------------------------------------------------------------------------------
def round_up(n, m):
    return (n + m - 1) // m * m


def fused_problem(B, N, seed):
    D = 128
    gen = torch.Generator().manual_seed(seed)
    X = clustered(B, N, D, seed)
    Z = torch.nn.functional.normalize(X + 0.05 * torch.randn(B, N, D, generator=gen), dim=2)
    bw = torch.linspace(0.35, 0.8, B)
    gO = torch.randn(B, N, D, generator=gen)
    grs = torch.randn(B, N, generator=gen)
    return X.cuda(), Z.cuda(), bw.cuda(), gO.cuda(), grs.cuda()


def fused_ref64(X, Z, bw, gO, grs):
    """One update and its backward pieces in fp64: K [B,q,k], O, rowsum, Zn, nrm, gS [B,q,k] (zero where the lower clamp is
    active), the exponent E."""
    X, Z, gO, grs = X.double(), Z.double(), gO.double(), grs.double()
    b2 = (bw.double() ** 2).view(-1, 1, 1)
    E = (Z @ X.transpose(1, 2) - 1.0) / b2
    K = torch.exp(E.clamp(-13.0, 75.0))
    O = K @ X
    rs = K.sum(-1)
    new = Z + (O / rs.unsqueeze(-1) - Z)
    nrm = new.norm(dim=-1)
    gS = (gO @ X.transpose(1, 2) + grs.unsqueeze(-1)) * K / b2 * (E > -13.0)
    return dict(E=E, K=K, O=O, rowsum=rs, Zn=new / nrm.unsqueeze(-1), nrm=nrm, gS=gS)


def out_guarded(shape):
    return guarded(shape, 4096, 65536, SENTINEL)


def fwd_outputs(B, N, D):
    outs = {k: out_guarded(s) for k, s in (("Zn", (B, N, D)), ("O", (B, N, D)), ("rowsum", (B, N)), ("nrm", (B, N)))}
    return outs


def check_fwd_outputs(outs, ref, report):
    for k, (v, base) in outs.items():
        assert torch.isfinite(v).all(), k
        assert_guards_intact(base, v)
        check(k, v, ref[k], report)


def near_gate(E):
    """Elements within 1e-4 of the lower clamp, where fp32 rounding decides the gate of gS: left out of the gS^T comparison."""
    return (E + 13.0).abs() < 1e-4


@pytest.mark.parametrize("N", [576, 200, 2088])
def test_fused_kernels_padded_streams_against_fp64(hiplib, N):
    """prifit_meanshift_fused_fwd writing K^T into a padded stream (ld_kt = round_up(N, 4) + 64, a gap between shapes), then
    prifit_meanshift_fused_bwd_dz reading that K^T with its NaN-pattern pad (balanced 0 and 1) and writing gS^T into another
    padded stream, then prifit_meanshift_fused_bwd_dx: all inputs in NaN guards, all outputs in sentinel guards, against fp64.
    N = 576: whole 64-query blocks (the exact-tile form, scalar offsets); 200, 2088: ragged (lane-offset bounds checks)."""
    from prifit_amd._lib import call, cur_stream, ptr
    B, D = 3, 128
    X, Z, bw, gO, grs = fused_problem(B, N, N)
    ref = fused_ref64(X, Z, bw, gO, grs)
    (Xg, xb), (Zg, zb), (gOg, gb), (grsg, rb) = (guarded_x(t) for t in (X, Z, gO, grs))
    ld = round_up(N, 4) + 64
    stride = N * ld + 128
    KT, ktb = padded_stream(B, N, ld, stride, SENTINEL)
    outs = fwd_outputs(B, N, D)
    call("prifit_meanshift_fused_fwd", ptr(Zg), ptr(Xg), ptr(bw), B, N, D, ptr(KT), LL(ld), LL(stride), ptr(outs["Zn"][0]),
         ptr(outs["O"][0]), ptr(outs["rowsum"][0]), ptr(outs["nrm"][0]), cur_stream())
    torch.cuda.synchronize()
    report = {}
    kt = KT[..., :N]
    assert torch.isfinite(kt).all()
    assert_guards_intact(ktb, kt)
    check("KT", kt, ref["K"].transpose(1, 2), report)
    check_fwd_outputs(outs, ref, report)

    keep = ~near_gate(ref["E"]).transpose(1, 2)
    gST64 = ref["gS"].transpose(1, 2)
    for bal in (0, 1):
        gST, gsb = padded_stream(B, N, ld, stride, SENTINEL)
        dZ, dzb = out_guarded((B, N, D))
        dZ.zero_()
        call("prifit_meanshift_fused_bwd_dz", ptr(gOg), LL(N * D), ptr(Xg), ptr(bw), ptr(grsg), ptr(KT), LL(ld), LL(stride),
             ptr(gST), B, N, D, ptr(dZ), bal, cur_stream())
        torch.cuda.synchronize()
        gs = gST[..., :N]
        assert torch.isfinite(gs).all() and torch.isfinite(dZ).all(), bal
        assert_guards_intact(gsb, gs)
        assert_guards_intact(dzb, dZ)
        check("gST:%d" % bal, gs * keep, gST64 * keep, report)
        check("dZ:%d" % bal, dZ, ref["gS"] @ X.double(), report)
    if N % 4 == 0:
        dX, dxb = out_guarded((B, N, D))
        dX.zero_()
        call("prifit_meanshift_fused_bwd_dx", ptr(gOg), ptr(Zg), ptr(Xg), ptr(bw), ptr(grsg), ptr(KT), LL(ld), LL(stride), B, N,
             D, ptr(dX), cur_stream())
        torch.cuda.synchronize()
        assert torch.isfinite(dX).all()
        assert_guards_intact(dxb, dX)
        dX64 = ref["gS"].transpose(1, 2) @ Z.double() + ref["K"].transpose(1, 2) @ gO.double()
        check("dX_fused", dX, dX64, report)
    for t, b in ((Xg, xb), (Zg, zb), (gOg, gb), (grsg, rb)):
        assert_guards_intact(b, t, NAN)
    assert_guards_intact(ktb, kt)                  # read, not written, by the backward kernels
    assert_bars(report)


def test_fused_bwd_dz_stream_k_padded_streams(hiplib):
    """The stream-K schedule of prifit_meanshift_fused_bwd_dz (B x N / 64 = 560 query blocks > 512 resident slots, not a
    multiple: split query blocks add halves into dZ) reading a padded, poisoned K^T: gS^T and dZ against fp64."""
    from prifit_amd._lib import call, cur_stream, ptr
    B, N, D = 35, 1024, 128
    X, Z, bw, gO, grs = fused_problem(B, N, 9)
    ref = fused_ref64(X, Z, bw, gO, grs)
    (Xg, xb), (gOg, gb), (grsg, rb) = (guarded_x(t) for t in (X, gO, grs))
    ld, stride = N + 64, N * (N + 64) + 128
    KT, ktb = padded_stream(B, N, ld, stride, NAN)
    KT[..., :N] = ref["K"].transpose(1, 2).float()
    del ref["K"], ref["O"]
    gST, gsb = padded_stream(B, N, ld, stride, SENTINEL)
    dZ, dzb = out_guarded((B, N, D))
    dZ.zero_()
    call("prifit_meanshift_fused_bwd_dz", ptr(gOg), LL(N * D), ptr(Xg), ptr(bw), ptr(grsg), ptr(KT), LL(ld), LL(stride),
         ptr(gST), B, N, D, ptr(dZ), 1, cur_stream())
    torch.cuda.synchronize()
    gs = gST[..., :N]
    assert torch.isfinite(gs).all() and torch.isfinite(dZ).all()
    assert_guards_intact(gsb, gs)
    assert_guards_intact(dzb, dZ)
    for t, b in ((KT[..., :N], ktb), (Xg, xb), (gOg, gb), (grsg, rb)):
        assert_guards_intact(b, t, NAN)
    report = {}
    keep = ~near_gate(ref["E"]).transpose(1, 2)
    check("gST:sk", gs * keep, ref["gS"].transpose(1, 2) * keep, report)
    check("dZ:sk", dZ, ref["gS"] @ X.double(), report)
    assert_bars(report)


@pytest.mark.parametrize("N", [576, 2048])
def test_fused_first_fwd_padded_chord_against_fp64(hiplib, N):
    """prifit_meanshift_fused_first_fwd (the first update from the chord matrix 2 - 2 X X^T) reading a padded chord matrix
    whose pad columns and inter-shape gap hold NaN; N = 576 is whole 64-row blocks but not whole 256-row ones."""
    from prifit_amd._lib import call, cur_stream, ptr
    B, D = 3, 128
    X = clustered(B, N, D, N + 1).cuda()
    bw = torch.tensor([0.35, 0.5, 0.8]).cuda()
    ref = fused_ref64(X, X, bw, torch.zeros_like(X), torch.zeros(B, N, device="cuda"))
    Xg, xb = guarded_x(X)
    ld, stride = N + 64, N * (N + 64) + 128
    C, cb = padded_stream(B, N, ld, stride, NAN)
    C[..., :N] = (2.0 - 2.0 * X.double() @ X.double().transpose(1, 2)).float()
    outs = fwd_outputs(B, N, D)
    call("prifit_meanshift_fused_first_fwd", ptr(Xg), ptr(C), LL(ld), LL(stride), ptr(bw), B, N, D, ptr(outs["Zn"][0]),
         ptr(outs["O"][0]), ptr(outs["rowsum"][0]), ptr(outs["nrm"][0]), cur_stream())
    torch.cuda.synchronize()
    report = {}
    check_fwd_outputs(outs, ref, report)
    assert_guards_intact(cb, C[..., :N], NAN)
    assert_guards_intact(xb, Xg, NAN)
    assert_bars(report)


# ---------------------------------------------------------------------------------------------------------------------------
def test_reference_defaults_quantile_001_twenty_iterations(F):
    """The reference trainer's defaults, --quantile 0.01 --msc_iterations 20, on a clustered embedding at B = 3, N = 2048,
    D = 128: fit_ops.compute_bandwidth -> mean_shift_trajectory (first update from the chord matrix) -> MeanShiftRowsFn (20 >
    16 iterations: the per-iteration launches), X in NaN guards.  Bandwidth against fp64; centres and dX against fp64
    iterations at the kernel's bandwidth (so that they measure the iterations, not the bandwidth's last bit)."""
    B, N, D, T, R = 3, 2048, 128, 20, 32
    cham, lab = synth.blobs_with_labels(B, 5000, 31)
    sel = np.random.default_rng(32).choice(5000, N, replace=False)
    X = torch.from_numpy(synth.prototype_embedding(lab[:, sel], D, 33, noise=0.01)).float().cuda()
    gen = torch.Generator().manual_seed(34)
    ids = torch.stack([torch.randperm(N, generator=gen)[:R] for _ in range(B)]).cuda()
    nr = torch.tensor([25, 8, 32], dtype=torch.int32).cuda()
    G = torch.randn(B, R, D, generator=gen).cuda()
    live = (torch.arange(R, device="cuda").view(1, R) < nr.view(B, 1).long()).unsqueeze(-1).float()

    Xg, base = guarded_x(X)
    Xg = Xg.detach().requires_grad_(True)
    keep = []
    bw = F.compute_bandwidth(Xg.detach(), 0.01, keep_chord=keep)
    with torch.no_grad():
        _, traj = F.mean_shift_trajectory(Xg.detach(), bw, T, keep_kernel=False, chord=keep[0])
    c = F.MeanShiftRowsFn.apply(Xg, bw, ids, nr, traj)
    (c * G).sum().backward()
    torch.cuda.synchronize()

    report = {}
    check("bw", bw, bandwidth64(X, 0.01), report)
    c64, dX64 = rows_ref64(X, bw, ids, G, live, T)
    check("centres_q01", c.detach() * live, c64 * live, report)
    check("dX_q01", Xg.grad, dX64, report)
    with torch.no_grad():                                   # the clamp census of the fp64 iterations
        X64, Z64, b2 = X.double(), X.double(), (bw.double() ** 2).view(-1, 1, 1)
        floor = 0
        for _ in range(T):
            E = (Z64 @ X64.transpose(1, 2) - 1.0) / b2
            floor += int((E <= -13.0).sum())
            K = torch.exp(E.clamp(-13.0, 75.0))
            new = Z64 + (K @ X64 / K.sum(-1, keepdim=True) - Z64)
            Z64 = new / new.norm(dim=-1, keepdim=True)
    print("bandwidth %s; kernel values on the exp(-13) floor: %.1f %%" % (bw.tolist(), 100.0 * floor / (T * B * N * N)))
    assert torch.isfinite(bw).all() and torch.isfinite(c).all() and torch.isfinite(Xg.grad).all()
    assert_guards_intact(base, Xg, NAN)
    assert_bars(report)

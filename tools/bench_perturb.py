"""The per-point augmentation kernel (ops.perturb_points, csrc/perturb.hip) at the training batch sizes: B 24, M 2048 and 5000, C 3
and 6, tables already on the device.  Arms per shape:
  affine    the per-shape map alone (with C = 6 the normals rotated too), out of place: what `ops.affine_points` does for xyz;
  full      map + jitter (sigma 0.01, clip 0.05) + dropout (ratio 0.4), out of place;
  inplace   the same in place: with dropout one workgroup per shape (the header says why);
  torch     the same law as torch operators (matmul per shape, randn, clamp, rand, where): what a caller would write without it.
Per arm, medians over the timed calls:
  gpu_us    device events around ONE call enqueued behind a few ms of other work (the events bracket the kernels, not the enqueue);
  chain_us  device events around 50 calls back to back, divided by 50 (launch gaps overlap: the sustained cost per call);
  gbps      algorithmic bytes (the batch read once and written once, 8 * B * M * C) over chain_us.
usage (GPU box): python tools/bench_perturb.py [timed calls, default 100]  -> one JSON line"""
import json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prifit_amd import ops, provider

steps = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 100
assert torch.cuda.is_available(), "bench_perturb.py times a GPU: no CPU path"
B, CHAIN = 24, 50
dev = torch.device("cuda", 0)
np.random.seed(0), torch.manual_seed(0)
aff = provider.compose_affine(y_angle=np.random.uniform(0, 2 * np.pi, B))      # rotations: the in-place arm keeps its magnitudes
aff_dev = torch.from_numpy(aff).to(dev)
ratio_dev = torch.full((B,), 0.4, device=dev)
A_dev = aff_dev[:, :9].reshape(B, 3, 3).contiguous()
busy = torch.randn(4096, 4096, device=dev)


def torch_arm(x, C):
    out = x.clone()
    out[:, :, 0:3] = torch.bmm(x[:, :, 0:3], A_dev) + aff_dev[:, 9:].reshape(B, 1, 3)
    if C == 6:
        out[:, :, 3:6] = torch.bmm(x[:, :, 3:6], A_dev)
    out[:, :, 0:3] += (0.01 * torch.randn(B, x.shape[1], 3, device=dev)).clamp_(-0.05, 0.05)
    drop = torch.rand(B, x.shape[1], device=dev) <= ratio_dev.reshape(B, 1)
    return torch.where(drop.unsqueeze(2), out[:, 0:1, :], out)


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    one, chain = [], []
    for _ in range(steps):
        for _ in range(3):
            torch.mm(busy, busy)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        one.append(e0.elapsed_time(e1) * 1e3)
    for _ in range(max(5, steps // 10)):
        for _ in range(3):
            torch.mm(busy, busy)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CHAIN):
            fn()
        e1.record()
        torch.cuda.synchronize()
        chain.append(e0.elapsed_time(e1) * 1e3 / CHAIN)
    return statistics.median(one), statistics.median(chain)


res = {"tool": "bench_perturb", "B": B, "steps": steps, "chain": CHAIN, "torch_version": torch.__version__,
       "device": torch.cuda.get_device_name(0), "shapes": {}}
for M in (2048, 5000):
    for C in (3, 6):
        x = torch.from_numpy(np.random.default_rng(M + C).uniform(-1, 1, (B, M, C)).astype(np.float32)).to(dev)
        out, work = torch.empty_like(x), x.clone()
        full = dict(rotate_normals=C == 6, sigma=0.01, clip=0.05, drop_ratio=ratio_dev, seed=7)
        arms = {
            "affine": lambda: ops.perturb_points(x, aff_dev, rotate_normals=C == 6, out=out),
            "full": lambda: ops.perturb_points(x, aff_dev, out=out, **full),
            "inplace": lambda: ops.perturb_points(work, aff_dev, out=work, **full),
            "torch": lambda: torch_arm(x, C),
        }
        row = {}
        for k, fn in arms.items():
            one, chain = timed(fn)
            row[k] = {"gpu_us": round(one, 1), "chain_us": round(chain, 2), "gbps": round(8.0 * B * M * C / chain / 1e3, 1)}
        res["shapes"]["M%d_C%d" % (M, C)] = row
print(json.dumps(res))

"""The self-supervised batch preparation at the pre-training shape (B 24, M 5000, npoint 2048, C 3; pretrain_partseg_shapenet.py:
321-351 without the rotation flags: scale, shift, channels-first copy, input subset), two arms of `Trainer._selfsup_batch`:
  torch   the default path: random_scale_shift (device draws, clone, multiply-add, slice assign), transpose().contiguous(), index
          gather with .contiguous(), the subset from np.random.choice uploaded as int64;
  fused   fused_augment=True: host draws, provider.compose_affine, ONE upload (matrices + subset), ONE prifit_affine_points launch;
and `kernel`: ops.affine_points alone with matrices and subset already on the device.
Per arm, medians over the timed calls:
  host_us   time.perf_counter around the call from an empty queue, no synchronise inside the window (the enqueue cost; both
            trainer arms include their draws and their host-to-device copy);
  gpu_us    device events around the call's work, enqueued behind a few ms of other work so the events bracket kernels and copies,
            not the host's enqueue;
  launches  kernels the torch profiler saw in one call (null if the profiler reports none).
The arms take turns call by call.  usage (GPU box): python tools/bench_augment.py [timed calls, default 200]  -> one JSON line"""
import json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prifit_amd import ops, provider, synth
from prifit_amd.train_step import Trainer

steps = max(50, int(sys.argv[1])) if len(sys.argv) > 1 else 200
assert torch.cuda.is_available(), "bench_augment.py times a GPU: no CPU path"
B, M, NPOINT = 24, 5000, 2048
dev = torch.device("cuda", 0)
cham = torch.from_numpy(synth.cloud("blobs", B, M, 0)).to(dev)
tr = Trainer(torch.nn.Linear(3, 2))           # _selfsup_batch does not touch the model
np.random.seed(0), torch.manual_seed(0)
aff_dev = torch.from_numpy(provider.compose_affine(scale=np.random.uniform(0.8, 1.25, B), shift=np.random.uniform(-0.1, 0.1, (B, 3)))).to(dev)
sub_dev = torch.from_numpy(np.random.choice(M, NPOINT, replace=False).astype(np.int32)).to(dev)
arms = {
    "torch": lambda: tr._selfsup_batch(cham, NPOINT, True, None),
    "fused": lambda: tr._selfsup_batch(cham, NPOINT, True, None, fused_augment=True),
    "kernel": lambda: ops.affine_points(cham, aff_dev, subset=sub_dev, want_cf=True),
}
for fn in arms.values():                       # warm-up: code objects loaded, allocator pools grown
    for _ in range(5):
        fn()
torch.cuda.synchronize()

host = {k: [] for k in arms}
for _ in range(steps):
    for k, fn in arms.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        host[k].append((time.perf_counter() - t0) * 1e6)
torch.cuda.synchronize()

A = torch.randn(4096, 4096, device=dev)
gpu = {k: [] for k in arms}
for _ in range(steps):
    for k, fn in arms.items():
        for _ in range(3):
            torch.mm(A, A)                     # the queue stays busy while the host enqueues the call
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        gpu[k].append(e0.elapsed_time(e1) * 1e3)

launches = {}
for k, fn in arms.items():
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                 and "memset" not in e.name.lower()]
        launches[k] = len(names) or None
    except Exception as e:                      # the figure is optional; the timings above are not
        print("# torch profiler: %s" % e, file=sys.stderr)
        launches[k] = None

res = {"tool": "bench_augment", "B": B, "M": M, "npoint": NPOINT, "C": 3, "steps": steps, "torch_version": torch.__version__,
       "device": torch.cuda.get_device_name(0)}
for k in arms:
    res[k] = {"host_us": round(statistics.median(host[k]), 1), "gpu_us": round(statistics.median(gpu[k]), 1), "launches": launches[k]}
res["fused_no_slower_on_host"] = res["fused"]["host_us"] <= res["torch"]["host_us"]
res["fused_no_slower_on_gpu"] = res["fused"]["gpu_us"] <= res["torch"]["gpu_us"]
print(json.dumps(res))

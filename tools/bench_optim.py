"""One optimizer step of momentum SGD over the MSG network's parameter set (104 tensors, 1.76 M floats), random gradients:
FlatSGD (prifit_amd/optim.py, one launch: csrc/optim.hip prifit_sgd_flat) against torch.optim.SGD with foreach=True and with
fused=True, each where the installed torch accepts it.  Two figures per arm, each the median over the timed steps:
  host_us  time.perf_counter around `opt.step()` from an empty queue (what the step costs the enqueuing thread);
  gpu_us   device events around the step's launches, enqueued behind a few ms of other work so that the events bracket the
           kernels and not the host's enqueue.
The arms take turns step by step, so they share whatever else the host is doing.  Needs no reference and no dataset.
usage (GPU box): python tools/bench_optim.py [timed steps, default 100, at least 50]      -> one JSON line"""
import json, os, statistics, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prifit_amd.models import pointnet2_part_seg_msg as M
from prifit_amd.optim import FlatSGD

steps = max(50, int(sys.argv[1])) if len(sys.argv) > 1 else 100
assert torch.cuda.is_available(), "bench_optim.py times a GPU: no CPU path"
dev = torch.device("cuda", 0)
torch.manual_seed(0)
shapes = [tuple(p.shape) for p in M.get_model(50).parameters()]
kw = dict(lr=1e-3, momentum=0.9)           # the trainer's arm (train_partseg_shapenet.py:261)


def make(build):
    params = [torch.nn.Parameter(torch.randn(*s, device=dev)) for s in shapes]
    opt = build(params)
    for p in params:                        # the same gradient tensors every step, as a static training step has them
        p.grad = torch.randn_like(p)
    return opt


arms = {"flat_sgd": make(lambda ps: FlatSGD(ps, **kw))}
for name, flag in (("torch_foreach", dict(foreach=True)), ("torch_fused", dict(fused=True))):
    try:
        arms[name] = make(lambda ps: torch.optim.SGD(ps, **kw, **flag))
        arms[name].step()                   # (fused: the device / dtype check happens in the first step)
    except (RuntimeError, TypeError, ValueError) as e:
        arms.pop(name, None)
        print("# torch.optim.SGD(%s) not accepted here: %s" % (", ".join("%s=%s" % kv for kv in flag.items()), e), file=sys.stderr)
arms["flat_sgd"].step()                     # one warm-up step each: code objects loaded, momentum buffers exist
torch.cuda.synchronize()

host = {k: [] for k in arms}
for _ in range(steps):
    for k, opt in arms.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.step()
        host[k].append((time.perf_counter() - t0) * 1e6)
torch.cuda.synchronize()

A = torch.randn(4096, 4096, device=dev)
gpu = {k: [] for k in arms}
for _ in range(steps):
    for k, opt in arms.items():
        for _ in range(3):
            torch.mm(A, A)                  # the queue stays busy while the host enqueues the step
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        opt.step()
        e1.record()
        torch.cuda.synchronize()
        gpu[k].append(e0.elapsed_time(e1) * 1e3)

res = {"tool": "bench_optim", "tensors": len(shapes), "floats": sum(p.numel() for p in arms["flat_sgd"].params), "steps": steps,
       "momentum": kw["momentum"], "torch": torch.__version__, "device": torch.cuda.get_device_name(0)}
for k in arms:
    res[k] = {"host_us": round(statistics.median(host[k]), 1), "gpu_us": round(statistics.median(gpu[k]), 1)}
rivals = [k for k in arms if k != "flat_sgd"]
if rivals:
    best = min(rivals, key=lambda k: res[k]["host_us"])
    res["torch_fastest_host"] = best
    res["flat_faster_on_host"] = res["flat_sgd"]["host_us"] < res[best]["host_us"]
print(json.dumps(res))

"""SegmentationEvaluator.update at the evaluation's shape (B = 24 shapes, N = 2048 points, P = 50 parts, fp32 logits), by HIP
events and by the host clock: the kernel path (one launch of csrc/seg_metrics.hip, nothing read back) against the torch path it
replaced, kept callable as SegmentationEvaluator(fused=False).  Also: the kernel alone (ops.seg_metrics into preallocated outputs)
with its achieved bytes/s against the B N P 4 bytes it must read, and the host synchronisations per update of both paths as
torch's sync debug mode counts them.  Both paths see the same seeded batch; their metrics are compared before anything is timed.
usage (GPU box): python tools/bench_seg_metrics.py [repetitions, default 200] [output file, default profiles/seg_metrics.txt]"""
import os, sys, time, warnings
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prifit_amd import ops, testing as T

B, N, P = 24, 2048, 50
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "seg_metrics.txt")
dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
cats = rng.integers(0, 16, size=B)
target_np = np.stack([rng.choice(T.seg_classes[T.classes[c]], size=N) for c in cats]).astype(np.int64)
logits_np = rng.normal(size=(B, N, P)).astype(np.float32)
logits_np[np.arange(B)[:, None], np.arange(N)[None], target_np] += 1.5
logits, target = torch.from_numpy(logits_np).to(dev), torch.from_numpy(target_np).to(dev)


def timed(step, warm, reps):
    """-> (ms per call by device events, ms per call on the host clock, both over the same window ending in a synchronise)."""
    for _ in range(warm): step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps): step()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, (time.perf_counter() - t0) * 1e3 / reps


def syncs_per_update(ev):
    """Synchronising calls in one update(), counted by torch.cuda.set_sync_debug_mode("warn"); None if the mode says nothing."""
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            float(logits[0, 0, 0])
            probe = len(w)
            ev.update(logits, target)
            n = len(w) - probe
    finally:
        torch.cuda.set_sync_debug_mode(before)
    return n if probe else None


fused, plain = T.SegmentationEvaluator(), T.SegmentationEvaluator(fused=False)
fused.update(logits, target); plain.update(logits, target)
mf, mp = fused.compute(), plain.compute()
agree = max(abs(mf[k] - mp[k]) for k in ("accuracy", "class_avg_iou", "instance_avg_iou"))
assert agree < 1e-12, (mf, mp)
sync_f, sync_p = syncs_per_update(fused), syncs_per_update(plain)
fused.reset(); plain.reset()

tab = fused._table
totals = torch.zeros(2 + 2 * P, dtype=torch.int64, device=dev)
outs = (torch.empty(B, N, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
        torch.zeros(B, P, dtype=torch.int32, device=dev), torch.zeros(B, P, dtype=torch.int32, device=dev))
k_ms, _ = timed(lambda: ops.seg_metrics(logits, target, tab, True, totals, out=outs), 20, 5 * reps)
rounds = []
for _ in range(3):                                           # the two paths alternate: the box is shared
    fused.reset(); plain.reset()
    rounds.append((timed(lambda: plain.update(logits, target), 5, reps), timed(lambda: fused.update(logits, target), 5, reps)))
(p_ms, p_host), (f_ms, f_host) = (tuple(float(np.median([r[i][j] for r in rounds])) for j in (0, 1)) for i in (0, 1))

nbytes = 4.0 * B * N * P
say = lambda n: "not counted (sync debug mode not honoured)" if n is None else "%d" % n
lines = ["SegmentationEvaluator.update, B = %d, N = %d, P = %d, fp32 logits (%.1f MB), %d repetitions, median of 3 alternating rounds, %s"
         % (B, N, P, nbytes / 1e6, reps, torch.cuda.get_device_name(0)),
         "torch path (fused=False)   %8.3f ms per update by device events, %8.3f ms on the host clock, host synchronisations per update: %s"
         % (p_ms, p_host, say(sync_p)),
         "kernel path                %8.3f ms per update by device events, %8.3f ms on the host clock, host synchronisations per update: %s"
         % (f_ms, f_host, say(sync_f)),
         "ratio torch / kernel       %8.1fx by device events, %.1fx on the host clock%s"
         % (p_ms / f_ms, p_host / f_host, "" if f_ms < p_ms and f_host < p_host else "  (kernel path NOT faster)"),
         "kernel alone (ops.seg_metrics, preallocated outputs, back to back) %.2f us per launch = %.0f GB/s of the %.1f MB it must read"
         % (k_ms * 1e3, nbytes / (k_ms * 1e-3) / 1e9, nbytes / 1e6),
         "metrics of the two paths on this batch agree to %.1e" % agree]
print("\n".join(lines))
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

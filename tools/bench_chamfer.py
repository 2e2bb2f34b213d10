"""Two-sided point-set Chamfer distance, forward + backward, by HIP events: the batched op (src/utils.py
chamfer_distance_kdtree -> fit_ops.ChamferNNFn, csrc/chamfer.hip) against the path it replaced -- one shape at a time, a
[4096, T] distance matrix per chunk, torch.argmin, gradient by autograd through the gather (copied below as `before`).
Shapes: B = 24 and B = 1, 10000 surface samples against 5000 cloud points.  Prints and writes both times and their ratio.
usage (GPU box): python tools/bench_chamfer.py [output file, default profiles/chamfer_nn.txt]"""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prifit_amd.src.utils import chamfer_distance_kdtree as after


def nearest_index(src, tgt, chunk=4096):
    out = []
    with torch.no_grad():
        for i in range(0, src.shape[0], chunk):
            d = ((src[i:i + chunk, None, :] - tgt[None, :, :]) ** 2).sum(-1)
            out.append(d.argmin(dim=1))
    return torch.cat(out)


def before(source_points, target_points):
    per = []
    for b in range(source_points.shape[0]):
        s, t = source_points[b], target_points[b]
        d_st = ((t - s[nearest_index(t, s)]) ** 2).sum(1)
        d_ts = ((s - t[nearest_index(s, t)]) ** 2).sum(1)
        per.append((d_st.mean() + d_ts.mean()) / 2.0)
    return torch.stack(per).mean()


def time_ms(fn, S, T, warm, reps):
    def step():
        S.grad = T.grad = None
        fn(S, T).backward()
    for _ in range(warm): step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): step()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


lines = ["two-sided chamfer distance, forward + backward, NA = 10000 surface samples, NB = 5000 cloud points, fp32, ms per call (HIP events)"]
g = torch.Generator().manual_seed(0)
for B, warm, reps in ((24, 3, 20), (1, 5, 50)):
    S = torch.randn(B, 10000, 3, generator=g).cuda().requires_grad_(True)
    T = torch.randn(B, 5000, 3, generator=g).cuda().requires_grad_(True)
    lb, la = before(S, T), after(S, T)
    t_before = time_ms(before, S, T, warm, reps)
    t_after = time_ms(after, S, T, warm, reps)
    lines.append("B = %2d  before (per-shape torch loop) %9.3f ms   after (batched HIP op) %8.3f ms   ratio %7.1fx%s   loss %.7f / %.7f"
                 % (B, t_before, t_after, t_before / t_after, "" if t_after < t_before else "  (NOT faster)", float(lb), float(la)))
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chamfer_nn.txt")
print("\n".join(lines))
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")

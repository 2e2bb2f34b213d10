"""The per-point embedding of the frozen MSG part-segmentation network at the benchmark shape (B = 24 clouds of N = 2048
points), by HIP events, for both precisions: (a) frozen.forward(embed=True) followed by the torch arg-max of seg -- the only way
to the embedding before FrozenPartSeg.embed(), with the permute to row-major a consumer needs -- against (b)
frozen.embed(return_labels=True); then the embedding chain (prifit_mlp_chain_embed_*) alone against the launches it replaces
on the same 49,152 fp1 rows: fp1's two products and its ReLU launch, conv1 + bn1's product and its ReLU launch, the conv2 and
extra_conv_emb products.  The arms alternate within a round (the box is shared); the table gives the median and (min .. max)
of the rounds.  The yardstick is this commit's own forward(embed=True), which embed() does not alter.  The outputs of the two
arms are compared before anything is timed.
usage (GPU box): python tools/bench_embed.py [repetitions, default 20] [rounds, default 5] [output file, default profiles/infer_embed.txt]"""
import ctypes, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prifit_amd import inference
from prifit_amd.models import pointnet2_part_seg_msg as M

B, N = 24, 2048
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "infer_embed.txt")
dev = torch.device("cuda", 0)


def timed(step, warm, reps):
    for _ in range(warm): step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): step()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(steps, warm, reps, rounds):
    """-> per step (median, min, max) ms over `rounds` rounds, the steps taking turns inside every round."""
    got = [[] for _ in steps]
    for _ in range(rounds):
        for i, s in enumerate(steps):
            got[i].append(timed(s, warm, reps))
    return [(float(np.median(g)), min(g), max(g)) for g in got]


def verdict(new, old):
    """`new` is faster beyond the run-to-run spread only if its slowest round beats the other arm's fastest."""
    return "faster beyond the spread" if new[2] < old[1] else "NOT faster beyond the spread"


torch.manual_seed(0)
net = M.get_model(50).to(dev)
with torch.no_grad():
    for m in net.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.weight.uniform_(0.5, 1.5); m.bias.normal_(0.0, 0.1)
    net.train()
    for _ in range(2):
        net(torch.rand(4, 3, N, device=dev) * 2 - 1, torch.eye(16, device=dev)[torch.randint(0, 16, (4,))].reshape(4, 1, 16))
net.eval()
g = torch.Generator().manual_seed(1)
xyz = (torch.rand(B, 3, N, generator=g) * 2 - 1).to(dev)
onehot = torch.eye(16)[torch.randint(0, 16, (B,), generator=g)].reshape(B, 1, 16).to(dev)
start = (torch.randint(0, N, (B,), generator=g).to(dev), torch.randint(0, 512, (B,), generator=g).to(dev))

lines = ["per-point embedding, B = %d x N = %d, %d repetitions x %d alternating rounds (median, min .. max), %s"
         % (B, N, reps, rounds, torch.cuda.get_device_name(0))]
for precision in inference.PRECISIONS:
    frozen = inference.freeze(net, precision=precision)

    def old_route():
        out = frozen(xyz, onehot, fps_start=start, embed=True)
        return out[-1].permute(0, 2, 1).contiguous(), out[0].argmax(dim=-1)

    def new_route():
        return frozen.embed(xyz, onehot, fps_start=start, return_labels=True)

    (e0, l0), (e1, l1) = old_route(), new_route()
    torch.cuda.synchronize()
    lines += ["", "precision %s: max |embed() - forward(embed=True)| = %.3g (max |emb| %.3g), labels equal on %.4f %% of the points"
              % (precision, float((e0 - e1).abs().max()), float(e0.abs().max()), 100.0 * float((l0 == l1.long()).float().mean()))]
    a, b = alternate([old_route, new_route], 3, reps, rounds)
    lines += ["(a) forward(embed=True) + permute + torch arg-max   %8.3f ms  (%.3f .. %.3f)" % a,
              "(b) embed(return_labels=True)                       %8.3f ms  (%.3f .. %.3f)   (b) is %s" % (b + (verdict(b, a),))]

    # the tail alone, on the same rows
    K0, widths, parts = frozen._embed_shape()
    P = B * N
    rows = torch.randn(P, K0, device=dev)
    st, w0, _, _ = frozen._fp["fp1"]
    rows4 = rows[:, :w0.W.shape[1]].contiguous()                  # the rows forward() builds: padded to 4, not 8
    emb = torch.empty(B, N, widths[-1], device=dev)
    lab = torch.empty(B, N, dtype=torch.int32, device=dev)

    def replaced():
        l0_up = torch.empty(P, st[-1].cout, device=dev)
        frozen._stack(rows4, False, st, w0.W, 0, l0_up)
        feat = torch.empty(P, frozen._head[0].cout, device=dev)
        frozen._stack(l0_up, False, frozen._head, frozen._head[0].W, 0, feat)
        return frozen._linear(feat, frozen._conv2), frozen._linear(feat, frozen._emb)

    def chain():
        frozen._chain_embed(rows, K0, widths, parts, emb, False, lab, None, None, N)

    def chain_norm():
        frozen._chain_embed(rows, K0, widths, parts, emb, True, lab, None, None, N)

    r, c, cn = alternate([replaced, chain, chain_norm], 3, reps, rounds)
    flops = 2.0 * P * (sum(k * w for k, w in zip([K0] + widths[:-1], widths)) + widths[-2] * parts)
    entry = inference._CHAINS[precision]["embed"][0]
    lines += ["the tail alone on %d fp1 rows (K0 = %d, widths %s + %d parts): 5 products and 2 ReLU launches (fp32 in both precisions)"
              % (P, K0, tuple(widths), parts),
              "replaced launches                      %8.3f ms  (%.3f .. %.3f)" % r,
              "%-30s         %8.3f ms  (%.3f .. %.3f)   %.1f TFLOP/s, %.0f GB/s of rows in + embedding out; %s"
              % ((entry,) + c + (flops / (c[0] * 1e-3) / 1e12, 4.0 * P * (K0 + widths[-1]) / (c[0] * 1e-3) / 1e9, verdict(c, r))),
              "%-30s         %8.3f ms  (%.3f .. %.3f)   %s" % ((entry + ", normalize",) + cn + (verdict(cn, r),))]
    del frozen

print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

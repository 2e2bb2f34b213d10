"""One iteration of the classifier-layer pre-training (`--init_cls`, train_partseg_shapenet.py:56-99) at the benchmark shape
(B = 24 clouds of N = 2048 points), by HIP events, three ways on the same weights, inputs, labels and sampling starts:
  (a) the live route: the model in .eval(), get_loss, autograd (the whole backward for conv2's 6,450 parameters), FlatSGD on conv2;
  (b) the frozen forward and the existing separate launches: FrozenPartSeg.forward() for (seg, feat), prifit_cross_entropy_fwd /
      _bwd on seg, log_softmax's backward in torch, the TN product dW = dz^T feat, torch's column sum, FlatSGD on conv2
      (the row chain's scores alone do not give a3, which the TN product needs: forward()'s feat is the existing way to it);
  (c) FrozenPartSeg.probe_step() + FlatSGD.step().
Every arm owns a copy of the network and steps it; the arms alternate within a round (the box is shared) and the table gives
the median and the (min .. max) of the rounds.  The first-iteration losses of the three arms are compared before anything is
timed.  Then the fused head alone (prifit_probe_head_f32) next to the forward row chain (prifit_mlp_chain_rows_f32) on the same
random fp1 rows.
usage (GPU box): python tools/bench_probe.py [repetitions, default 20] [rounds, default 5] [output file, default profiles/probe_head.txt]"""
import copy, ctypes, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prifit_amd import inference, nn_ops
from prifit_amd._lib import call, cur_stream, dll, ptr
from prifit_amd.models import pointnet2_part_seg_msg as M
from prifit_amd.optim import FlatSGD

B, N = 24, 2048
argv = sys.argv[1:]
reps = int(argv[0]) if len(argv) > 0 else 20
rounds = int(argv[1]) if len(argv) > 1 else 5
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "probe_head.txt")
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
target = torch.randint(0, 50, (B, N), generator=g).to(dev)
flat_target = target.reshape(-1)

net_a, net_b, net_c = copy.deepcopy(net), copy.deepcopy(net), copy.deepcopy(net)
crit = M.get_loss()
params_a = list(net_a.parameters())
opt_a = FlatSGD(net_a.conv2.parameters(), lr=0.1, momentum=0.5)
frozen_b, frozen_c = inference.freeze(net_b), inference.freeze(net_c)
opt_b = FlatSGD(net_b.conv2.parameters(), lr=0.1, momentum=0.5)
opt_c = FlatSGD(net_c.conv2.parameters(), lr=0.1, momentum=0.5)
last = {}


def live():
    for p in params_a: p.grad = None
    seg = net_a(xyz, onehot, fps_start=start)[0]
    loss = crit(seg.contiguous().view(-1, 50), flat_target)
    loss.backward()
    opt_a.step()
    last["a"] = loss.detach()


def separate():
    w, b = net_b.conv2.weight, net_b.conv2.bias
    frozen_b._conv2.W.copy_(w.detach().reshape(50, 128)); frozen_b._conv2.b.copy_(b.detach())    # the live conv2 into the folded buffer
    out = frozen_b(xyz, onehot, fps_start=start)
    seg, feat = out[0].reshape(-1, 50), out[2].permute(0, 2, 1).reshape(-1, 128)
    y = seg.detach().requires_grad_()
    loss = nn_ops.CrossEntropyFn.apply(y, flat_target)
    loss.backward()
    dy = y.grad
    dz = (dy - torch.exp(seg) * dy.sum(dim=1, keepdim=True)).contiguous()
    feat = feat.contiguous()
    w.grad = nn_ops._weight_grad(dz, B * N, 50, feat, 128, None, out=torch.zeros(50, 128, device=dev)).reshape(w.shape)
    b.grad = dz.sum(dim=0)
    opt_b.step()
    last["b"] = loss.detach()


def fused():
    last["c"] = frozen_c.probe_step(xyz, onehot, target, fps_start=start)[0]
    opt_c.step()


live(); separate(); fused()
torch.cuda.synchronize()
lines = ["classifier-layer pre-training, one iteration, B = %d x N = %d, %d repetitions x %d alternating rounds (median, min .. max), %s"
         % (B, N, reps, rounds, torch.cuda.get_device_name(0)),
         "first-iteration loss: (a) %.7f  (b) %.7f  (c) %.7f" % (float(last["a"]), float(last["b"]), float(last["c"]))]
(a_ms, a_lo, a_hi), (b_ms, b_lo, b_hi), (c_ms, c_lo, c_hi) = alternate([live, separate, fused], 3, reps, rounds)
lines += ["(a) live eval forward, get_loss, autograd, FlatSGD(conv2)          %8.3f ms  (%.3f .. %.3f)" % (a_ms, a_lo, a_hi),
          "(b) frozen forward, cross-entropy launches, TN product, FlatSGD    %8.3f ms  (%.3f .. %.3f)" % (b_ms, b_lo, b_hi),
          "(c) probe_step() + FlatSGD.step()                                  %8.3f ms  (%.3f .. %.3f)" % (c_ms, c_lo, c_hi),
          "ratio (a) / (c) %6.2fx     ratio (b) / (c) %6.2fx%s" % (a_ms / c_ms, b_ms / c_ms, "" if c_ms <= b_hi else "  ((c) NOT faster than (b))")]

# the head alone
tail, K0 = frozen_c._tail, frozen_c._tail_kp
widths = [ly.cout for ly in tail]
P = B * N
rows = torch.randn(P, K0, device=dev)
Ws = [frozen_c._tail_w0.W] + [ly.W for ly in tail[1:]]
bs = [ly.b for ly in tail]
cw = (ctypes.c_int32 * 4)(*widths)
dW, db, loss4 = torch.empty(50, 128, device=dev), torch.empty(50, device=dev), torch.empty(4, device=dev)
ws = torch.empty(dll().prifit_probe_head_workspace(P, K0, 4, cw), device=dev)
scores = torch.empty(P, widths[-1], device=dev)


def head():
    call("prifit_probe_head_f32", ptr(rows), K0, P, K0, 4, cw, nn_ops._ptr_array(Ws), (ctypes.c_longlong * 4)(*[W.stride(0) for W in Ws]),
         nn_ops._ptr_array(bs), ptr(flat_target), ptr(dW), 128, ptr(db), ptr(loss4), ptr(ws), cur_stream())


def chain_rows():
    call("prifit_mlp_chain_rows_f32", ptr(rows), K0, P, K0, 4, cw, nn_ops._ptr_array(Ws), (ctypes.c_longlong * 4)(*[W.stride(0) for W in Ws]),
         nn_ops._ptr_array(bs), ptr(scores), widths[-1], None, None, None, N, None, cur_stream())


(h_ms, h_lo, h_hi), (r_ms, r_lo, r_hi) = alternate([head, chain_rows], 3, reps, rounds)
flops = 2.0 * P * (sum(k * c for k, c in zip([K0] + widths[:-1], widths)) + 128 * widths[-1])
lines += ["", "the head alone on %d fp1 rows (K0 = %d, widths %s), both launches; next to it the forward row chain writing scores" % (P, K0, tuple(widths)),
          "prifit_probe_head_f32      %7.3f ms  (%.3f .. %.3f)   %4.1f %% of the fp32 MFMA peak (157.3 TF) over forward + dW flops"
          % (h_ms, h_lo, h_hi, 100.0 * flops / (h_ms * 1e-3) / 157.3e12),
          "prifit_mlp_chain_rows_f32  %7.3f ms  (%.3f .. %.3f)" % (r_ms, r_lo, r_hi)]
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

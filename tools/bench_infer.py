"""The eval-mode forward of the MSG part-segmentation network at the benchmark shape (B = 24 clouds of N = 2048 points), by
HIP events: (a) the live model in .eval() under no_grad -- the route evaluate_loader has always run -- against (b) the frozen
model of prifit_amd.inference on the same weights, inputs and sampling starts; then, per SA1 / SA2 scale, the chain kernel
(prifit_mlp_chain_pool_f32) against the launches it replaces (SharedMLPFn in eval mode on the same first-layer rows: the
coefficient arithmetic, two products, the pool).  Every arm sees the same seeded state in every repeat; the arms alternate
within a round (the box is shared) and the table gives the median and the (min .. max) of the rounds.  The outputs of the two
arms are compared before anything is timed.  Then the part labels: (c) frozen.predict() followed by the torch restricted
arg-max of SegmentationEvaluator.predict -- the only way to labels before FrozenPartSeg.labels() -- against (d) frozen.labels(),
and the row chain (prifit_mlp_chain_rows_f32) alone against the launches it replaces on the same fp1 rows; written to a
second file.  Last, the bf16 arms, to a third file: the frozen forward and labels() of precision="fp32"
against precision="bf16", per scale the bf16 chain against the fp32 chain on the same first-layer rows, the row chains
likewise, the share of the points whose labels agree and the largest |seg_bf16 - seg_fp32|.
usage (GPU box): python tools/bench_infer.py [repetitions, default 20] [rounds, default 5] [output file, default profiles/infer.txt]
                                             [labels output file, default profiles/infer_labels.txt]
                                             [bf16 output file, default profiles/infer_bf16.txt] [--bf16-only]"""
import ctypes, os, sys
import numpy as np, torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prifit_amd import inference, nn_ops, testing as T
from prifit_amd._lib import call, cur_stream, ptr, query
from prifit_amd.models import pointnet2_part_seg_msg as M
from prifit_amd.nn_ops import FrontEnd, SharedMLPFn

B, N = 24, 2048
argv = [a for a in sys.argv[1:] if a != "--bf16-only"]
bf16_only = "--bf16-only" in sys.argv
reps = int(argv[0]) if len(argv) > 0 else 20
rounds = int(argv[1]) if len(argv) > 1 else 5
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "infer.txt")
labels_path = argv[3] if len(argv) > 3 else os.path.join(ROOT, "profiles", "infer_labels.txt")
bf16_path = argv[4] if len(argv) > 4 else os.path.join(ROOT, "profiles", "infer_bf16.txt")
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
frozen = inference.freeze(net)
g = torch.Generator().manual_seed(1)
xyz = (torch.rand(B, 3, N, generator=g) * 2 - 1).to(dev)
onehot = torch.eye(16)[torch.randint(0, 16, (B,), generator=g)].reshape(B, 1, 16).to(dev)
start = (torch.randint(0, N, (B,), generator=g).to(dev), torch.randint(0, 512, (B,), generator=g).to(dev))


def live():
    with torch.no_grad():
        return net(xyz, onehot, fps_start=start)


def cold():
    return frozen(xyz, onehot, fps_start=start)


def section_forward():
    a, b = live(), cold()
    torch.cuda.synchronize()
    d_seg, d_feat = float((a[0] - b[0]).abs().max()), float((a[2] - b[2]).abs().max())
    same = float((a[0].argmax(-1) == b[0].argmax(-1)).float().mean())
    lines = ["eval-mode forward, B = %d x N = %d, %d repetitions x %d alternating rounds (median, min .. max), %s"
             % (B, N, reps, rounds, torch.cuda.get_device_name(0)),
             "outputs: max |seg_live - seg_frozen| = %.3g, max |feat_live - feat_frozen| = %.3g, arg-max equal on %.4f %% of the points"
             % (d_seg, d_feat, 100.0 * same)]
    (l_ms, l_lo, l_hi), (f_ms, f_lo, f_hi) = alternate([live, cold], 3, reps, rounds)
    lines += ["(a) live model.eval(), no_grad   %8.3f ms  (%.3f .. %.3f)" % (l_ms, l_lo, l_hi),
              "(b) frozen                       %8.3f ms  (%.3f .. %.3f)" % (f_ms, f_lo, f_hi),
              "ratio live / frozen              %8.2fx%s" % (l_ms / f_ms, "" if f_ms <= l_ms else "  (frozen NOT faster)"),
              "", "per scale: layers 2 + 3 + pool of one set-abstraction scale on its first-layer rows",
              "  scale (C0, C1, C2, K)        rows      replaced launches ms        chain kernel ms      ratio   share of the fp32 MFMA peak"]

    for lv in frozen._sa:
        S = lv["npoint"]
        for (st, _), K in zip(lv["scales"], lv["nsamples"]):
            C0, C1, C2 = st[0].cout, st[1].cout, st[2].cout
            G = B * S
            P = G * K
            X = torch.randn(P, C0, device=dev)
            out = torch.empty(G, C2, device=dev)
            ts = [None, None] + [getattr(st[0].bn, k) for k in ("weight", "bias", "running_mean", "running_var")]
            for ly in st[1:]:
                ts += [ly.conv.weight.reshape(ly.cout, -1), ly.conv.bias] + [getattr(ly.bn, k) for k in ("weight", "bias", "running_mean", "running_var")]

            def replaced():
                cfg = {"pool_K": K, "training": False, "eps": st[0].bn.eps, "momentum": [0.1] * 3, "front": FrontEnd("preact", True),
                       "pool_out": out}
                with torch.no_grad():
                    SharedMLPFn.apply(X, cfg, *ts)

            def chain():
                call("prifit_mlp_chain_pool_f32", ptr(X), C0, G, K, C0, C1, C2, ptr(st[1].W), st[1].ldw, ptr(st[1].b), ptr(st[2].W),
                     st[2].ldw, ptr(st[2].b), ptr(out), C2, None, cur_stream())

            taken = bool(query("prifit_mlp_chain_pool_supported", C0, C1, C2, K))
            if not taken:
                lines.append("  (%3d, %3d, %3d, %3d)  %9d   not taken by the chain kernel: the folded products serve it" % (C0, C1, C2, K, P))
                continue
            (r_ms, r_lo, r_hi), (c_ms, c_lo, c_hi) = alternate([replaced, chain], 3, reps, rounds)
            peak = 2.0 * P * (C0 * C1 + C1 * C2) / (c_ms * 1e-3) / 157.3e12
            lines.append("  (%3d, %3d, %3d, %3d)  %9d   %7.3f (%.3f .. %.3f)   %7.3f (%.3f .. %.3f)   %5.2fx   %4.1f %%%s"
                         % (C0, C1, C2, K, P, r_ms, r_lo, r_hi, c_ms, c_lo, c_hi, r_ms / c_ms, 100.0 * peak,
                            "" if c_ms <= r_hi else "  (chain NOT faster)"))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def section_labels():
    # ---- part labels: (c) the parent's way -- frozen.predict() and the torch restricted arg-max of SegmentationEvaluator.predict
    # -- against (d) frozen.labels(); then the row chain alone against the launches it replaces, on the same fp1 rows
    ev = T.SegmentationEvaluator()
    col_host = ev.cat_of_label
    shape_cat = onehot.reshape(B, 16).argmax(dim=1)
    first = torch.stack([(col_host == int(c)).nonzero()[0, 0] for c in shape_cat.cpu()])
    target = first.view(B, 1).expand(B, N).contiguous().to(dev)              # target[:, 0] selects the category, as in testing.py:142
    col_dev = col_host.to(torch.int32).to(dev)
    cat_dev = shape_cat.to(torch.int32)


    def old_labels():
        return ev.predict(frozen.predict(xyz, onehot, fps_start=start), target)[0]


    def new_labels():
        return frozen.labels(xyz, onehot, cat_dev, col_dev, fps_start=start)


    c, d = old_labels(), new_labels()
    torch.cuda.synchronize()
    agree = float((c == d.long()).float().mean())
    (c_ms, c_lo, c_hi), (d_ms, d_lo, d_hi) = alternate([old_labels, new_labels], 3, reps, rounds)
    lab = ["part labels, B = %d x N = %d, %d repetitions x %d alternating rounds (median, min .. max), %s"
           % (B, N, reps, rounds, torch.cuda.get_device_name(0)),
           "labels of the two arms equal on %.4f %% of the points" % (100.0 * agree),
           "(c) frozen.predict() + torch restricted arg-max   %8.3f ms  (%.3f .. %.3f)" % (c_ms, c_lo, c_hi),
           "(d) frozen.labels()                               %8.3f ms  (%.3f .. %.3f)" % (d_ms, d_lo, d_hi),
           "ratio (c) / (d)                                   %8.2fx%s"
           % (c_ms / d_ms, "" if d_ms <= c_hi else "  (labels() NOT faster)")]

    tail, K0 = frozen._tail, frozen._tail_kp
    widths = [ly.cout for ly in tail]
    P = B * N
    rows = torch.randn(P, K0, device=dev)
    rows4 = rows[:, :frozen._fp["fp1"][1].W.shape[1]].contiguous()            # the rows forward() builds: padded to 4, not 8
    Ws = [frozen._tail_w0.W] + [ly.W for ly in tail[1:]]
    out = torch.empty(P, dtype=torch.int32, device=dev)
    allowed = col_dev.view(1, 1, -1) == cat_dev.view(-1, 1, 1)


    def replaced_tail():
        st, w0, _, _ = frozen._fp["fp1"]
        l0_up = torch.empty(P, st[-1].cout, device=dev)
        frozen._stack(rows4, False, st, w0.W, 0, l0_up)
        feat = torch.empty(P, frozen._head[0].cout, device=dev)
        frozen._stack(l0_up, False, frozen._head, frozen._head[0].W, 0, feat)
        seg = F.log_softmax(frozen._linear(feat, frozen._conv2), dim=1).reshape(B, N, -1)
        return seg.masked_fill(~allowed, float("-inf")).argmax(dim=-1)


    def chain_rows():
        call("prifit_mlp_chain_rows_f32", ptr(rows), K0, P, K0, 4, (ctypes.c_int32 * 4)(*widths), nn_ops._ptr_array(Ws),
             (ctypes.c_longlong * 4)(*[W.stride(0) for W in Ws]), nn_ops._ptr_array([ly.b for ly in tail]), None, widths[-1], ptr(out),
             ptr(col_dev), ptr(cat_dev), N, None, cur_stream())


    (r_ms, r_lo, r_hi), (k_ms, k_lo, k_hi) = alternate([replaced_tail, chain_rows], 3, reps, rounds)
    flops = 2.0 * P * sum(k * c for k, c in zip([K0] + widths[:-1], widths))
    lab += ["", "the tail alone on %d fp1 rows (K0 = %d, widths %s): 4 products, 2 ReLU launches, log_softmax, masked arg-max" % (P, K0, tuple(widths)),
            "replaced launches        %8.3f ms  (%.3f .. %.3f)" % (r_ms, r_lo, r_hi),
            "prifit_mlp_chain_rows_f32 %7.3f ms  (%.3f .. %.3f)   %5.2fx   %4.1f %% of the fp32 MFMA peak (157.3 TF)%s"
            % (k_ms, k_lo, k_hi, r_ms / k_ms, 100.0 * flops / (k_ms * 1e-3) / 157.3e12, "" if k_ms <= r_hi else "  (chain NOT faster)")]
    print("\n".join(lab))
    with open(labels_path, "w") as f:
        f.write("\n".join(lab) + "\n")


def section_bf16():
    """precision="bf16" against precision="fp32" of the same run: the baseline of every time is the fp32 arm next to it."""
    cold16 = inference.freeze(net, precision="bf16")
    col_dev = T.SegmentationEvaluator().cat_of_label.to(torch.int32).to(dev)
    cat_dev = onehot.reshape(B, 16).argmax(dim=1).to(torch.int32)
    fwd32 = lambda: frozen(xyz, onehot, fps_start=start)
    fwd16 = lambda: cold16(xyz, onehot, fps_start=start)
    lab32 = lambda: frozen.labels(xyz, onehot, cat_dev, col_dev, fps_start=start)
    lab16 = lambda: cold16.labels(xyz, onehot, cat_dev, col_dev, fps_start=start)
    seg32, seg16, l32, l16 = fwd32()[0], fwd16()[0], lab32(), lab16()
    torch.cuda.synchronize()
    out = ["frozen inference, precision fp32 against bf16, B = %d x N = %d, %d repetitions x %d alternating rounds (median, min .. max), %s"
           % (B, N, reps, rounds, torch.cuda.get_device_name(0)),
           "labels() of the two precisions agree on %.4f %% of the %d points; arg-max of seg on %.4f %%; max |seg_bf16 - seg_fp32| = %.4g"
           % (100.0 * float((l32 == l16).float().mean()), B * N, 100.0 * float((seg32.argmax(-1) == seg16.argmax(-1)).float().mean()),
              float((seg32 - seg16).abs().max()))]
    for what, a, b in (("forward()", fwd32, fwd16), ("labels() ", lab32, lab16)):
        (a_ms, a_lo, a_hi), (b_ms, b_lo, b_hi) = alternate([a, b], 3, reps, rounds)
        out += ["%s fp32   %8.3f ms  (%.3f .. %.3f)" % (what, a_ms, a_lo, a_hi),
                "%s bf16   %8.3f ms  (%.3f .. %.3f)   fp32 / bf16 %5.2fx%s"
                % (what, b_ms, b_lo, b_hi, a_ms / b_ms, "" if b_hi < a_lo else "  (NOT faster beyond the spread)")]
    out += ["", "per scale: layers 2 + 3 + pool on the same first-layer rows, weights of the frozen modules",
            "  scale (C0, C1, C2, K)        rows      fp32 chain ms               bf16 chain ms          ratio   bf16: TFLOP/s   HBM GB/s (rows in)"]
    for lv in cold16._sa:
        S = lv["npoint"]
        for (st, _), (w1, w2), K in zip(lv["scales"], lv["bf16"], lv["nsamples"]):
            C0, C1, C2 = st[0].cout, st[1].cout, st[2].cout
            G = B * S
            P = G * K
            X = torch.randn(P, C0, device=dev)
            o32, o16 = torch.empty(G, C2, device=dev), torch.empty(G, C2, device=dev)

            def f32():
                call("prifit_mlp_chain_pool_f32", ptr(X), C0, G, K, C0, C1, C2, ptr(st[1].W), st[1].ldw, ptr(st[1].b), ptr(st[2].W),
                     st[2].ldw, ptr(st[2].b), ptr(o32), C2, None, cur_stream())

            def b16():
                call("prifit_mlp_chain_pool_bf16", ptr(X), C0, G, K, C0, C1, C2, ptr(w1.W), w1.ldk, ptr(st[1].b), ptr(w2.W), w2.ldk,
                     ptr(st[2].b), ptr(o16), C2, None, cur_stream())

            (a_ms, a_lo, a_hi), (b_ms, b_lo, b_hi) = alternate([f32, b16], 3, reps, rounds)
            out.append("  (%3d, %3d, %3d, %3d)  %9d   %7.3f (%.3f .. %.3f)   %7.3f (%.3f .. %.3f)   %5.2fx   %7.1f   %7.0f%s"
                       % (C0, C1, C2, K, P, a_ms, a_lo, a_hi, b_ms, b_lo, b_hi, a_ms / b_ms,
                          2.0 * P * (C0 * C1 + C1 * C2) / (b_ms * 1e-3) / 1e12, 4.0 * P * C0 / (b_ms * 1e-3) / 1e9,
                          "" if b_hi < a_lo else "  (bf16 NOT faster beyond the spread)"))
    tail, K0 = cold16._tail, cold16._tail_kp
    widths = [ly.cout for ly in tail]
    P = B * N
    rows = torch.randn(P, K0, device=dev)
    W32 = [frozen._tail_w0.W] + [ly.W for ly in frozen._tail[1:]]
    W16 = [w.W for w in cold16._tail_bf16]
    lab = torch.empty(P, dtype=torch.int32, device=dev)

    def rows_chain(entry, Ws, bs):
        return lambda: call(entry, ptr(rows), K0, P, K0, 4, (ctypes.c_int32 * 4)(*widths), nn_ops._ptr_array(Ws),
                            (ctypes.c_longlong * 4)(*[W.stride(0) for W in Ws]), nn_ops._ptr_array(bs), None, widths[-1], ptr(lab),
                            ptr(col_dev), ptr(cat_dev), N, None, cur_stream())

    (a_ms, a_lo, a_hi), (b_ms, b_lo, b_hi) = alternate([rows_chain("prifit_mlp_chain_rows_f32", W32, [ly.b for ly in frozen._tail]),
                                                        rows_chain("prifit_mlp_chain_rows_bf16", W16, [ly.b for ly in tail])], 3, reps, rounds)
    flops = 2.0 * P * sum(k * c for k, c in zip([K0] + widths[:-1], widths))
    out += ["", "the tail alone on %d fp1 rows (K0 = %d, widths %s)" % (P, K0, tuple(widths)),
            "prifit_mlp_chain_rows_f32   %7.3f ms  (%.3f .. %.3f)" % (a_ms, a_lo, a_hi),
            "prifit_mlp_chain_rows_bf16  %7.3f ms  (%.3f .. %.3f)   %5.2fx   %.1f TFLOP/s, %.0f GB/s of rows in%s"
            % (b_ms, b_lo, b_hi, a_ms / b_ms, flops / (b_ms * 1e-3) / 1e12, 4.0 * P * K0 / (b_ms * 1e-3) / 1e9,
               "" if b_hi < a_lo else "  (bf16 NOT faster beyond the spread)")]
    print("\n".join(out))
    os.makedirs(os.path.dirname(os.path.abspath(bf16_path)), exist_ok=True)
    with open(bf16_path, "w") as f:
        f.write("\n".join(out) + "\n")


if not bf16_only:
    section_forward()
    section_labels()
section_bf16()

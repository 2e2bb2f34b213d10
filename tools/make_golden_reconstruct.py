"""Writes tests/golden/atlas_decoder.npz and tests/golden/atlas_model.npz: what the reference's own AtlasNet and
ChamferDistance (models/reconstruction.py) return in fp64 on CPU tensors for the seeded recipes of tests/atlas_common.py.
Needs the reference tree (oracle/refshim.py imports it; PRIFIT_REFERENCE names its root).  The files hold returned values
only; weights, z and targets are regenerated from their seeds by the tests.

atlas_decoder.npz, per case (B, num_charts, num_points): output_points, the loss against the seeded target cloud, the
gradient of z, per parameter tensor the sum and the sum of squares of its gradient, chart 0's updated running statistics;
one eval-mode output.

atlas_model.npz: the reference's whole part-segmentation net with reconstruct=True, B = 2, N = 512.  Its forward stops on
CPU tensors at the in-place update of the loss (:118), so a forward hook on fp1 captures l0_points; z is its mean, and
AtlasNet / ChamferDistance are then called on their own as :116-118 do.

    python tools/make_golden_reconstruct.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refshim  # noqa: E402
import atlas_common as ac  # noqa: E402


def load(net, sd, dtype):
    net.load_state_dict({k: torch.from_numpy(np.array(v)).to(dtype if v.dtype == np.float32 else torch.int64)
                         for k, v in sd.items()})


def decoder_cases(REC):
    out = {}
    for B, C, npts, seed in ac.GOLDEN_CASES:
        tag = "%d_%d_%d|" % (B, C, npts)
        sd = ac.make_state(seed, C)
        z, target = ac.make_inputs(seed, B)
        net = REC.AtlasNet(num_charts=C, num_points=npts).double()
        load(net, sd, torch.float64)
        net.train()
        zt = torch.from_numpy(z).double().requires_grad_(True)
        pts = net(zt)
        loss = REC.ChamferDistance()(pts, torch.from_numpy(target).double())
        loss.backward()
        out[tag + "out"] = pts.detach().numpy()
        out[tag + "loss"] = loss.detach().numpy()
        out[tag + "gz"] = zt.grad.numpy()
        mom = np.zeros((len(ac.PARAM_ORDER), C, 2))
        named = dict(net.named_parameters())
        for a, name in enumerate(ac.PARAM_ORDER):
            for i in range(C):
                g = named["decoder.%d.%s" % (i, name)].grad.numpy()
                mom[a, i] = g.sum(), (g * g).sum()
        out[tag + "grad_moments"] = mom
        for l in (1, 2, 3):
            bn = getattr(net.decoder[0], "bn%d" % l)
            out[tag + "bn%d.running_mean" % l] = bn.running_mean.numpy().copy()
            out[tag + "bn%d.running_var" % l] = bn.running_var.numpy().copy()
    B, C, npts, seed = ac.GOLDEN_EVAL
    net = REC.AtlasNet(num_charts=C, num_points=npts).double()
    load(net, ac.make_state(seed, C), torch.float64)
    net.eval()
    with torch.no_grad():
        out["eval|out"] = net(torch.from_numpy(ac.make_inputs(seed, B)[0]).double()).numpy()
    return out


def model_case(REC):
    MODEL = refshim.ref("models.pointnet2_part_seg_msg")
    torch.manual_seed(ac.MODEL_CASE["seed"])
    net = MODEL.get_model(50, reconstruct=True)
    load(net.atlasnet, ac.make_state(ac.MODEL_CASE["decoder_seed"], 25), torch.float32)
    net.train()
    xyz, cls = ac.model_inputs()
    got = {}
    net.fp1.register_forward_hook(lambda m, i, o: got.__setitem__("l0", o.detach()))
    try:                               # the backbone runs in fp32 (its index arithmetic is typed); the decoder below in fp64
        net(torch.from_numpy(xyz), torch.from_numpy(cls))
    except RuntimeError as e:          # the in-place update of the leaf total_loss, after fp1 has run
        print("reference forward stopped as expected:", str(e).splitlines()[0])
    z = got["l0"].mean(dim=2).double()
    net.atlasnet.double()
    with torch.no_grad():
        pts = net.atlasnet(z)
        rec = net.chamferdistance(pts, torch.from_numpy(xyz).double().permute(0, 2, 1))
    return {"z": z.numpy(), "output_points": pts.numpy(), "rec": rec.numpy()}


def main():
    REC = refshim.ref("models.reconstruction")
    for name, data in (("atlas_decoder", decoder_cases(REC)), ("atlas_model", model_case(REC))):
        path = os.path.join(ROOT, "tests", "golden", name + ".npz")
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

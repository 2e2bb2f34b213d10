"""Writes tests/golden/chamfer_pointsets.npz: the values the reference's own point-set Chamfer functions (src/utils.py
chamfer_distance :271, chamfer_distance_one_side :297, chamfer_distance_single_shape :324, chamfer_distance_kdtree :361)
return on CPU tensors for one seeded pair of clouds, B = 2, N = 130, M = 97.  Needs the reference tree (oracle/refshim.py
imports it; PRIFIT_REFERENCE names its root) and scikit-learn for its KD-tree.  The file holds the inputs and the returned
values only.

    python tools/make_golden_chamfer.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import refshim  # noqa: E402


def main():
    UT = refshim.ref("src.utils")
    rng = np.random.default_rng(20240611)
    pred = rng.standard_normal((2, 130, 3)).astype(np.float32)
    gt = rng.standard_normal((2, 97, 3)).astype(np.float32)
    P, Q = torch.from_numpy(pred), torch.from_numpy(gt)
    out = {"pred": pred, "gt": gt}

    def put(name, value, **kw):
        key = name + "".join("|%s=%d" % (k, int(v)) for k, v in sorted(kw.items()))
        out[key] = value.detach().numpy().astype(np.float32)
        print("%-70s %s" % (key, out[key] if out[key].ndim == 0 else out[key].shape))

    for sq in (False, True):
        put("chamfer_distance", UT.chamfer_distance(P, Q, sqrt=sq), sqrt=sq)
        put("chamfer_distance_kdtree", UT.chamfer_distance_kdtree(P, Q, sqrt=sq), sqrt=sq)
    for side in (0, 1):
        put("chamfer_distance_one_side", UT.chamfer_distance_one_side(P, Q, side=side), side=side)
    for one_side in (False, True):
        for sq in (False, True):
            for reduce in (False, True):
                if not one_side and not reduce:
                    continue        # adds an [N] and an [M] vector: upstream's broadcast fails for N != M
                put("chamfer_distance_single_shape",
                    UT.chamfer_distance_single_shape(P[0], Q[0], one_side=one_side, sqrt=sq, reduce=reduce),
                    one_side=one_side, sqrt=sq, reduce=reduce)
    path = os.path.join(ROOT, "tests", "golden", "chamfer_pointsets.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

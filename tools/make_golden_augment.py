"""Write tests/golden/augment_provider.npz from the upstream reference's `provider` module (CPU, needs the reference tree:
oracle/refshim.py finds it; nothing of it is copied, only arrays it computes are stored).

    python tools/make_golden_augment.py

Three groups of arrays:
  fn_input [3,17,3] float32, fn_angle, and per function `fn_<name>`: its output on a copy of fn_input after np.random.seed(7)
      (the eight per-shape affine functions prifit_amd/provider.py adds; the two *_by_angle functions take fn_angle);
  seq_input [2,40,3] float32, seq_output: the chamfer_points side of pretrain_partseg_shapenet.py:321-337 with all three flags on
      after np.random.seed(9) -- random_scale, shift, random_anisotropic_scale, rotate_point_cloud_y, rotate_point_cloud_y_pi4,
      each assigned back into the float32 array as the script does;
  seq_scale [2], seq_shift [2,3], seq_aniso [2,1,3], seq_angle [2], seq_angle2 [2]: that sequence's draws, read off the same
      seeded stream in the order the five functions make them (angles in radians: uniform() * 2 pi, randint(1, 8) * pi / 4).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import refshim  # noqa: E402

FN_SEED, SEQ_SEED, FN_ANGLE = 7, 9, 0.7
RANDOM_FNS = ("rotate_point_cloud", "rotate_point_cloud_z", "rotate_point_cloud_y", "rotate_point_cloud_y_pi4",
              "rotate_perturbation_point_cloud", "random_anisotropic_scale_point_cloud")
ANGLE_FNS = ("rotate_point_cloud_y_by_angle", "rotate_point_cloud_by_angle")


def main():
    ref = refshim.ref("provider")
    out = {}
    rng = np.random.default_rng(11)
    fn_input = rng.uniform(-1, 1, (3, 17, 3)).astype(np.float32)
    out["fn_input"], out["fn_angle"] = fn_input, np.float64(FN_ANGLE)
    for name in RANDOM_FNS:
        np.random.seed(FN_SEED)
        out["fn_" + name] = getattr(ref, name)(fn_input.copy())
    for name in ANGLE_FNS:
        out["fn_" + name] = getattr(ref, name)(fn_input.copy(), FN_ANGLE)

    seq_input = rng.uniform(-1, 1, (2, 40, 3)).astype(np.float32)
    cham = seq_input.copy()
    np.random.seed(SEQ_SEED)
    cham[:, :, 0:3] = ref.random_scale_point_cloud(cham[:, :, 0:3])
    cham[:, :, 0:3] = ref.shift_point_cloud(cham[:, :, 0:3])
    cham[:, :, 0:3] = ref.random_anisotropic_scale_point_cloud(cham[:, :, 0:3], scale_low=0.8, scale_high=1.25)
    cham[:, :, 0:3] = ref.rotate_point_cloud_y(cham[:, :, 0:3])
    cham[:, :, 0:3] = ref.rotate_point_cloud_y_pi4(cham[:, :, 0:3])
    out["seq_input"], out["seq_output"] = seq_input, cham

    B = seq_input.shape[0]
    np.random.seed(SEQ_SEED)
    out["seq_scale"] = np.random.uniform(0.8, 1.25, B)
    out["seq_shift"] = np.random.uniform(-0.1, 0.1, (B, 3))
    out["seq_aniso"] = np.random.uniform(0.8, 1.25, [B, 1, 3])
    out["seq_angle"] = np.array([np.random.uniform() * 2 * np.pi for _ in range(B)])
    out["seq_angle2"] = np.array([np.random.randint(1, 8) * np.pi / 4 for _ in range(B)])

    path = os.path.join(ROOT, "tests", "golden", "augment_provider.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()

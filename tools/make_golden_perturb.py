"""Write tests/golden/perturb_provider.npz from the upstream reference's `provider` module (CPU, needs the reference tree:
oracle/refshim.py finds it; nothing of it is copied, only arrays it computes are stored).

    python tools/make_golden_perturb.py

The seven functions prifit_amd/provider.py adds beside the per-shape affine family, each on a copy of its input after
np.random.seed(FN_SEED):
  in6 [3,37,6] float32 (xyz, unit normals), in3 = its xyz [3,37,3], labels [3] int64, angle;
  fn_random_point_dropout (in3), fn_rotate_point_cloud_with_normal, fn_rotate_perturbation_point_cloud_with_normal,
  fn_rotate_point_cloud_by_angle_with_normal (in6, angle), fn_shuffle_points, fn_normalize_data (in6): the returned array;
  fn_shuffle_data_data / _labels / _idx: the three values shuffle_data(in6, labels) returns.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import refshim  # noqa: E402

FN_SEED, FN_ANGLE = 13, 0.7


def main():
    ref = refshim.ref("provider")
    rng = np.random.default_rng(23)
    in6 = rng.uniform(-1, 1, (3, 37, 6)).astype(np.float32)
    in6[:, :, 3:] /= np.linalg.norm(in6[:, :, 3:], axis=2, keepdims=True)
    in3 = np.ascontiguousarray(in6[:, :, :3])
    labels = np.array([4, 0, 9], dtype=np.int64)
    out = {"in6": in6, "in3": in3, "labels": labels, "angle": np.float64(FN_ANGLE)}

    def seeded(name, *args):
        np.random.seed(FN_SEED)
        return getattr(ref, name)(*args)

    out["fn_random_point_dropout"] = seeded("random_point_dropout", in3.copy())
    out["fn_rotate_point_cloud_with_normal"] = seeded("rotate_point_cloud_with_normal", in6.copy())
    out["fn_rotate_perturbation_point_cloud_with_normal"] = seeded("rotate_perturbation_point_cloud_with_normal", in6.copy())
    out["fn_rotate_point_cloud_by_angle_with_normal"] = seeded("rotate_point_cloud_by_angle_with_normal", in6.copy(), FN_ANGLE)
    out["fn_shuffle_points"] = seeded("shuffle_points", in6.copy())
    out["fn_normalize_data"] = seeded("normalize_data", in6.copy())
    data, lab, idx = seeded("shuffle_data", in6.copy(), labels.copy())
    out["fn_shuffle_data_data"], out["fn_shuffle_data_labels"], out["fn_shuffle_data_idx"] = data, lab, idx

    path = os.path.join(ROOT, "tests", "golden", "perturb_provider.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()

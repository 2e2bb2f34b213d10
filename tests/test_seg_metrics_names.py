"""CPU: the names the one-launch part-segmentation metrics add -- the entry point in the header and in the built library,
`ops.seg_metrics`, `src.eval_utils.mean_IOU_one_sample` under the reference's module path -- and the evaluator's CPU path, which
stays the torch path, against the loop form of testing.py:139-241 (tests/seg_metrics_common.py)."""
import ctypes
import importlib
import inspect
import sys

import numpy as np
import torch

import seg_metrics_common as S
from prifit_amd import _lib
from prifit_amd import testing as T


def test_library_exports_seg_metrics_with_the_headers_signature(hiplib):
    assert "prifit_seg_metrics" in _lib.declared_symbols()
    # scores, ld, target, B, N, P, cat_of_label, restricted, pred, shape_cat, inter, uni, totals, stream
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib._signatures()["prifit_seg_metrics"] == [P, LL, P, I, I, I, P, I, P, P, P, P, P, P]
    fn = hiplib.prifit_seg_metrics
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib._signatures()["prifit_seg_metrics"]


def test_entry_point_rejects_bad_shapes_without_a_launch(hiplib):
    """P > 64, ld < P, B or N <= 0: non-zero before anything is launched (no device is needed to be told so; the pointers are
    never followed)."""
    fn = hiplib.prifit_seg_metrics
    p = 256                                                  # any non-NULL address
    ok = dict(ld=50, B=2, N=8, P=50)
    for bad in (dict(P=65, ld=65), dict(P=0), dict(ld=49), dict(B=0), dict(N=0), dict(B=-1), dict(N=-3)):
        a = dict(ok, **bad)
        assert fn(p, a["ld"], p, a["B"], a["N"], a["P"], p, 1, None, p, p, p, p, None) != 0, bad


def test_ops_seg_metrics_signature():
    from prifit_amd import ops
    params = inspect.signature(ops.seg_metrics).parameters
    assert list(params)[:5] == ["scores", "target", "cat_of_label", "restricted", "totals"]
    assert params["restricted"].default is True and params["totals"].default is None


def test_evaluator_keeps_the_torch_path_callable():
    params = inspect.signature(T.SegmentationEvaluator.__init__).parameters
    assert list(params)[:3] == ["self", "num_part", "categories"] and params["fused"].default is True


def test_compat_resolves_eval_utils():
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k.split(".")[0] in ("models", "src", "convex_loss")}
    try:
        from prifit_amd import compat
        assert "src.eval_utils" in compat.install()
        fn = importlib.import_module("src.eval_utils").mean_IOU_one_sample
        assert fn.__module__ == "prifit_amd.src.eval_utils"
        assert list(inspect.signature(fn).parameters) == ["pred", "gt", "C"]
    finally:
        for k in list(sys.modules):
            if k.split(".")[0] in ("models", "src", "convex_loss"):
                del sys.modules[k]
        sys.modules.update({k: v for k, v in saved.items() if v is not None})


def test_mean_iou_one_sample_toy_case():
    from prifit_amd.src.eval_utils import mean_IOU_one_sample
    pred = np.array([0, 0, 1, 1, 1, 0])
    gt = np.array([0, 1, 1, 1, 0, 0])
    # label 0: 2 of 4, label 1: 2 of 4, label 2: absent from both -> eps / eps = 1
    eps = np.finfo(np.float32).eps
    direct = 0.0
    for inter, union in ((2, 4), (2, 4), (0, 0)):
        direct = direct + (np.float64(inter) + eps) / (np.float64(union) + eps)
    direct = direct / 3
    got = mean_IOU_one_sample(pred, gt, 3)
    assert got == direct and abs(got - 2.0 / 3.0) < 1e-7
    assert mean_IOU_one_sample(gt, gt, 3) == 1.0


def test_cpu_path_gives_the_loop_forms_dict():
    """The CPU path is today's torch path: same numbers as the loop form on a seeded input with every category, one of them
    twice, and a part that neither occurs nor is predicted."""
    col, names = S.cat_table()
    batches = S.seeded_batches(11, [(T.classes[:6], 70), (T.classes[6:12], 70), (T.classes[12:] + ["Motorbike", "Bag"], 70)])
    ev = T.SegmentationEvaluator()
    for logits, target in batches:
        pred = ev.update(torch.from_numpy(logits), torch.from_numpy(target))
        assert pred.dtype == torch.int64 and np.array_equal(pred.numpy(), S.batch_counts(logits, target, col)[0])
    got, ref = ev.compute(), S.metrics(batches, col, names)
    for k in ("accuracy", "class_avg_accuracy", "class_avg_iou", "instance_avg_iou"):
        assert S.same(got[k], ref[k]) or abs(got[k] - ref[k]) < 1e-12, (k, got[k], ref[k])
    for name, v in ref["category_iou"].items():
        assert abs(got["category_iou"][name] - v) < 1e-12, name
    assert type(ev.correct) is int and ev.correct == ref["correct"] and ev.seen == ref["seen"]
    assert ev.seen_class.dtype == torch.int64 and np.array_equal(ev.seen_class.numpy(), ref["seen_class"])
    assert np.array_equal(ev.correct_class.numpy(), ref["correct_class"])
    assert ev.bad == 0 and ev._totals is None and not ev._pending          # the kernel path was not taken

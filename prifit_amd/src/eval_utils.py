"""src/eval_utils.py of the reference under its own name: the per-sample mean IoU in its eps form (numpy, host)."""
import numpy as np

_EPS = float(np.finfo(np.float32).eps)      # float32's eps as a float64 value: the counts are integers, the sums float64


def mean_IOU_one_sample(pred, gt, C):
    """Mean over the labels 0 .. C-1 of (|pred == l and gt == l| + eps) / (|pred == l or gt == l| + eps), eps that of
    float32: a label absent from both counts as 1.  Summed in label order, in float64, as the reference does."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    total = 0.0
    for label in range(C):
        in_pred, in_gt = pred == label, gt == label
        both = np.count_nonzero(in_pred & in_gt)
        either = np.count_nonzero(in_pred | in_gt)
        total = total + (both + _EPS) / (either + _EPS)
    return total / C

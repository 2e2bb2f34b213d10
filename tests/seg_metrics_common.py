"""The yardstick of the part-segmentation metrics tests: testing.py:139-204 of the reference restated in numpy, per-shape loops
and np.argmax over the category's columns.  The averages over shapes and categories (:226-240) are then taken the way
SegmentationEvaluator.compute() has always taken them -- shapes in batch order, a float64 host tensor's .mean() per category and
over all shapes, categories without shapes left out of the class average -- so that `==` can be asked of them too (np.mean and
torch's mean add in different orders: the last bit)."""
import numpy as np
import torch

from prifit_amd import testing as T


def cat_table(num_part=50, categories=None):
    """-> (int64 [num_part] category of each part, -1 = none; the category names)."""
    categories = categories if categories is not None else T.seg_classes
    names = list(categories.keys())
    col = np.full(num_part, -1, dtype=np.int64)
    for ci, name in enumerate(names):
        col[categories[name]] = ci
    return col, names


def batch_counts(logits, target, col, restricted=True):
    """One batch, the loop form: logits [B,N,P] float32, target [B,N] with every label in [0, P).
    -> pred [B,N] int64, shape_cat [B], inter [B,P], uni [B,P] (int64), shape_iou [B] float64, correct, seen_class [P],
    correct_class [P]."""
    B, N, P = logits.shape
    pred = np.zeros((B, N), dtype=np.int64)
    shape_cat = np.zeros(B, dtype=np.int64)
    inter = np.zeros((B, P), dtype=np.int64)
    uni = np.zeros((B, P), dtype=np.int64)
    shape_iou = np.zeros(B, dtype=np.float64)
    for i in range(B):
        cat = col[target[i, 0]]
        shape_cat[i] = cat
        parts = np.nonzero(col == cat)[0]
        if restricted:
            pred[i] = np.argmax(logits[i][:, parts], 1) + parts[0]
        else:
            pred[i] = np.argmax(logits[i], 1)
        part_ious = []
        for part in range(P):
            inter[i, part] = np.sum((target[i] == part) & (pred[i] == part))
            uni[i, part] = np.sum((target[i] == part) | (pred[i] == part))
        for part in parts:
            if np.sum(target[i] == part) == 0 and np.sum(pred[i] == part) == 0:
                part_ious.append(1.0)
            else:
                part_ious.append(np.sum((target[i] == part) & (pred[i] == part)) / float(np.sum((target[i] == part) | (pred[i] == part))))
        shape_iou[i] = np.mean(part_ious)
    correct = int(np.sum(pred.reshape(-1, 1) == target.reshape(-1, 1)))
    seen_class = np.array([np.sum(target == part) for part in range(P)], dtype=np.int64)
    correct_class = np.array([np.sum((pred == part) & (target == part)) for part in range(P)], dtype=np.int64)
    return pred, shape_cat, inter, uni, shape_iou, correct, seen_class, correct_class


def metrics(batches, col, names):
    """The evaluator's dict over a list of (logits, target) batches."""
    P = col.shape[0]
    correct, seen = 0, 0
    seen_class, correct_class = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    ious, cats = [], []
    for logits, target in batches:
        _, shape_cat, _, _, shape_iou, c, sc, cc = batch_counts(logits, target, col)
        correct += c
        seen += target.size
        seen_class += sc
        correct_class += cc
        ious.extend(shape_iou.tolist())
        cats.extend(shape_cat.tolist())
    ious, cats = torch.tensor(ious, dtype=torch.float64), torch.tensor(cats, dtype=torch.long)
    per_cat = {name: (float(ious[cats == ci].mean()) if bool((cats == ci).any()) else float("nan")) for ci, name in enumerate(names)}
    with np.errstate(invalid="ignore", divide="ignore"):
        class_acc = float(np.mean(correct_class.astype(np.float64) / seen_class.astype(np.float64)))
    present = [v for v in per_cat.values() if not np.isnan(v)]
    return {"accuracy": correct / float(seen), "class_avg_accuracy": class_acc, "class_avg_iou": float(np.mean(present)),
            "instance_avg_iou": float(ious.mean()), "category_iou": per_cat,
            "correct": correct, "seen": seen, "seen_class": seen_class, "correct_class": correct_class}


def same(a, b):
    """== on two floats, nan equal to nan."""
    return (np.isnan(a) and np.isnan(b)) or a == b


def assert_same_metrics(got, ref):
    for k in ("accuracy", "class_avg_accuracy", "class_avg_iou", "instance_avg_iou"):
        assert same(got[k], ref[k]), (k, got[k], ref[k])
    assert list(got["category_iou"]) == list(ref["category_iou"])
    for name, v in ref["category_iou"].items():
        assert same(got["category_iou"][name], v), (name, got["category_iou"][name], v)


def seeded_batches(seed, shapes, P=50, boost=1.5):
    """[(logits [B,N,P] float32, target [B,N] int64)]: `shapes` = a list of (list of category names, N) per batch; labels drawn
    from the category's parts, logits normal with the target's column raised (mostly right)."""
    rng = np.random.default_rng(seed)
    out = []
    for cats, N in shapes:
        tgt = np.stack([rng.choice(T.seg_classes[c], size=N) for c in cats]).astype(np.int64)
        logits = rng.normal(size=(len(cats), N, P)).astype(np.float32)
        logits[np.arange(len(cats))[:, None], np.arange(N)[None], tgt] += boost
        out.append((logits, tgt))
    return out

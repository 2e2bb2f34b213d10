"""GPU: the part-segmentation metrics in one launch (csrc/seg_metrics.hip prifit_seg_metrics, ops.seg_metrics, the kernel path of
testing.SegmentationEvaluator) against the numpy loop form of testing.py:139-204 in tests/seg_metrics_common.py -- never against
the code under test.  Everything the kernel produces is an integer count, so every comparison is `==`: on the counts, and on the
float64 metrics compute() forms from them."""
import numpy as np
import pytest
import torch

import seg_metrics_common as S
from prifit_amd import testing as T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENT32, SENT64 = 0x5eadbeef, 0x5eadbeef5eadbeef


def table(col):
    return torch.from_numpy(col.astype(np.int32)).to(DEV)


def run(logits, target, col, restricted=True, totals=None):
    """ops.seg_metrics on host arrays -> numpy (pred, shape_cat, inter, uni, totals)."""
    from prifit_amd import ops
    scores = logits if torch.is_tensor(logits) else torch.from_numpy(logits).to(DEV)
    out = ops.seg_metrics(scores, torch.from_numpy(target).to(DEV), table(col), restricted, totals)
    return tuple(t.cpu().numpy() for t in out)


def check_against_loops(logits_np, target, col, restricted=True, scores=None):
    P = col.shape[0]
    pred, shape_cat, inter, uni, totals = run(logits_np if scores is None else scores, target, col, restricted)
    r_pred, r_cat, r_inter, r_uni, _, r_correct, r_seen, r_corr = S.batch_counts(logits_np, target, col, restricted)
    assert pred.dtype == np.int64 and shape_cat.dtype == np.int32 and inter.dtype == np.int32 and totals.dtype == np.int64
    assert np.array_equal(pred, r_pred)
    assert np.array_equal(shape_cat, r_cat)
    assert np.array_equal(inter, r_inter) and np.array_equal(uni, r_uni)
    assert totals.shape == (2 + 2 * P,) and totals[0] == r_correct and totals[1] == 0
    assert np.array_equal(totals[2:2 + P], r_seen) and np.array_equal(totals[2 + P:], r_corr)
    return pred


def evaluator_metrics(batches, **kw):
    ev = T.SegmentationEvaluator(**kw)
    for logits, target in batches:
        pred = ev.update(torch.from_numpy(logits).to(DEV), torch.from_numpy(target).to(DEV))
        assert pred.is_cuda and pred.dtype == torch.int64 and tuple(pred.shape) == target.shape
    assert ev._pending and ev.correct == 0                   # the kernel path: nothing has been read back yet
    return ev, ev.compute()


@pytest.mark.parametrize("cats,N", [(["Motorbike", "Bag", "Airplane"], 70),      # 6 parts, 2 parts; N crosses 64 rows
                                    (["Lamp"], 1),
                                    (["Table", "Motorbike"], 2048 + 40)])       # several workgroups per shape, ragged tail
def test_counts_and_metrics_match_the_loop_form(cats, N):
    col, names = S.cat_table()
    batches = S.seeded_batches(3, [(cats, N)])
    check_against_loops(batches[0][0], batches[0][1], col)
    ev, got = evaluator_metrics(batches)
    ref = S.metrics(batches, col, names)
    S.assert_same_metrics(got, ref)
    assert type(ev.correct) is int and ev.correct == ref["correct"] and ev.seen == ref["seen"]
    assert ev.seen_class.dtype == torch.int64 and not ev.seen_class.is_cuda
    assert np.array_equal(ev.seen_class.numpy(), ref["seen_class"]) and np.array_equal(ev.correct_class.numpy(), ref["correct_class"])


@pytest.mark.parametrize("restricted", [True, False])
def test_row_stride_64_pad_columns_are_never_read(restricted):
    """P = 50 scores in rows of 64 floats; columns 50 .. 63 hold +inf and NaN, either of which would win every arg-max."""
    col, _ = S.cat_table()
    (logits, target), = S.seeded_batches(4, [(["Chair", "Mug", "Rocket"], 70)])
    B, N, P = logits.shape
    buf = torch.empty(B * N, 64, device=DEV)
    buf[:, 50::2] = float("inf")
    buf[:, 51::2] = float("nan")
    buf[:, :P] = torch.from_numpy(logits).to(DEV).view(B * N, P)
    scores = buf.view(B, N, 64)[..., :P]
    assert scores.stride() == (N * 64, 64, 1)
    check_against_loops(logits, target, col, restricted, scores=scores)


def test_unrestricted_13_parts_one_category():
    col = np.zeros(13, dtype=np.int64)
    rng = np.random.default_rng(5)
    logits = rng.normal(size=(2, 70, 13)).astype(np.float32)
    target = rng.integers(0, 13, size=(2, 70)).astype(np.int64)
    check_against_loops(logits, target, col, restricted=False)
    check_against_loops(logits, target, col, restricted=True)          # one category over every part: the same thing
    # ... and through the evaluator: a 13-part category's shape IoU is np.mean over 13 parts
    cats = {"All": list(range(13))}
    ev, got = evaluator_metrics([(logits, target)], num_part=13, categories=cats)
    S.assert_same_metrics(got, S.metrics([(logits, target)], col, ["All"]))


def special_rows():
    """One Motorbike shape (parts 30 .. 35): ties among the allowed parts, larger scores in foreign columns, -inf and NaN."""
    neg_nan = np.copysign(np.float32("nan"), np.float32(-1.0))
    rows = []                       # (allowed scores [6], foreign fill, expected part)
    rows.append(([1, 5, 2, 5, 0, -1], 100.0, 31))                        # two share the maximum, a foreign part holds more
    rows.append(([7, 7, 7, 1, 0, -1], np.inf, 30))                       # three share it, foreign +inf
    rows.append(([0, 1, 2, 3, 9, 9], np.nan, 34))                        # a tie at the end, foreign NaN
    rows.append(([-np.inf] * 6, 3.0, 30))                                # all allowed -inf: the first allowed part
    rows.append(([-np.inf, -np.inf, -3e38, -np.inf, -3e38, -np.inf], 0.0, 32))
    rows.append(([1, 7, np.nan, 2, np.nan, 0], 50.0, 32))                # NaN after a larger finite value: the first NaN
    rows.append(([np.inf, 1, 2, neg_nan, 0, np.nan], -1.0, 33))          # NaN beats +inf, whatever its sign bit
    rows.append(([-0.0, 0.0, -1, -2, -3, -4], -5.0, 30))                 # -0 == +0: the first of them
    rows.append(([-1, 0.0, -0.0, -2, -3, -4], -5.0, 31))
    rows.append(([-1e-45, -2, 1e-45, 1e-45, -3, -4], 0.0, 32))           # denormals are ordered, not flushed
    logits = np.empty((1, len(rows), 50), dtype=np.float32)
    for r, (allowed, foreign, _) in enumerate(rows):
        logits[0, r, :] = foreign
        logits[0, r, 30:36] = allowed
    target = np.array([[30, 31, 32, 33, 34, 35, 30, 31, 32, 33][:len(rows)]], dtype=np.int64)
    return logits, target, np.array([e for _, _, e in rows])


def test_ties_infinities_and_nan_follow_numpy():
    col, names = S.cat_table()
    logits, target, expect = special_rows()
    with np.errstate(invalid="ignore"):
        pred = check_against_loops(logits, target, col)
    assert pred[0].tolist() == expect.tolist()
    # unrestricted, the same rows: now the foreign columns count (+inf, NaN and the larger values win, first index)
    with np.errstate(invalid="ignore"):
        check_against_loops(logits, np.full_like(target, 3), col, restricted=False)


def test_absent_part_counts_as_iou_one():
    """A Cap shape (parts 6, 7) where only part 6 occurs and is predicted: IoU(6) = 1, IoU(7) = 1 (absent from both); a Bag shape
    (4, 5) with target 4 4 5 5 predicted 4 4 4 5: IoU(4) = 2/3, IoU(5) = 1/2."""
    lg = np.full((2, 4, 50), -5.0, dtype=np.float32)
    lg[0, :, 20] = 9.0
    lg[0, [0, 1, 2], 4] = 1.0
    lg[0, 3, 5] = 1.0
    lg[1, :, 6] = 1.0
    tg = np.array([[4, 4, 5, 5], [6, 6, 6, 6]], dtype=np.int64)
    col, names = S.cat_table()
    ev, got = evaluator_metrics([(lg, tg)])
    assert got["category_iou"]["Cap"] == 1.0
    assert got["category_iou"]["Bag"] == np.mean([2.0 / 3.0, 1.0 / 2.0]) and got["accuracy"] == 7.0 / 8.0
    S.assert_same_metrics(got, S.metrics([(lg, tg)], col, names))
    _, _, inter, uni, _ = run(lg, tg, col)
    assert inter[1].tolist() == [0] * 6 + [4] + [0] * 43 and uni[1].tolist() == [0] * 6 + [4] + [0] * 43


def test_updates_accumulate_and_reset_clears():
    from prifit_amd import ops
    col, names = S.cat_table()
    b1, b2, b3 = S.seeded_batches(6, [(["Car", "Guitar"], 70), (["Knife", "Car", "Laptop"], 33), (["Pistol"], 130)])
    ev = T.SegmentationEvaluator()
    for lg, tg in (b1, b2):
        ev.update(torch.from_numpy(lg).to(DEV), torch.from_numpy(tg).to(DEV))
    assert len(ev._slabs) == 1 and ev._totals.is_cuda          # one zeroed count buffer and one totals tensor for both batches
    S.assert_same_metrics(ev.compute(), S.metrics([b1, b2], col, names))
    S.assert_same_metrics(ev.compute(), S.metrics([b1, b2], col, names))          # compute() twice: the same
    ev.update(torch.from_numpy(b3[0]).to(DEV), torch.from_numpy(b3[1]).to(DEV))   # ... and goes on accumulating
    S.assert_same_metrics(ev.compute(), S.metrics([b1, b2, b3], col, names))
    ev.reset()
    assert ev._totals is None and not ev._slabs and not ev._pending and ev.correct == 0 and ev.seen == 0
    ev.update(torch.from_numpy(b3[0]).to(DEV), torch.from_numpy(b3[1]).to(DEV))
    ref = S.metrics([b3], col, names)
    S.assert_same_metrics(ev.compute(), ref)
    assert ev.correct == ref["correct"] and np.array_equal(ev.seen_class.numpy(), ref["seen_class"])
    # the entry point itself: totals passed again are added to, inter / uni are this batch's alone
    tab = table(col)
    *_, totals = ops.seg_metrics(torch.from_numpy(b1[0]).to(DEV), torch.from_numpy(b1[1]).to(DEV), tab)
    _, _, inter, _, same = ops.seg_metrics(torch.from_numpy(b2[0]).to(DEV), torch.from_numpy(b2[1]).to(DEV), tab, True, totals)
    assert same is totals
    r1, r2 = S.batch_counts(b1[0], b1[1], col), S.batch_counts(b2[0], b2[1], col)
    tot = totals.cpu().numpy()
    assert tot[0] == r1[5] + r2[5] and tot[1] == 0 and np.array_equal(tot[2:52], r1[6] + r2[6]) and np.array_equal(tot[52:], r1[7] + r2[7])
    assert np.array_equal(inter.cpu().numpy(), r2[2])


def test_many_batches_spill_into_a_second_count_buffer(monkeypatch):
    col, names = S.cat_table()
    monkeypatch.setattr(T.SegmentationEvaluator, "_SLAB_SHAPES", 4)
    batches = S.seeded_batches(8, [(["Car", "Guitar", "Cap"], 40)] * 3)           # 4 * B = 12 shapes per buffer: 4, then a new one
    batches += S.seeded_batches(9, [(["Earphone", "Skateboard", "Cap"], 40)] * 3)
    ev, got = evaluator_metrics(batches)
    S.assert_same_metrics(got, S.metrics(batches, col, names))


def guarded_int(numel, dtype, sentinel, lead=300):
    base = torch.full((lead + numel + lead,), sentinel, dtype=dtype, device=DEV)
    return base, base[lead:lead + numel]


def surround_intact(base, numel, sentinel, lead=300):
    return bool((base[:lead] == sentinel).all()) and bool((base[lead + numel:] == sentinel).all())


def test_bad_labels_are_counted_and_write_nothing_out_of_range():
    from prifit_amd import ops
    col, names = S.cat_table()
    (logits, clean), = S.seeded_batches(7, [(["Motorbike", "Bag", "Airplane"], 70)])
    B, N, P = logits.shape
    target = clean.copy()
    target[0, 37] = P                                        # in the middle of a shape
    target[1, 41] = -1

    def launch(tgt, tab):
        pb, pred = guarded_int(B * N, torch.int64, SENT64)
        cb, cat = guarded_int(B, torch.int32, SENT32)
        ib, inter = guarded_int(B * P, torch.int32, SENT32)
        ub, uni = guarded_int(B * P, torch.int32, SENT32)
        inter.zero_()
        uni.zero_()
        out = ops.seg_metrics(torch.from_numpy(logits).to(DEV), torch.from_numpy(tgt).to(DEV), tab, True, None,
                              out=(pred.view(B, N), cat, inter.view(B, P), uni.view(B, P)))
        torch.cuda.synchronize()
        for base, n, s in ((pb, B * N, SENT64), (cb, B, SENT32), (ib, B * P, SENT32), (ub, B * P, SENT32)):
            assert surround_intact(base, n, s)
        return tuple(t.cpu().numpy() for t in out)

    pred, cat, inter, uni, totals = launch(target, table(col))
    r_pred, r_cat = S.batch_counts(logits, clean, col)[:2]            # the arg-max does not look at a row's own label
    ok = (target >= 0) & (target < P)
    assert np.array_equal(pred, r_pred) and np.array_equal(cat, r_cat)
    assert totals[1] == 2 and totals[0] == np.sum(ok & (pred == target))
    for part in range(P):
        assert np.array_equal(inter[:, part], np.sum(ok & (pred == part) & (target == part), 1))
        assert np.array_equal(uni[:, part], np.sum(ok & ((pred == part) | (target == part)), 1))
        assert totals[2 + part] == np.sum(ok & (target == part)) and totals[2 + P + part] == np.sum(ok & (pred == part) & (target == part))
    ev = T.SegmentationEvaluator()
    ev.update(torch.from_numpy(logits).to(DEV), torch.from_numpy(target).to(DEV))
    with pytest.raises(ValueError, match=r"\b2 point"):
        ev.compute()
    # a shape whose FIRST label has no category (here: the Table parts taken out of the table): the reference stops at its
    # lookup; every row of that shape is counted as bad and nothing else, the other shapes are unaffected
    col2 = col.copy()
    col2[47:] = -1
    tgt2 = clean.copy()
    tgt2[1, :] = 47 + (tgt2[1, :] % 3)
    pred, cat, inter, uni, totals = launch(tgt2, table(col2))
    keep = [0, 2]
    r = S.batch_counts(logits[keep], tgt2[keep], col2)
    assert cat.tolist() == [r[1][0], -1, r[1][1]] and np.array_equal(pred[keep], r[0]) and (pred[1] == -1).all()
    assert np.array_equal(inter[keep], r[2]) and np.array_equal(uni[keep], r[3]) and not inter[1].any() and not uni[1].any()
    assert totals[1] == N and totals[0] == r[5] and np.array_equal(totals[2:2 + P], r[6]) and np.array_equal(totals[2 + P:], r[7])


def test_update_does_not_wait_for_the_device():
    """The second update (table uploaded, inputs on the device) runs under torch's sync debug mode "error": any device-to-host
    copy or synchronisation in it would raise."""
    col, names = S.cat_table()
    b1, b2 = S.seeded_batches(10, [(["Lamp", "Mug"], 70), (["Mug", "Earphone"], 70)])
    dev_batches = [(torch.from_numpy(lg).to(DEV), torch.from_numpy(tg).to(DEV)) for lg, tg in (b1, b2)]
    probe = torch.ones(3, device=DEV)
    ev = T.SegmentationEvaluator()
    ev.update(*dev_batches[0])
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.sum().item()
            honoured = False
        except RuntimeError:
            honoured = True
        ev.update(*dev_batches[1])                           # raises here if it waits
    finally:
        torch.cuda.set_sync_debug_mode(before)
    S.assert_same_metrics(ev.compute(), S.metrics([b1, b2], col, names))
    if not honoured:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') did not stop an .item() in this build: the no-wait assertion says nothing")


def test_torch_path_stays_callable_on_the_device():
    """fused=False is the torch path of before, kept for tools/bench_seg_metrics.py: the same numbers to 1e-12 (its sums run in
    another order on the device), the same predictions on rows without ties."""
    col, names = S.cat_table()
    batches = S.seeded_batches(12, [(["Motorbike", "Bag", "Airplane"], 70)])
    ev = T.SegmentationEvaluator(fused=False)
    pred = ev.update(torch.from_numpy(batches[0][0]).to(DEV), torch.from_numpy(batches[0][1]).to(DEV))
    assert not ev._pending and ev.correct > 0
    assert np.array_equal(pred.cpu().numpy(), S.batch_counts(batches[0][0], batches[0][1], col)[0])
    got, ref = ev.compute(), S.metrics(batches, col, names)
    for k in ("accuracy", "class_avg_iou", "instance_avg_iou"):
        assert abs(got[k] - ref[k]) < 1e-12, k

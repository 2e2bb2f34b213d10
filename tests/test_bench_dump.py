"""CPU: `bench.py --dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy, float32 / float64, a
larger array as the same seeded sample in every run, at most bench.DUMP_MAX_BYTES in all."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_each_array(tmp_path):
    rng = np.random.default_rng(3)
    outs = {"loss": np.array([1.25], dtype=np.float64), "seg_log_probs": rng.standard_normal((4, 8, 5)).astype(np.float32)}
    bench.dump_outputs(outs, str(tmp_path / "a"))
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["loss", "seg_log_probs"]
    assert got["loss"].dtype == np.float64 and got["seg_log_probs"].dtype == np.float32
    np.testing.assert_array_equal(got["seg_log_probs"], outs["seg_log_probs"])


def test_dump_outputs_samples_a_large_array_the_same_way(tmp_path):
    big = np.arange(bench.DUMP_MAX_ELEMENTS + 1000, dtype=np.float32).reshape(-1, 8)
    for d in ("a", "b"):
        bench.dump_outputs({"embedding": big}, str(tmp_path / d))
    a, b = np.load(tmp_path / "a" / "embedding.npy"), np.load(tmp_path / "b" / "embedding.npy")
    assert a.shape == (bench.DUMP_MAX_ELEMENTS,) and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0)               # sorted positions of the flattened array
    assert np.array_equal(a, big.reshape(-1)[a.astype(np.int64)])


def test_dump_outputs_refuses_more_than_the_limit(tmp_path):
    n = bench.DUMP_MAX_BYTES // 4 // 8 + 1
    outs = {"x%d" % i: np.zeros(min(n, bench.DUMP_MAX_ELEMENTS), dtype=np.float32) for i in range(8)}
    with pytest.raises(SystemExit):
        bench.dump_outputs(outs, str(tmp_path / "c"))

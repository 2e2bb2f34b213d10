"""CPU: the route functions of the mean-shift clustering path in prifit_amd/fit_ops.py on the shapes of a c3
clustering call -- B = 24 embeddings of N = 2048 points, D = 128, 32 cluster slots, 10 updates -- and on the edge shapes that
change an arm, under the default switches and with each switch changed alone.  The library is not loaded: its shape queries are
answered from a table, the answers of the host-side functions prifit_meanshift_fused_first_supported (csrc/meanshift_fused.hip:
N % 64 == 0, D = 128), prifit_meanshift_split_supported (csrc/meanshift_split.hip: D = 128, N % 256 == 0, N <= 16384, modes
1..3) and prifit_meanshift_rows_supported (csrc/meanshift_rows.hip: D in 32 / 64 / 128, 1..64 rows)."""
import pytest

from prifit_amd import fit_ops as F

N, D, KM = 2048, 128, 32
ANSWERS = {
    ("prifit_meanshift_fused_first_supported", 2048, 128): 1,
    ("prifit_meanshift_fused_first_supported", 200, 128): 0,
    ("prifit_meanshift_fused_first_supported", 333, 128): 0,
    ("prifit_meanshift_split_supported", 2048, 128, 2): 1,
    ("prifit_meanshift_split_supported", 200, 128, 2): 0,
    ("prifit_meanshift_split_supported", 333, 128, 2): 0,
    ("prifit_meanshift_rows_supported", 2048, 128, 32): 1,
    ("prifit_meanshift_rows_supported", 2048, 128, 64): 1,
    ("prifit_meanshift_rows_supported", 200, 128, 32): 1,
    ("prifit_meanshift_rows_supported", 333, 128, 32): 1,
    ("prifit_meanshift_rows_supported", 2048, 64, 32): 1,
}
DEFAULTS = {"BWD_MODE": "hybrid", "DX_STREAMS": False, "MS_BALANCED": True, "CHORD_SYM": True, "FUSE_NMS_OWNER": True,
            "ROWS_BWD": True, "MS_SPLIT": "0", "MS_FIRST_CHORD": True, "MS_ROWS_MODE": "auto", "NMS_MASK": True}


@pytest.fixture
def routes(monkeypatch):
    """Every route of one cluster() call (forward and backward, both engines' plans) per shape, with the switches `changed`."""
    monkeypatch.setattr(F, "query", lambda name, *args: ANSWERS[(name,) + args])    # a question outside the table: KeyError

    def of(n, d, slots=KM):
        return {
            "chord": F._chord_route(True, n, n, d, True, True),       # compute_bandwidth: the embedding against itself
            "engine": F._shift_engine(n, d, slots),
            "forward": F._forward_route(n, d, False, True),           # cluster(): no kernel matrix kept, the chord matrix given
            "forward_kept": F._forward_route(n, d, True, True),       # keep_kernel=True (MeanShiftFn): no split, no chord-first
            "nms": F._nms_route(n, d, True, True),
            "rows_bwd": F.rows_mode(slots),
            "dense_bwd": F._dense_bwd_route(n, d),
        }

    def run(**changed):
        for name, value in dict(DEFAULTS, **changed).items():
            monkeypatch.setattr(F, name, value)
        return {"c3": of(N, D), "n200": of(200, D), "n333": of(333, D), "d64": of(N, 64), "slots64": of(N, D, 64)}
    return run


FUSED = F.ShiftRoute(first="fused", rest="fused", kernel_kept=False)
KEPT = F.ShiftRoute(first="fused", rest="fused", kernel_kept=True)
HYBRID = F.DenseBwdRoute(engine="hybrid", dx="dual", balanced=True)
KT_DUAL = F.DenseBwdRoute(engine="gemm_kt", dx="dual", balanced=False)
KT_TWO = F.DenseBwdRoute(engine="gemm_kt", dx="two", balanced=False)
FLASH = F.DenseBwdRoute(engine="fused", dx=None, balanced=False)
C3 = {"chord": "sym", "engine": "rows", "forward": FUSED._replace(first="chord"), "forward_kept": KEPT, "nms": "mask",
      "rows_bwd": 2, "dense_bwd": HYBRID}
# N % 32 != 0 (and no whole 64-row / 128-row tiles): the general chord product, the float nms, no first update from the chord
# matrix, the GEMM chain on K^T; N % 4 == 0 still lets PRIFIT_MS_BWD=fused in
N200 = dict(C3, chord="gemm", nms="float", forward=FUSED, dense_bwd=KT_TWO)
DEFAULT = {
    "c3": C3,
    "n200": N200,
    "n333": N200,                                                      # N % 4 != 0: the GEMM chain whatever the engine asked for
    "d64": dict(C3, forward=F.ShiftRoute("gemm", "gemm", False), forward_kept=F.ShiftRoute("gemm", "gemm", True),
                dense_bwd=F.DenseBwdRoute(engine="gemm", dx="two", balanced=False)),
    "slots64": dict(C3, rows_bwd=1),
}
SHAPES = sorted(DEFAULT)


def changed_everywhere(**fields):
    return {s: dict(DEFAULT[s], **fields) for s in SHAPES}


def test_routes_of_a_c3_clustering_call_under_the_default_switches(routes):
    assert routes() == DEFAULT


@pytest.mark.parametrize("switch,changed", [
    ({"BWD_MODE": "gemm"}, {"c3": dict(C3, dense_bwd=KT_DUAL), "slots64": dict(DEFAULT["slots64"], dense_bwd=KT_DUAL)}),
    ({"BWD_MODE": "fused"}, {"c3": dict(C3, dense_bwd=FLASH), "slots64": dict(DEFAULT["slots64"], dense_bwd=FLASH),
                             "n200": dict(N200, dense_bwd=FLASH)}),
    ({"DX_STREAMS": True}, {"c3": dict(C3, dense_bwd=HYBRID._replace(dx="streams")),
                            "slots64": dict(DEFAULT["slots64"], dense_bwd=HYBRID._replace(dx="streams"))}),
    # without the symmetric kernel nothing leaves owner keys: nms reads the float matrix twice
    ({"CHORD_SYM": False}, changed_everywhere(chord="gemm", nms="float")),
    ({"FUSE_NMS_OWNER": False}, changed_everywhere(nms="float")),
    ({"NMS_MASK": False}, {"c3": dict(C3, nms="float_owner"), "d64": dict(DEFAULT["d64"], nms="float_owner"),
                           "slots64": dict(DEFAULT["slots64"], nms="float_owner")}),
    ({"ROWS_BWD": False}, changed_everywhere(engine="dense")),
    ({"MS_FIRST_CHORD": False}, {"c3": dict(C3, forward=FUSED), "slots64": dict(DEFAULT["slots64"], forward=FUSED)}),
    # the experiment: whole 256-row blocks, D = 128, and only where the kernel matrix is not kept; no first update from the chord
    ({"MS_SPLIT": "bf16x6"}, {"c3": dict(C3, forward=F.ShiftRoute("split", "split", False)),
                              "slots64": dict(DEFAULT["slots64"], forward=F.ShiftRoute("split", "split", False))}),
    ({"MS_ROWS_MODE": "0"}, changed_everywhere(rows_bwd=0)),
    ({"MS_ROWS_MODE": "1"}, changed_everywhere(rows_bwd=1)),
    ({"MS_ROWS_MODE": "2"}, changed_everywhere(rows_bwd=2)),
])
def test_routes_of_a_c3_clustering_call_with_one_switch_changed(routes, switch, changed):
    assert routes(**switch) == dict(DEFAULT, **changed)


def test_routes_outside_the_clustering_call(routes):
    routes()                                                     # (installs the query table, default switches)
    assert F._forward_route(N, D, False, False) == FUSED         # the caller has no chord matrix
    assert F._chord_route(False, N, N, D, True, True) == "gemm"  # two different sets (nms_pair)
    assert F._chord_route(True, N, N, D, False, True) == "gemm" and F._chord_route(True, N, N, D, True, False) == "gemm"
    assert F._nms_route(N, D, True, False) == "float"            # rows not 16-byte aligned
    assert routes(MS_BALANCED=False)["c3"]["dense_bwd"] == HYBRID._replace(balanced=False)
    assert routes(DX_STREAMS=True)["n200"]["dense_bwd"] == KT_TWO         # the stream-fed dX kernel: hybrid engine, N % 64 == 0


def test_shift_iter_fields_in_the_order_of_the_row_sparse_backward():
    """prifit_meanshift_rows_bwd takes the per-iteration tables Zin, Zout, O, rowsum, nrm: items 0, 4, 2, 3, 5 of a trajectory
    item, which callers outside fit_ops.py (tests, tools) still index by position."""
    assert F.ShiftIter._fields == ("Z", "K", "O", "rowsum", "Zn", "nrm")
    assert [F.ShiftIter._fields[k] for k in (0, 4, 2, 3, 5)] == ["Z", "Zn", "O", "rowsum", "nrm"]
    assert F.Shifted._fields == ("Z", "traj", "Zgrad")
    assert F.Round._fields == ("shapes", "accepted", "X", "bw", "shifted", "ids", "count", "labels", "used")

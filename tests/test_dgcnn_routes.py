"""CPU: the two route functions of prifit_amd/src/dgcnn.py on the shapes of a c5 step -- B = 24 clouds of
N = 2048 points, k = 20 neighbours, the layer widths of DGCNGn -- under the default switches and with each switch off.
The library is not loaded: its shape queries are answered from a table (the answers the library gives for these shapes)."""
import pytest
import torch

from prifit_amd.src import dgcnn as D

B, N, K = 24, 2048, 20
P = B * N
ANSWERS = {
    ("prifit_reduce_rows_per_slab",): 128,
    ("prifit_edge_tables_supported", N, K, 64): 1,
    ("prifit_edge_tables_supported", N, K, 128): 1,
    ("prifit_gemm_stats_tile_m", P, 1024): 128,
    ("prifit_gemm_stats_tile_m", P, 512): 128,
    ("prifit_gemm_stats_tile_m", P, 256): 128,
    ("prifit_gn_finalize_supported", 1024, 8): 1,
    ("prifit_gn_finalize_supported", 512, 8): 1,
    ("prifit_gn_finalize_supported", 256, 4): 1,
    ("prifit_gemm_pool_supported", P, 1024, 256): 1,
    ("prifit_global_pool_winners_supported", 1024, 256): 1,
}
SWITCHES = ["_GN_KERNELS", "_GN_COLSUMS", "_KNN3_FUSED", "_KNN_GRAM_SYM", "_EDGE_LINEARITY", "_EDGE_FUSED_BWD", "_EDGE_TABLES",
            "_GLOBAL_POOL_FUSED", "_GLOBAL_POOL_ALG", "_GLOBAL_POOL_NOSTORE"]


@pytest.fixture
def routes(monkeypatch):
    """The routes of every block of a c5 step, in forward order, with `off` (a switch name or None) set to False."""
    monkeypatch.setattr(D, "query", lambda name, *args: ANSWERS[(name,) + args])    # a question outside the table: KeyError
    x = torch.empty(4, 4)       # (its address: 16-byte aligned, as a [B N, 256] device tensor is)
    assert x.data_ptr() % 16 == 0

    def cfg(groups, pool_K=0):
        return {"groups": groups, "rps": N, "slope": 0.0, "pool_K": pool_K, "eps": 1e-5}

    def run(off=None):
        for name in SWITCHES:
            monkeypatch.setattr(D, name, name != off)
        csr = D._want_csr(N)
        pool_K = N if D._GLOBAL_POOL_FUSED and D.pool_product_ok(P, 1024, 256) else 0
        offset = D._decoder_route(512, 8) == "offset"
        return {
            "dec": D._decoder_route(512, 8),
            "conv1": D._edge_route(N, K, 3, 64, False, csr),
            "conv2": D._edge_route(N, K, 64, 64, False, csr),
            "conv3": D._edge_route(N, K, 64, 128, False, csr),
            "mlp1": D._conv_block_route(P, 1024, 256, cfg(8, pool_K), True, False, x),
            # the decoder: conv1 on the point features with x4's part as an offset, or on upstream's [B N, 1280] rows
            "dec1": D._conv_block_route(P, 512, 256 if offset else 1280, cfg(8), not offset, offset, x),
            "dec2": D._conv_block_route(P, 256, 512, cfg(4), True, False, x),
            "seg1": D._conv_block_route(P, 256, 256, cfg(4), True, False, x),
        }
    return run


PLAIN = D.ConvRoute(tile=128, keep_chsum=True, product="gemm", store_y=True, backward="dense")
PLAIN_TORCH_SUMS = PLAIN._replace(keep_chsum=False)
DEFAULT = {"dec": "offset", "conv1": "tables", "conv2": "tables", "conv3": "tables",
           "mlp1": D.ConvRoute(tile=128, keep_chsum=True, product="pool", store_y=False, backward="alg"),
           "dec1": PLAIN, "dec2": PLAIN, "seg1": PLAIN}


def test_routes_of_a_c5_step_under_the_default_switches(routes):
    assert routes() == DEFAULT


@pytest.mark.parametrize("off,changed", [
    # the statistics' torch form keeps no column sums, and without them the pooled block has no algebraic backward
    ("_GN_KERNELS", {"mlp1": DEFAULT["mlp1"]._replace(keep_chsum=False, store_y=True, backward="dense"),
                     "dec1": PLAIN_TORCH_SUMS, "dec2": PLAIN_TORCH_SUMS, "seg1": PLAIN_TORCH_SUMS}),
    ("_GN_COLSUMS", {"mlp1": DEFAULT["mlp1"]._replace(keep_chsum=False, store_y=True, backward="dense"),
                     "dec1": PLAIN_TORCH_SUMS, "dec2": PLAIN_TORCH_SUMS, "seg1": PLAIN_TORCH_SUMS}),
    # (the decoder's first layer follows the same switch: upstream's concatenated rows, with the bias)
    ("_EDGE_LINEARITY", {"dec": "concat", "conv1": "rows", "conv2": "rows", "conv3": "rows"}),
    ("_EDGE_FUSED_BWD", {"conv1": "linear_unfused", "conv2": "linear_unfused", "conv3": "linear_unfused"}),
    ("_EDGE_TABLES", {"conv1": "linear_fused", "conv2": "linear_fused", "conv3": "linear_fused"}),
    ("_GLOBAL_POOL_FUSED", {"mlp1": PLAIN}),
    ("_GLOBAL_POOL_ALG", {"mlp1": DEFAULT["mlp1"]._replace(store_y=True, backward="dense")}),
    ("_GLOBAL_POOL_NOSTORE", {"mlp1": DEFAULT["mlp1"]._replace(store_y=True)}),
    ("_KNN3_FUSED", {}), ("_KNN_GRAM_SYM", {}),          # the graph's own switches: no block changes its route
])
def test_routes_of_a_c5_step_with_one_switch_off(routes, off, changed):
    assert routes(off) == dict(DEFAULT, **changed)


def test_edge_route_without_the_in_edge_lists_or_outside_the_kernels_limits(routes):
    routes()                                                     # (installs the query table, default switches)
    assert D._edge_route(N, K, 64, 64, False, False) == "linear_fused"      # the lists were not built
    assert D._edge_route(N, K, 64, 64, True, True) == "rows"                # a bias: not by linearity
    assert D._edge_route(100, 3, 64, 64, False, True) == "rows"             # N k is not whole 128-row slabs
    assert not D._want_csr(8193)

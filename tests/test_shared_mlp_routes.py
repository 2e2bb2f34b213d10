"""CPU: the two route functions of the shared-MLP stack in prifit_amd/nn_ops.py, _forward_route and
_backward_route, on every layer of the stacks a c3 step runs -- B = 24 clouds of 2048 points through the MSG part-segmentation
net -- and on the edges that change an arm, under the default switches and with each switch changed alone.  The library is not
loaded: its shape queries are answered from a table, the answers of the host-side functions
  prifit_gemm_stream_supported (csrc/gemm_stream.hip: NT / NN, 32768 <= M < 2^24, N and K in 64 / 96 / 128),
  prifit_gemm_stream_tn_supported (csrc/gemm_stream.hip: Mo, No multiples of 32 in 32..128, 32768 <= P < 2^30, P % 8 == 0),
  prifit_gemm_stream_bwd_supported (csrc/gemm_stream_bwd.hip: P >= 64, [Cout x Cin] one of 128 x 128 / 96 / 64, 96 x 64, 64 x 64;
    pooled: K % 64 == 0, P % K == 0, Cout != 96),
  prifit_gemm_pool_supported (csrc/gemm.hip: N > 96, M % 32 == 0, K % 4 == 0, more than 512 tiles of 128 x 128) and
  prifit_gather_linear_bwd_csr_supported (csrc/sa_gather_bwd.hip: N <= 8192, C <= 128, C even).
The expected backward routes are what _backward_route of the commit before the forward got its plan returned on these inputs;
the expected forward arms were read off the if / elif chain SharedMLPFn.forward had then."""
import types

import pytest

from prifit_amd import nn_ops as N
from prifit_amd.models import pointnet_util as PU

NT, NN = 0, 1
ANSWERS = {
    ("prifit_gather_linear_bwd_csr_supported", 512, 128): 1,
    ("prifit_gemm_pool_supported", 3072, 1024, 512): 0,
    ("prifit_gemm_pool_supported", 196608, 256, 128): 1,
    ("prifit_gemm_pool_supported", 393216, 64, 32): 0,
    ("prifit_gemm_pool_supported", 393216, 128, 64): 1,
    ("prifit_gemm_pool_supported", 393216, 256, 196): 1,
    ("prifit_gemm_pool_supported", 786432, 96, 64): 0,
    ("prifit_gemm_pool_supported", 786432, 128, 64): 1,
    ("prifit_gemm_pool_supported", 1572864, 128, 96): 1,
    ("prifit_gemm_stream_bwd_supported", 49152, 128, 128, 0): 1,
    ("prifit_gemm_stream_bwd_supported", 196608, 128, 128, 0): 1,
    ("prifit_gemm_stream_bwd_supported", 393216, 64, 64, 0): 1,
    ("prifit_gemm_stream_bwd_supported", 786432, 64, 64, 0): 1,
    ("prifit_gemm_stream_bwd_supported", 786432, 128, 64, 64): 1,
    ("prifit_gemm_stream_bwd_supported", 1572864, 96, 64, 0): 1,
    ("prifit_gemm_stream_bwd_supported", 1572864, 128, 96, 128): 1,
    ("prifit_gemm_stream_supported", 0, 3072, 1024, 512): 0,
    ("prifit_gemm_stream_supported", 0, 196608, 256, 128): 0,
    ("prifit_gemm_stream_supported", 0, 393216, 64, 32): 0,
    ("prifit_gemm_stream_supported", 0, 393216, 128, 64): 1,
    ("prifit_gemm_stream_supported", 0, 393216, 256, 196): 0,
    ("prifit_gemm_stream_supported", 0, 786432, 64, 64): 1,
    ("prifit_gemm_stream_supported", 0, 786432, 96, 64): 1,
    ("prifit_gemm_stream_supported", 0, 786432, 128, 64): 1,
    ("prifit_gemm_stream_supported", 0, 1572864, 96, 64): 1,
    ("prifit_gemm_stream_supported", 0, 1572864, 128, 96): 1,
    ("prifit_gemm_stream_supported", 1, 3072, 256, 256): 0,
    ("prifit_gemm_stream_supported", 1, 3072, 256, 512): 0,
    ("prifit_gemm_stream_supported", 1, 3072, 512, 1024): 0,
    ("prifit_gemm_stream_supported", 1, 49152, 128, 128): 1,
    ("prifit_gemm_stream_supported", 1, 196608, 128, 128): 1,
    ("prifit_gemm_stream_supported", 1, 196608, 128, 256): 0,
    ("prifit_gemm_stream_supported", 1, 393216, 32, 32): 0,
    ("prifit_gemm_stream_supported", 1, 393216, 32, 64): 0,
    ("prifit_gemm_stream_supported", 1, 393216, 64, 64): 1,
    ("prifit_gemm_stream_supported", 1, 393216, 64, 128): 1,
    ("prifit_gemm_stream_supported", 1, 393216, 128, 196): 0,
    ("prifit_gemm_stream_supported", 1, 393216, 196, 256): 0,
    ("prifit_gemm_stream_supported", 1, 786432, 64, 64): 1,
    ("prifit_gemm_stream_supported", 1, 786432, 64, 96): 1,
    ("prifit_gemm_stream_supported", 1, 786432, 64, 128): 1,
    ("prifit_gemm_stream_supported", 1, 1572864, 64, 96): 1,
    ("prifit_gemm_stream_supported", 1, 1572864, 96, 128): 1,
    ("prifit_gemm_stream_tn_supported", 64, 64, 393216): 1,
    ("prifit_gemm_stream_tn_supported", 64, 64, 786432): 1,
    ("prifit_gemm_stream_tn_supported", 96, 64, 1572864): 1,
    ("prifit_gemm_stream_tn_supported", 128, 64, 786432): 1,
    ("prifit_gemm_stream_tn_supported", 128, 96, 1572864): 1,
    ("prifit_gemm_stream_tn_supported", 128, 128, 49152): 1,
    ("prifit_gemm_stream_tn_supported", 128, 128, 196608): 1,
}
DEFAULTS = {"_STREAM": True, "_FUSE_RED": True, "_FUSE_POOL_FWD": True, "_FUSE_BN_APPLY": True, "_FUSE_POOL": True,
            "_FUSE_BWD": "auto", "_GATHER_BWD_CSR": True}

B, S1, S2 = 24, 512, 128
SA1 = {32: ((32, 0), (32, 32), (64, 32)), 64: ((64, 0), (64, 64), (128, 64)), 128: ((64, 0), (96, 64), (128, 96))}
SA2 = {64: ((128, 0), (128, 128), (256, 128)), 128: ((128, 0), (196, 128), (256, 196))}
FP1 = ((128, 152), (128, 128))
# name: (P, pool_K, mode, ((Cout, Kin) per layer), what differs from a stack whose every operand is aligned and dense)
STACKS = {
    "sa1_k32": (B * S1 * 32, 32, "direct", SA1[32], {}),
    "sa1_k64": (B * S1 * 64, 64, "direct", SA1[64], {}),
    "sa1_k128": (B * S1 * 128, 128, "direct", SA1[128], {}),
    "sa1_k64_norows": (B * S1 * 64, 64, "norows", SA1[64], {}),
    "sa1_k128_norows": (B * S1 * 128, 128, "norows", SA1[128], {}),
    "sa2_k64": (B * S2 * 64, 64, "gather", SA2[64], {"N0": S1}),
    "sa2_k128": (B * S2 * 128, 128, "gather", SA2[128], {"N0": S1}),
    "group_all": (B * S2, S2, "plain", ((256, 516), (512, 256), (1024, 512)), {"need_dx": True}),
    "fp3": (B * S2, 0, "plain", ((256, 1536), (256, 256)), {"need_dx": True}),
    "fp1": (B * 2048, 0, "plain", FP1, {"need_dx": True}),
    "head": (B * 2048, 0, "plain", ((128, 128),), {"need_dx": True}),
    # the edges
    "k32": (B * S1 * 32, 32, "direct", SA1[64], {}),                                  # pool_K 32 on the 64-sample scale's widths
    "cout96": (B * S1 * 64, 64, "direct", ((64, 0), (64, 64), (96, 64)), {}),         # a 96-wide pooled layer
    "unaligned": (B * S1 * 64, 64, "direct", SA1[64], {"aligned": False}),
    "sa2_wide_gradient": (B * S2 * 64, 64, "gather", SA2[64], {"N0": S1, "g_contig": False}),
    "fp1_no_dx": (B * 2048, 0, "plain", FP1, {"need_dx": False}),
    "fp1_no_dw": (B * 2048, 0, "plain", FP1, {"need_dx": True, "need_dW": False}),
    "fp1_g_strided": (B * 2048, 0, "plain", FP1, {"need_dx": True, "g_dense": False}),
    "fp1_below_ld": (B * 2048, 0, "plain", FP1, {"need_dx": True, "below_ld4": False}),
    "sa1_k64_below_ld": (B * S1 * 64, 64, "direct", SA1[64], {"below_ld4": False}),
    "sa1_k64_eval": (B * S1 * 64, 64, "preact", SA1[64], {"training": False}),       # (eval mode: SAGroupDirectFn's rows)
    "fp1_eval": (B * 2048, 0, "plain", FP1, {"need_dx": True, "training": False}),
}
NOROWS_NEEDS = ("_STREAM", "_FUSE_RED", "_FUSE_BN_APPLY")   # pointnet_util._norows_scales: no norows stack without them


def layer_routes(P, pool_K, mode, dims, edge):
    """Per layer "forward arm / backward route:kernel[+red]", as SharedMLPFn.forward and .backward ask for them."""
    e = dict({"training": True, "need_dW": True, "need_dx": False, "g_dense": True, "g_contig": True, "below_ld4": True,
              "aligned": True, "N0": 0}, **edge)
    L, out = len(dims), []
    for l, (Cout, Kin) in enumerate(dims):
        fwd = N._forward_route(l, L, P, Cout, Kin, pool_K, e["training"], mode, e["aligned"], l > 0)
        assert fwd.cand == (fwd.arm in ("stream_pool", "tiled_pool"))
        assert fwd.slab == {"preact": "front", "eval": None}.get(fwd.arm, "launch")
        stored_below = l > 0 and not (l == 1 and mode == "norows")
        bwd = N._backward_route(l, L, P, Cout, Kin, pool_K, e["training"], mode, e["need_dW"], e["need_dx"], e["g_dense"],
                                e["g_contig"], stored_below and e["below_ld4"], e["N0"])
        out.append("%s / %s:%s%s" % (fwd.arm, bwd.name, bwd.kernel, "+red" if bwd.red else ""))
    return out


@pytest.fixture
def routes(monkeypatch):
    def table(name, *args):
        return ANSWERS[(name,) + args]                              # a question outside the table: KeyError

    monkeypatch.setattr(N, "query", table)
    monkeypatch.setattr(PU, "query", table)

    def run(**changed):
        for name, value in dict(DEFAULTS, **changed).items():
            monkeypatch.setattr(N, name, value)
        norows = all(getattr(N, s) for s in NOROWS_NEEDS)
        return {k: layer_routes(*v) for k, v in STACKS.items() if norows or v[2] != "norows"}
    return run


DEFAULT = {
    "sa1_k32": ["preact / direct0:rows", "gemm / plain:tiled+red", "gemm / plain:tiled+red"],
    "sa1_k64": ["preact / direct0:rows", "gemm / bn:one_pass+red", "stream_pool / pool:pair+red"],
    "sa1_k128": ["preact / direct0:rows", "gemm / bn:one_pass+red", "stream_pool / pool:pair+red"],
    "sa1_k64_norows": ["preact / direct0:gather", "norows_gather / norows:one_pass+red", "stream_pool / pool:pair+red"],
    "sa1_k128_norows": ["preact / direct0:gather", "norows_gather / norows:one_pass+red", "stream_pool / pool:pair+red"],
    "sa2_k64": ["preact / gather0:csr", "gemm / bn:one_pass+red", "tiled_pool / plain:tiled+red"],
    "sa2_k128": ["preact / gather0:csr", "gemm / plain:tiled+red", "tiled_pool / plain:tiled+red"],
    "group_all": ["gemm / plain:gemm", "gemm / plain:tiled+red", "gemm / plain:tiled+red"],
    "fp3": ["gemm / plain:gemm", "gemm / plain:tiled+red"],
    "fp1": ["gemm / plain:gemm", "gemm / bn:one_pass+red"],
    "head": ["gemm / plain:gemm"],
    "k32": ["preact / direct0:rows", "gemm / bn:one_pass+red", "stream_pool / plain:stream+red"],
    "cout96": ["preact / direct0:rows", "gemm / bn:one_pass+red", "stream_pool / plain:stream+red"],
    "unaligned": ["preact / direct0:rows", "gemm / bn:one_pass+red", "gemm / pool:pair+red"],
    "sa2_wide_gradient": ["preact / gather0:atomic", "gemm / bn:one_pass+red", "tiled_pool / plain:tiled+red"],
    "fp1_no_dx": ["gemm / plain:None", "gemm / bn:one_pass+red"],
    "fp1_no_dw": ["gemm / plain:gemm", "gemm / plain:stream+red"],
    "fp1_g_strided": ["gemm / plain:gemm", "gemm / plain:stream+red"],
    "fp1_below_ld": ["gemm / plain:gemm", "gemm / bn:pair+red"],
    "sa1_k64_below_ld": ["preact / direct0:rows", "gemm / bn:pair+red", "stream_pool / pool:pair+red"],
    "sa1_k64_eval": ["preact / preact0:None", "eval / plain:stream+red", "eval / plain:stream+red"],
    "fp1_eval": ["eval / plain:gemm", "eval / plain:stream+red"],
}


def without_norows(table):
    return {k: v for k, v in table.items() if STACKS[k][2] != "norows"}


def test_routes_of_a_c3_step_under_the_default_switches(routes):
    assert routes() == DEFAULT


@pytest.mark.parametrize("switch,changed", [
    ({"_STREAM": False}, {
        "sa1_k64": ["preact / direct0:rows", "gemm / plain:tiled+red", "tiled_pool / plain:tiled+red"],
        "sa1_k128": ["preact / direct0:rows", "gemm / plain:tiled+red", "tiled_pool / plain:tiled+red"],
        "sa2_k64": ["preact / gather0:csr", "gemm / plain:tiled+red", "tiled_pool / plain:tiled+red"],
        "fp1": ["gemm / plain:gemm", "gemm / plain:tiled+red"],
        "k32": ["preact / direct0:rows", "gemm / plain:tiled+red", "tiled_pool / plain:tiled+red"],
        "cout96": ["preact / direct0:rows", "gemm / plain:tiled+red", "gemm / plain:tiled+red"],
        "unaligned": ["preact / direct0:rows", "gemm / plain:tiled+red", "gemm / plain:tiled+red"],
        "sa2_wide_gradient": ["preact / gather0:atomic", "gemm / plain:tiled+red", "tiled_pool / plain:tiled+red"],
        "fp1_no_dx": ["gemm / plain:None", "gemm / plain:tiled+red"],
        "fp1_no_dw": ["gemm / plain:gemm", "gemm / plain:tiled+red"],
        "fp1_g_strided": ["gemm / plain:gemm", "gemm / plain:tiled+red"],
        "fp1_below_ld": ["gemm / plain:gemm", "gemm / plain:tiled+red"],
        "sa1_k64_below_ld": ["preact / direct0:rows", "gemm / plain:tiled+red", "tiled_pool / plain:tiled+red"],
        "sa1_k64_eval": ["preact / preact0:None", "eval / plain:tiled+red", "eval / plain:tiled+red"],
        "fp1_eval": ["eval / plain:gemm", "eval / plain:tiled+red"],
    }),
    ({"_FUSE_RED": False}, {
        "sa1_k32": ["preact / direct0:rows", "gemm / plain:gemm", "gemm / plain:gemm"],
        "sa1_k64": ["preact / direct0:rows", "gemm / plain:gemm", "stream_pool / pool:pair"],
        "sa1_k128": ["preact / direct0:rows", "gemm / plain:gemm", "stream_pool / pool:pair"],
        "sa2_k64": ["preact / gather0:csr", "gemm / plain:gemm", "tiled_pool / plain:gemm"],
        "sa2_k128": ["preact / gather0:csr", "gemm / plain:gemm", "tiled_pool / plain:gemm"],
        "group_all": ["gemm / plain:gemm", "gemm / plain:gemm", "gemm / plain:gemm"],
        "fp3": ["gemm / plain:gemm", "gemm / plain:gemm"],
        "fp1": ["gemm / plain:gemm", "gemm / plain:gemm"],
        "k32": ["preact / direct0:rows", "gemm / plain:gemm", "stream_pool / plain:gemm"],
        "cout96": ["preact / direct0:rows", "gemm / plain:gemm", "stream_pool / plain:gemm"],
        "unaligned": ["preact / direct0:rows", "gemm / plain:gemm", "gemm / pool:pair"],
        "sa2_wide_gradient": ["preact / gather0:atomic", "gemm / plain:gemm", "tiled_pool / plain:gemm"],
        "fp1_no_dx": ["gemm / plain:None", "gemm / plain:gemm"],
        "fp1_no_dw": ["gemm / plain:gemm", "gemm / plain:gemm"],
        "fp1_g_strided": ["gemm / plain:gemm", "gemm / plain:gemm"],
        "fp1_below_ld": ["gemm / plain:gemm", "gemm / plain:gemm"],
        "sa1_k64_below_ld": ["preact / direct0:rows", "gemm / plain:gemm", "stream_pool / pool:pair"],
        "sa1_k64_eval": ["preact / preact0:None", "eval / plain:gemm", "eval / plain:gemm"],
        "fp1_eval": ["eval / plain:gemm", "eval / plain:gemm"],
    }),
    ({"_FUSE_POOL_FWD": False}, {
        "sa1_k64": ["preact / direct0:rows", "gemm / bn:one_pass+red", "gemm / pool:pair+red"],
        "sa1_k128": ["preact / direct0:rows", "gemm / bn:one_pass+red", "gemm / pool:pair+red"],
        "sa1_k64_norows": ["preact / direct0:gather", "norows_gather / norows:one_pass+red", "gemm / pool:pair+red"],
        "sa1_k128_norows": ["preact / direct0:gather", "norows_gather / norows:one_pass+red", "gemm / pool:pair+red"],
        "sa2_k64": ["preact / gather0:csr", "gemm / bn:one_pass+red", "gemm / plain:tiled+red"],
        "sa2_k128": ["preact / gather0:csr", "gemm / plain:tiled+red", "gemm / plain:tiled+red"],
        "k32": ["preact / direct0:rows", "gemm / bn:one_pass+red", "gemm / plain:stream+red"],
        "cout96": ["preact / direct0:rows", "gemm / bn:one_pass+red", "gemm / plain:stream+red"],
        "sa2_wide_gradient": ["preact / gather0:atomic", "gemm / bn:one_pass+red", "gemm / plain:tiled+red"],
        "sa1_k64_below_ld": ["preact / direct0:rows", "gemm / bn:pair+red", "gemm / pool:pair+red"],
    }),
    ({"_FUSE_BN_APPLY": False}, {
        "sa1_k64": ["preact / direct0:rows", "gemm / plain:stream+red", "stream_pool / pool:pair+red"],
        "sa1_k128": ["preact / direct0:rows", "gemm / plain:stream+red", "stream_pool / pool:pair+red"],
        "sa2_k64": ["preact / gather0:csr", "gemm / plain:stream+red", "tiled_pool / plain:tiled+red"],
        "fp1": ["gemm / plain:gemm", "gemm / plain:stream+red"],
        "k32": ["preact / direct0:rows", "gemm / plain:stream+red", "stream_pool / plain:stream+red"],
        "cout96": ["preact / direct0:rows", "gemm / plain:stream+red", "stream_pool / plain:stream+red"],
        "unaligned": ["preact / direct0:rows", "gemm / plain:stream+red", "gemm / pool:pair+red"],
        "sa2_wide_gradient": ["preact / gather0:atomic", "gemm / plain:stream+red", "tiled_pool / plain:tiled+red"],
        "fp1_no_dx": ["gemm / plain:None", "gemm / plain:stream+red"],
        "fp1_below_ld": ["gemm / plain:gemm", "gemm / plain:stream+red"],
        "sa1_k64_below_ld": ["preact / direct0:rows", "gemm / plain:stream+red", "stream_pool / pool:pair+red"],
    }),
    ({"_FUSE_POOL": False}, {
        "sa1_k64": ["preact / direct0:rows", "gemm / bn:one_pass+red", "stream_pool / plain:stream+red"],
        "sa1_k128": ["preact / direct0:rows", "gemm / bn:one_pass+red", "stream_pool / plain:stream+red"],
        "sa1_k64_norows": ["preact / direct0:gather", "norows_gather / norows:one_pass+red", "stream_pool / plain:stream+red"],
        "sa1_k128_norows": ["preact / direct0:gather", "norows_gather / norows:one_pass+red", "stream_pool / plain:stream+red"],
        "unaligned": ["preact / direct0:rows", "gemm / bn:one_pass+red", "gemm / plain:stream+red"],
        "sa1_k64_below_ld": ["preact / direct0:rows", "gemm / bn:pair+red", "stream_pool / plain:stream+red"],
    }),
    ({"_FUSE_BWD": "0"}, {
        "sa1_k64": ["preact / direct0:rows", "gemm / bn:pair+red", "stream_pool / pool:pair+red"],
        "sa1_k128": ["preact / direct0:rows", "gemm / bn:pair+red", "stream_pool / pool:pair+red"],
        "sa2_k64": ["preact / gather0:csr", "gemm / bn:pair+red", "tiled_pool / plain:tiled+red"],
        "fp1": ["gemm / plain:gemm", "gemm / bn:pair+red"],
        "k32": ["preact / direct0:rows", "gemm / bn:pair+red", "stream_pool / plain:stream+red"],
        "cout96": ["preact / direct0:rows", "gemm / bn:pair+red", "stream_pool / plain:stream+red"],
        "unaligned": ["preact / direct0:rows", "gemm / bn:pair+red", "gemm / pool:pair+red"],
        "sa2_wide_gradient": ["preact / gather0:atomic", "gemm / bn:pair+red", "tiled_pool / plain:tiled+red"],
        "fp1_no_dx": ["gemm / plain:None", "gemm / bn:pair+red"],
    }),
    ({"_FUSE_BWD": "1"}, {
        "sa1_k64": ["preact / direct0:rows", "gemm / bn:one_pass+red", "stream_pool / pool:one_pass+red"],
        "sa1_k128": ["preact / direct0:rows", "gemm / bn:one_pass+red", "stream_pool / pool:one_pass+red"],
        "sa1_k64_norows": ["preact / direct0:gather", "norows_gather / norows:one_pass+red", "stream_pool / pool:one_pass+red"],
        "sa1_k128_norows": ["preact / direct0:gather", "norows_gather / norows:one_pass+red", "stream_pool / pool:one_pass+red"],
        "unaligned": ["preact / direct0:rows", "gemm / bn:one_pass+red", "gemm / pool:one_pass+red"],
    }),
    ({"_GATHER_BWD_CSR": False}, {
        "sa2_k64": ["preact / gather0:atomic", "gemm / bn:one_pass+red", "tiled_pool / plain:tiled+red"],
        "sa2_k128": ["preact / gather0:atomic", "gemm / plain:tiled+red", "tiled_pool / plain:tiled+red"],
    }),
])
def test_routes_of_a_c3_step_with_one_switch_changed(routes, switch, changed):
    base = DEFAULT if all(switch.get(s, True) for s in NOROWS_NEEDS) else without_norows(DEFAULT)
    assert set(changed) <= set(base)
    assert routes(**switch) == dict(base, **changed)


def test_norows_needs_what_norows_scales_checks(routes, monkeypatch):
    """_backward_route asserts that layer 1 above unstored rows gets the one-pass streaming backward.  What makes that hold is
    the precondition of pointnet_util._norows_scales, the only place that hands out mode "norows": the three switches, a
    64-wide first layer, whole 64-row tiles per centre, >= 3 layers, and layer 2 on the streaming forward and one-pass backward
    kernels.  Without any one of the switches it offers no scale, and the route would raise."""
    blocks = [[types.SimpleNamespace(weight=types.SimpleNamespace(shape=(cout, kin if kin else 6, 1, 1))) for cout, kin in SA1[K]]
              for K in (32, 64, 128)]
    monkeypatch.setattr(PU, "_SA_NOROWS", True)
    routes()
    assert PU._norows_scales(blocks, B, S1, [32, 64, 128]) == [False, True, True]
    assert PU._norows_scales([blocks[1][:2]], B, S1, [64]) == [False]                       # two layers
    for switch in NOROWS_NEEDS:
        routes(**{switch: False})
        assert PU._norows_scales(blocks, B, S1, [32, 64, 128]) == [False, False, False]
        with pytest.raises(AssertionError, match="norows"):
            layer_routes(*STACKS["sa1_k64_norows"])
    routes()
    with pytest.raises(AssertionError, match="norows"):                                     # eval mode: SAGroupDirectFn's job
        N._forward_route(1, 3, B * S1 * 64, 64, 64, 64, False, "norows", False, True)
    with pytest.raises(AssertionError, match="norows"):
        N._forward_route(1, 2, B * S1 * 64, 64, 64, 64, True, "norows", False, True)


def test_records_carry_the_fields_their_readers_name():
    assert N._FwdRoute._fields == ("arm", "slab", "cand") and N._Route._fields == ("name", "kernel", "red")
    assert set(N._FWD_ARMS) == {"preact", "eval", "norows_gather", "stream_pool", "tiled_pool", "gemm"}
    assert set(N._ROUTES) == {"pool", "bn", "norows", "direct0", "gather0", "preact0", "plain"}
    assert N._SavedLayer._fields == ("Y", "W", "scale", "shift", "mean", "invstd")
    assert N._SavedStack._fields == ("layers", "x", "arg", "P", "dev", "mode", "front", "bias0", "cfg")

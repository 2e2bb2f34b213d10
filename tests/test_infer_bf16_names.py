"""CPU: the names frozen inference in bf16 adds -- the precision argument of `freeze` / `FrozenPartSeg`, the bf16 entry points
in the header and in the built library, their shape queries (host functions: no device needed) and the argument checks that
return before a launch."""
import ctypes
import inspect

import pytest

from prifit_amd import _lib

ENTRY_POINTS = ("prifit_pack_bf16_multi", "prifit_pack_bf16_max_jobs",
                "prifit_mlp_chain_pool_bf16", "prifit_mlp_chain_pool_bf16_supported", "prifit_mlp_chain_pool_bf16_workspace",
                "prifit_mlp_chain_rows_bf16", "prifit_mlp_chain_rows_bf16_supported", "prifit_mlp_chain_rows_bf16_workspace")
POOL_SHAPES = [(32, 32, 64), (64, 64, 128), (64, 96, 128), (128, 128, 256), (128, 196, 256)]


def _widths(*w):
    return (ctypes.c_int32 * len(w))(*w)


def test_header_declares_and_library_exports_the_entry_points(hiplib):
    declared = _lib.declared_symbols()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    for name in ENTRY_POINTS:
        assert name in declared and hasattr(hiplib, name), name
    sigs = _lib._signatures()
    # njobs, w, rows, cols, ldw, order, out, stream
    assert sigs["prifit_pack_bf16_multi"] == [I, P, P, P, P, P, P, P]
    assert sigs["prifit_pack_bf16_max_jobs"] == []
    # the fp32 entry points' parameter lists, slot for slot
    for name in ("prifit_mlp_chain_pool", "prifit_mlp_chain_rows"):
        assert sigs[name + "_bf16"] == sigs[name + "_f32"]
        assert sigs[name + "_bf16_supported"] == sigs[name + "_supported"]
        assert sigs[name + "_bf16_workspace"] == sigs[name + "_workspace"]
        assert getattr(hiplib, name + "_bf16_workspace").restype is ctypes.c_longlong
    assert sigs["prifit_mlp_chain_pool_bf16"] == [P, LL, I, I, I, I, I, P, LL, P, P, LL, P, P, LL, P, P]
    assert sigs["prifit_mlp_chain_rows_bf16"] == [P, LL, LL, I, I, P, P, P, P, P, LL, P, P, P, I, P, P]
    assert _lib.abi_version() >= 802 and hiplib.prifit_version(None) == _lib.abi_version()


def test_shape_queries(hiplib):
    pool = hiplib.prifit_mlp_chain_pool_bf16_supported
    for C0, C1, C2 in POOL_SHAPES:
        for K in (32, 64, 128):
            assert pool(C0, C1, C2, K) == 1, (C0, C1, C2, K)
            assert hiplib.prifit_mlp_chain_pool_bf16_workspace(1536, K, C0, C1, C2) == 0
        for K in (0, 16, 48, 256):
            assert pool(C0, C1, C2, K) == 0, (C0, C1, C2, K)
    assert pool(64, 96, 256, 64) == 0
    assert pool(64, 128, 128, 64) == 0
    assert pool(256, 512, 1024, 128) == 0
    rows = hiplib.prifit_mlp_chain_rows_bf16_supported
    for K0 in range(8, 161, 8):
        for CL in (1, 33, 50, 64):
            assert rows(K0, 4, _widths(128, 128, 128, CL)) == 1, (K0, CL)
    assert hiplib.prifit_mlp_chain_rows_bf16_workspace(49152, 152, 4, _widths(128, 128, 128, 50)) == 0
    assert rows(4, 4, _widths(128, 128, 128, 50)) == 0
    assert rows(0, 4, _widths(128, 128, 128, 50)) == 0
    assert rows(156, 4, _widths(128, 128, 128, 50)) == 0
    assert rows(168, 4, _widths(128, 128, 128, 50)) == 0
    assert rows(152, 4, _widths(128, 128, 128, 65)) == 0
    assert rows(152, 4, _widths(128, 128, 128, 0)) == 0
    assert rows(152, 4, _widths(128, 96, 128, 50)) == 0
    assert rows(152, 3, _widths(128, 128, 50)) == 0
    assert rows(152, 4, None) == 0


def test_pack_refuses_bad_jobs_without_a_launch(hiplib):
    most = hiplib.prifit_pack_bf16_max_jobs()
    assert most >= 14                                      # 5 scales x 2 layers + 4 tail layers in one launch
    p = 256                                                # any non-NULL 16-byte aligned address: never followed
    pack = hiplib.prifit_pack_bf16_multi

    def args(n, **kw):
        a = dict(n=n, w=(ctypes.c_void_p * n)(*[p] * n), rows=_widths(*[128] * n), cols=_widths(*[152] * n), ldw=_widths(*[152] * n),
                 order=_widths(*[1] * n), out=(ctypes.c_void_p * n)(*[p] * n), stream=None)
        a.update(kw)
        return list(a.values())

    assert pack(*args(most + 1)) != 0                      # one job more than the table holds
    assert pack(*args(0)[:1] + args(1)[1:]) != 0
    two = lambda *v: _widths(*v)
    bad = [dict(w=None), dict(w=(ctypes.c_void_p * 2)(p, None)), dict(out=None), dict(out=(ctypes.c_void_p * 2)(p, 264)),
           dict(rows=two(128, 0)), dict(cols=two(0, 152)), dict(ldw=two(152, 148)), dict(order=two(0, 2)), dict(order=two(-1, 0)),
           dict(rows=None), dict(cols=None), dict(ldw=None), dict(order=None)]
    for kw in bad:
        assert pack(*args(2, **kw)) != 0, kw


def test_chains_reject_bad_arguments_without_a_launch(hiplib):
    p = 256
    pool = hiplib.prifit_mlp_chain_pool_bf16

    def pargs(**kw):
        a = dict(X=p, ldx=128, G=3, K=128, C0=128, C1=196, C2=256, W1=p, ldw1=128, b1=p, W2=p, ldw2=208, b2=p, out=p, ldo=256,
                 ws=None, stream=None)
        a.update(kw)
        return list(a.values())

    for kw in [dict(X=None), dict(X=260), dict(ldx=124), dict(G=0), dict(K=16), dict(C1=192), dict(W1=None), dict(W1=264),
               dict(ldw1=120), dict(ldw1=132), dict(W2=None), dict(ldw2=196), dict(ldw2=200), dict(ldw2=212), dict(b1=None),
               dict(b2=260), dict(out=None), dict(ldo=252)]:
        assert pool(*pargs(**kw)) != 0, kw
    rows = hiplib.prifit_mlp_chain_rows_bf16
    ptrs = lambda *v: (ctypes.c_void_p * 4)(*v)
    lds = lambda *v: (ctypes.c_longlong * 4)(*v)

    def rargs(**kw):
        a = dict(X=p, ldx=152, P=200, K0=152, L=4, widths=_widths(128, 128, 128, 50), W=ptrs(p, p, p, p), ldw=lds(160, 128, 128, 128),
                 b=ptrs(p, p, p, p), scores=p, lds=50, labels=p, cat=p, shape_cat=p, N=100, ws=None, stream=None)
        a.update(kw)
        return list(a.values())

    for kw in [dict(X=None), dict(ldx=148), dict(P=0), dict(P=1 << 31), dict(K0=156), dict(K0=4, ldx=4), dict(L=3),
               dict(widths=_widths(128, 128, 128, 65)), dict(W=None), dict(W=ptrs(p, None, p, p)), dict(W=ptrs(p, p, 264, p)),
               dict(ldw=lds(152, 128, 128, 128)), dict(ldw=lds(160, 128, 132, 128)), dict(ldw=lds(160, 128, 128, 120)), dict(b=None),
               dict(b=ptrs(p, p, p, None)), dict(scores=None, labels=None), dict(lds=49), dict(cat=None), dict(N=0), dict(N=96)]:
        assert rows(*rargs(**kw)) != 0, kw


def test_freeze_takes_a_precision():
    from prifit_amd import inference
    from prifit_amd.models import pointnet2_part_seg_msg as M
    for fn in (inference.freeze, inference.FrozenPartSeg.__init__):
        params = inspect.signature(fn).parameters
        assert list(params)[-2:] == ["model", "precision"] and params["precision"].default == "fp32"
    net = M.get_model(50, normal_channel=False)
    for bad in ("int8", "fp16", "BF16", None):
        with pytest.raises(ValueError):
            inference.freeze(net, precision=bad)
        with pytest.raises(ValueError):
            inference.FrozenPartSeg(net, precision=bad)

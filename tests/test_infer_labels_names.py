"""CPU: the names the frozen label route adds -- `FrozenPartSeg.labels`, the row-chain entry points in the header and in the
built library, their shape query (a host function: no device needed) and the argument checks that return before a launch."""
import ctypes
import inspect

from prifit_amd import _lib

ENTRY_POINTS = ("prifit_mlp_chain_rows_f32", "prifit_mlp_chain_rows_supported", "prifit_mlp_chain_rows_workspace")


def _widths(*w):
    return (ctypes.c_int32 * len(w))(*w)


def test_header_declares_and_library_exports_the_entry_points(hiplib):
    declared = _lib.declared_symbols()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    for name in ENTRY_POINTS:
        assert name in declared and hasattr(hiplib, name), name
    sigs = _lib._signatures()
    # X, ldx, P, K0, L, widths, W, ldw, b, scores, lds, labels, cat_of_label, shape_cat, rows_per_shape, workspace, stream
    assert sigs["prifit_mlp_chain_rows_f32"] == [P, LL, LL, I, I, P, P, P, P, P, LL, P, P, P, I, P, P]
    assert sigs["prifit_mlp_chain_rows_supported"] == [I, I, P]
    assert sigs["prifit_mlp_chain_rows_workspace"] == [LL, I, I, P]
    assert hiplib.prifit_mlp_chain_rows_workspace.restype is ctypes.c_longlong


def test_shape_query(hiplib):
    sup = hiplib.prifit_mlp_chain_rows_supported
    for K0 in (152, 160):
        for CL in range(1, 65):
            assert sup(K0, 4, _widths(128, 128, 128, CL)) == 1, (K0, CL)
        assert hiplib.prifit_mlp_chain_rows_workspace(49152, K0, 4, _widths(128, 128, 128, 50)) == 0
    assert sup(156, 4, _widths(128, 128, 128, 50)) == 0          # K0 % 8 != 0
    assert sup(168, 4, _widths(128, 128, 128, 50)) == 0          # K0 > 160
    assert sup(0, 4, _widths(128, 128, 128, 50)) == 0
    assert sup(152, 4, _widths(128, 96, 128, 50)) == 0
    assert sup(152, 4, _widths(96, 128, 128, 50)) == 0
    assert sup(152, 4, _widths(128, 128, 128, 65)) == 0
    assert sup(152, 4, _widths(128, 128, 128, 0)) == 0
    assert sup(152, 3, _widths(128, 128, 50)) == 0
    assert sup(152, 5, _widths(128, 128, 128, 128, 50)) == 0
    assert sup(152, 4, None) == 0


def test_launch_rejects_bad_arguments_without_a_launch(hiplib):
    p = 256                                                # any non-NULL 16-byte aligned address: never followed
    ptrs = lambda *v: (ctypes.c_void_p * 4)(*v)
    lds = lambda *v: (ctypes.c_longlong * 4)(*v)
    chain = hiplib.prifit_mlp_chain_rows_f32

    def args(**kw):
        a = dict(X=p, ldx=152, P=200, K0=152, L=4, widths=_widths(128, 128, 128, 50), W=ptrs(p, p, p, p), ldw=lds(152, 128, 128, 128),
                 b=ptrs(p, p, p, p), scores=p, lds=50, labels=p, cat=p, shape_cat=p, N=100, ws=None, stream=None)
        a.update(kw)
        return list(a.values())

    bad = [dict(X=None), dict(X=260), dict(ldx=148), dict(ldx=154), dict(P=0), dict(P=1 << 31), dict(K0=156), dict(L=3),
           dict(widths=_widths(128, 128, 128, 65)), dict(widths=_widths(128, 96, 128, 50)), dict(widths=None), dict(W=None),
           dict(W=ptrs(p, None, p, p)), dict(W=ptrs(p, p, 260, p)), dict(ldw=None), dict(ldw=lds(148, 128, 128, 128)),
           dict(ldw=lds(152, 128, 130, 128)), dict(ldw=lds(152, 128, 128, 124)), dict(b=None), dict(b=ptrs(p, p, p, None)),
           dict(b=ptrs(264, p, p, p)), dict(scores=None, labels=None), dict(lds=49), dict(cat=None), dict(shape_cat=None),
           dict(N=0), dict(N=-4), dict(N=96)]              # 200 % 96 != 0
    for kw in bad:
        assert chain(*args(**kw)) != 0, kw


def test_labels_is_a_method_of_the_frozen_model():
    from prifit_amd import inference
    params = inspect.signature(inference.FrozenPartSeg.labels).parameters
    assert list(params) == ["self", "xyz", "cls_label", "shape_cat", "cat_of_label", "fps_start", "return_scores"]
    assert params["shape_cat"].default is None and params["cat_of_label"].default is None
    assert params["fps_start"].default is None and params["return_scores"].default is False
    # forward() and predict() keep their parameter lists
    assert list(inspect.signature(inference.FrozenPartSeg.predict).parameters) == ["self", "xyz", "cls_label", "fps_start"]

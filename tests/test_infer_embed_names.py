"""CPU: the names the frozen embedding route adds -- `FrozenPartSeg.embed`, the six embedding-chain entry points in the header
and in the built library, and their shape queries (host functions: no device needed)."""
import ctypes
import inspect

from prifit_amd import _lib

ENTRY_POINTS = ("prifit_mlp_chain_embed_f32", "prifit_mlp_chain_embed_supported", "prifit_mlp_chain_embed_workspace",
                "prifit_mlp_chain_embed_bf16", "prifit_mlp_chain_embed_bf16_supported", "prifit_mlp_chain_embed_bf16_workspace")


def _widths(*w):
    return (ctypes.c_int32 * len(w))(*w)


def test_header_declares_and_library_exports_the_entry_points(hiplib):
    declared = _lib.declared_symbols()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    for name in ENTRY_POINTS:
        assert name in declared and hasattr(hiplib, name), name
    sigs = _lib._signatures()
    # X, ldx, P, K0, L, widths, W, ldw, b, W_cls, ldw_cls, b_cls, CL, emb, lde, normalize, scores, lds, labels, cat_of_label,
    # shape_cat, rows_per_shape, workspace, stream
    launch = [P, LL, LL, I, I, P, P, P, P, P, LL, P, I, P, LL, I, P, LL, P, P, P, I, P, P]
    for stem in ("prifit_mlp_chain_embed", "prifit_mlp_chain_embed_bf16"):
        assert sigs[stem + ("_f32" if stem.endswith("embed") else "")] == launch
        assert sigs[stem + "_supported"] == [I, I, P, I]
        assert sigs[stem + "_workspace"] == [LL, I, I, P, I]
        assert getattr(hiplib, stem + "_workspace").restype is ctypes.c_longlong
    assert _lib.abi_version() >= 805 and hiplib.prifit_version(None) == _lib.abi_version()


def test_shape_query(hiplib):
    for sup, ws in ((hiplib.prifit_mlp_chain_embed_supported, hiplib.prifit_mlp_chain_embed_workspace),
                    (hiplib.prifit_mlp_chain_embed_bf16_supported, hiplib.prifit_mlp_chain_embed_bf16_workspace)):
        w = _widths(128, 128, 128, 128)
        for K0 in (8, 152, 160):
            for CL in range(0, 65):
                assert sup(K0, 4, w, CL) == 1, (K0, CL)
            assert ws(49152, K0, 4, w, 50) == 0
        assert sup(156, 4, w, 50) == 0          # K0 % 8 != 0
        assert sup(168, 4, w, 50) == 0          # K0 > 160
        assert sup(0, 4, w, 50) == 0
        assert sup(152, 4, w, 65) == 0
        assert sup(152, 4, w, -1) == 0
        assert sup(152, 4, _widths(128, 96, 128, 128), 50) == 0
        assert sup(152, 4, _widths(128, 128, 128, 50), 50) == 0      # the last width is the embedding's, not C_L
        assert sup(152, 4, _widths(128, 128, 128, 64), 0) == 0
        assert sup(152, 3, _widths(128, 128, 128), 50) == 0
        assert sup(152, 5, _widths(128, 128, 128, 128, 128), 50) == 0
        assert sup(152, 4, None, 50) == 0


def test_embed_is_a_method_of_the_frozen_model():
    from prifit_amd import inference
    params = inspect.signature(inference.FrozenPartSeg.embed).parameters
    assert list(params) == ["self", "xyz", "cls_label", "fps_start", "l2_norm", "shape_cat", "cat_of_label", "return_labels"]
    for name in ("fps_start", "l2_norm", "shape_cat", "cat_of_label"):
        assert params[name].default is None, name
    assert params["return_labels"].default is False
    assert inference._CHAINS["fp32"]["embed"][0] == "prifit_mlp_chain_embed_f32"
    assert inference._CHAINS["bf16"]["embed"][0] == "prifit_mlp_chain_embed_bf16"
    # the other methods keep their parameter lists
    assert list(inspect.signature(inference.FrozenPartSeg.predict).parameters) == ["self", "xyz", "cls_label", "fps_start"]
    assert list(inspect.signature(inference.FrozenPartSeg.labels).parameters) == \
        ["self", "xyz", "cls_label", "shape_cat", "cat_of_label", "fps_start", "return_scores"]

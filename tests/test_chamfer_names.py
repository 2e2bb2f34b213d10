"""CPU: the point-set Chamfer functions of the reference's src/utils.py:271-358 resolve through the reference's module path
with the reference's parameter names and defaults, and the C ABI declares their kernels (tests/test_library_abi.py then
checks that the library exports them and that every call site passes as many arguments as the header declares)."""
import importlib
import inspect
import sys

from prifit_amd import _lib

EXPECTED = {
    "chamfer_distance": [("pred", inspect.Parameter.empty), ("gt", inspect.Parameter.empty), ("sqrt", False)],
    "chamfer_distance_one_side": [("pred", inspect.Parameter.empty), ("gt", inspect.Parameter.empty), ("side", 1)],
    "chamfer_distance_single_shape": [("pred", inspect.Parameter.empty), ("gt", inspect.Parameter.empty), ("one_side", False),
                                      ("sqrt", False), ("reduce", True)],
    "chamfer_distance_kdtree": [("source_points", inspect.Parameter.empty), ("target_points", inspect.Parameter.empty),
                                ("sqrt", False)],
}


def test_reference_names_and_defaults():
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k.split(".")[0] in ("models", "src", "convex_loss")}
    try:
        from prifit_amd import compat
        compat.install()
        ut = importlib.import_module("src.utils")
        assert ut.__name__.startswith("prifit_amd.")
        for name, want in EXPECTED.items():
            fn = getattr(ut, name)
            got = [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
            assert got == want, (name, got)
            assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in inspect.signature(fn).parameters.values())
    finally:
        for k in list(sys.modules):
            if k.split(".")[0] in ("models", "src", "convex_loss"):
                del sys.modules[k]
        sys.modules.update({k: v for k, v in saved.items() if v is not None})


def test_header_declares_the_entry_points():
    sigs = _lib._signatures()
    assert len(sigs["prifit_chamfer_nn_workspace_floats"]) == 3
    assert len(sigs["prifit_chamfer_nn_fwd"]) == 11      # a, b, na, nb, B, NA, NB, d2, idx, workspace, stream
    assert len(sigs["prifit_chamfer_nn_bwd"]) == 13      # a, b, na, nb, B, NA, NB, idx, g, ga, gb, accumulate_b, stream
    assert _lib._declared()["prifit_chamfer_nn_workspace_floats"] == "long long"
    assert _lib.abi_version() >= 300                     # the parameter lists above first appear in 0.3.0

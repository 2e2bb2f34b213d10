"""CPU: the names the classifier-layer pre-training adds -- the probe-head entry points in the header and in the built
library, their shape and workspace queries (host functions: no device needed), the argument checks that return before a
launch, and the Python surface (FrozenPartSeg.probe_step, Trainer.init_classifier, train_step.train_init_class)."""
import ctypes
import inspect

from prifit_amd import _lib

ENTRY_POINTS = ("prifit_probe_head_f32", "prifit_probe_head_supported", "prifit_probe_head_workspace")


def _widths(*w):
    return (ctypes.c_int32 * len(w))(*w)


def test_header_declares_and_library_exports_the_entry_points(hiplib):
    declared = _lib.declared_symbols()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    for name in ENTRY_POINTS:
        assert name in declared and hasattr(hiplib, name), name
    sigs = _lib._signatures()
    # X, ldx, P, K0, L, widths, W, ldw, b, target, dW, lddw, db, loss, workspace, stream
    assert sigs["prifit_probe_head_f32"] == [P, LL, LL, I, I, P, P, P, P, P, P, LL, P, P, P, P]
    assert sigs["prifit_probe_head_supported"] == [I, I, P]
    assert sigs["prifit_probe_head_workspace"] == [LL, I, I, P]
    assert hiplib.prifit_probe_head_workspace.restype is ctypes.c_longlong
    # the existing row chain keeps its contract
    assert sigs["prifit_mlp_chain_rows_f32"] == [P, LL, LL, I, I, P, P, P, P, P, LL, P, P, P, I, P, P]
    assert hiplib.prifit_mlp_chain_rows_workspace(49152, 152, 4, _widths(128, 128, 128, 50)) == 0


def test_shape_query_answers_as_the_rows_query(hiplib):
    sup, rows = hiplib.prifit_probe_head_supported, hiplib.prifit_mlp_chain_rows_supported
    cases = [(K0, 4, _widths(128, 128, 128, CL)) for K0 in (8, 64, 152, 160) for CL in range(1, 65)]
    cases += [(156, 4, _widths(128, 128, 128, 50)), (168, 4, _widths(128, 128, 128, 50)), (0, 4, _widths(128, 128, 128, 50)),
              (152, 4, _widths(128, 96, 128, 50)), (152, 4, _widths(96, 128, 128, 50)), (152, 4, _widths(128, 128, 128, 65)),
              (152, 4, _widths(128, 128, 128, 0)), (152, 3, _widths(128, 128, 50)), (152, 5, _widths(128, 128, 128, 128, 50)),
              (152, 4, None)]
    for c in cases:
        assert sup(*c) == rows(*c), c[:2]
    assert sup(152, 4, _widths(128, 128, 128, 50)) == 1 and sup(156, 4, _widths(128, 128, 128, 50)) == 0


def test_workspace_does_not_grow_with_the_rows(hiplib):
    ws = hiplib.prifit_probe_head_workspace
    w = _widths(128, 128, 128, 50)
    part = 64 * 128 + 64 + 4                               # a workgroup's partial: dW, db, three scalars (+ one reserved)
    assert ws(49152, 152, 4, w) == ws(10 ** 6, 152, 4, w) == 256 * part > 0
    assert ws(1, 152, 4, w) == part and ws(129, 152, 4, w) == 2 * part and ws(128 * 256 + 40, 160, 4, w) == 256 * part
    assert ws(49152, 156, 4, w) == 0                       # an unsupported shape


def test_launch_rejects_bad_arguments_without_a_launch(hiplib):
    p = 256                                                # any non-NULL 16-byte aligned address: never followed
    ptrs = lambda *v: (ctypes.c_void_p * 4)(*v)
    lds = lambda *v: (ctypes.c_longlong * 4)(*v)
    head = hiplib.prifit_probe_head_f32

    def args(**kw):
        a = dict(X=p, ldx=152, P=200, K0=152, L=4, widths=_widths(128, 128, 128, 50), W=ptrs(p, p, p, p), ldw=lds(152, 128, 128, 128),
                 b=ptrs(p, p, p, p), target=p, dW=p, lddw=128, db=p, loss=p, ws=p, stream=None)
        a.update(kw)
        return list(a.values())

    # what the rows chain rejects ...
    bad = [dict(X=None), dict(X=260), dict(ldx=148), dict(ldx=154), dict(P=0), dict(P=1 << 31), dict(K0=156), dict(L=3),
           dict(widths=_widths(128, 128, 128, 65)), dict(widths=_widths(128, 96, 128, 50)), dict(widths=None), dict(W=None),
           dict(W=ptrs(p, None, p, p)), dict(W=ptrs(p, p, 260, p)), dict(W=ptrs(p, p, p, 260)), dict(ldw=None),
           dict(ldw=lds(148, 128, 128, 128)), dict(ldw=lds(152, 128, 130, 128)), dict(ldw=lds(152, 128, 128, 124)), dict(b=None),
           dict(b=ptrs(p, p, p, None)), dict(b=ptrs(264, p, p, p)),
           # ... and the head's own
           dict(target=None), dict(dW=None), dict(db=None), dict(loss=None), dict(lddw=127), dict(lddw=0), dict(dW=264),
           dict(ws=None)]
    for kw in bad:
        assert head(*args(**kw)) != 0, kw


def test_python_surface():
    from prifit_amd import inference, train_step
    params = inspect.signature(inference.FrozenPartSeg.probe_step).parameters
    assert list(params) == ["self", "xyz", "cls_label", "target", "fps_start"] and params["fps_start"].default is None
    # labels(), forward() and predict() keep their parameter lists
    assert list(inspect.signature(inference.FrozenPartSeg.labels).parameters) == \
        ["self", "xyz", "cls_label", "shape_cat", "cat_of_label", "fps_start", "return_scores"]
    assert list(inspect.signature(inference.FrozenPartSeg.predict).parameters) == ["self", "xyz", "cls_label", "fps_start"]
    assert list(inspect.signature(inference.FrozenPartSeg.forward).parameters) == \
        ["self", "xyz", "cls_label", "fps_start", "include_convex_loss", "embed", "ignored_forward_kwargs"]
    params = inspect.signature(train_step.Trainer.init_classifier).parameters
    assert list(params) == ["self", "batches", "epochs", "lr", "momentum", "augment", "log"]
    assert [params[k].default for k in list(params)[2:]] == [500, 0.1, 0.5, True, None]
    params = inspect.signature(train_step.train_init_class).parameters
    assert list(params) == ["classifier", "criterion", "trainDataLoader", "num_classes", "num_part", "num_epoch"]
    assert params["num_epoch"].default == 500

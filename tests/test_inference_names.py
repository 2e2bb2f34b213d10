"""CPU: the names frozen inference adds -- `prifit_amd.inference.freeze` / `FrozenPartSeg`, the fold and chain entry points in
the header and in the built library, their shape queries (host functions: no device needed) -- and freeze()'s refusal of every
network but the MSG part-segmentation one."""
import ctypes
import inspect

import pytest

from prifit_amd import _lib

ENTRY_POINTS = ("prifit_fold_bn", "prifit_fold_bn_max_jobs", "prifit_mlp_chain_pool_f32", "prifit_mlp_chain_pool_supported",
                "prifit_mlp_chain_pool_workspace")
CHAIN_SHAPES = [(32, 32, 64, 32), (64, 64, 128, 64), (64, 96, 128, 128), (128, 128, 256, 64), (128, 196, 256, 128)]


def test_module_exposes_freeze_and_frozen_part_seg():
    from prifit_amd import inference
    import torch.nn as nn
    assert callable(inference.freeze) and issubclass(inference.FrozenPartSeg, nn.Module)
    params = inspect.signature(inference.FrozenPartSeg.forward).parameters
    assert list(params)[:4] == ["self", "xyz", "cls_label", "fps_start"] and params["include_convex_loss"].default is False
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())      # the live model's other keywords
    for name in ("predict", "refresh"):
        assert callable(getattr(inference.FrozenPartSeg, name))


def test_header_declares_and_library_exports_the_entry_points(hiplib):
    declared = _lib.declared_symbols()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    for name in ENTRY_POINTS:
        assert name in declared and hasattr(hiplib, name), name
    sigs = _lib._signatures()
    # X, ldx, G, pool_K, C0, C1, C2, W1, ldw1, b1, W2, ldw2, b2, out, ldo, workspace, stream
    assert sigs["prifit_mlp_chain_pool_f32"] == [P, LL, I, I, I, I, I, P, LL, P, P, LL, P, P, LL, P, P]
    # njobs, W, cout, kin, bias, gamma, beta, mean, var, eps, w_off, ldw, b_off, flat, flat_len, stream
    assert sigs["prifit_fold_bn"] == [I, P, P, P, P, P, P, P, P, P, P, P, P, P, LL, P]
    assert hiplib.prifit_mlp_chain_pool_workspace.restype is ctypes.c_longlong
    assert _lib.abi_version() >= 800


def test_shape_queries(hiplib):
    sup = hiplib.prifit_mlp_chain_pool_supported
    for C0, C1, C2, K in CHAIN_SHAPES:
        assert sup(C0, C1, C2, K) == 1                      # every SA1 / SA2 scale: the chain kernel lost on none of them
        assert sup(C0, C1, C2, 0) == 0 and sup(C0, C1, C2, 48) == 0
        assert hiplib.prifit_mlp_chain_pool_workspace(3, K, C0, C1, C2) >= 0
    assert sup(256, 512, 1024, 128) == 0 and sup(64, 64, 64, 64) == 0 and sup(128, 196, 128, 128) == 0
    assert hiplib.prifit_fold_bn_max_jobs() >= 27          # every layer of the MSG part-segmentation network in one launch


def test_entry_points_reject_bad_arguments_without_a_launch(hiplib):
    p = 256                                                # any non-NULL 16-byte aligned address: never followed
    chain = hiplib.prifit_mlp_chain_pool_f32
    ok = [p, 32, 3, 32, 32, 32, 64, p, 32, p, p, 32, p, p, 64, None, None]
    for at, bad in ((3, 0), (3, 48), (4, 40), (2, 0), (1, 30), (1, 34), (8, 28), (11, 30), (14, 63), (0, None), (0, 260), (13, None)):
        a = list(ok)
        a[at] = bad
        assert chain(*a) != 0, (at, bad)
    assert chain(p, 1024, 3, 128, 256, 512, 1024, p, 256, p, p, 512, p, p, 1024, None, None) != 0
    assert hiplib.prifit_fold_bn(0, p, p, p, p, p, p, p, p, p, p, p, p, p, 64, None) != 0
    assert hiplib.prifit_fold_bn(hiplib.prifit_fold_bn_max_jobs() + 1, p, p, p, p, p, p, p, p, p, p, p, p, p, 64, None) != 0


def test_freeze_refuses_other_networks():
    import torch.nn as nn
    from prifit_amd import inference
    from prifit_amd.models import pointnet2_cls_ssg, pointnet2_part_seg_msg, pointnet2_part_seg_ssg
    for other in (pointnet2_part_seg_ssg.get_model(50), pointnet2_cls_ssg.get_model(40, normal_channel=False), nn.Linear(3, 3)):
        with pytest.raises(TypeError):
            inference.freeze(other)
    with pytest.raises(TypeError):
        inference.freeze(pointnet2_part_seg_msg.get_model(50, reconstruct=True))

"""reconstruct=True without a GPU: the module tree, the state_dict keys and the parameter count of upstream
(models/pointnet2_part_seg_msg.py:60-62, models/reconstruction.py:8-70), the compat alias, the declared entry points, and the
restatement of tests/atlas_common.py against what the reference itself returned (tests/golden/atlas_decoder.npz, fp64)."""
import sys

import numpy as np
import pytest
import torch

import atlas_common as ac


@pytest.fixture(scope="module")
def net():
    from prifit_amd.models.pointnet2_part_seg_msg import get_model
    return get_model(50, reconstruct=True)


def test_builds_with_upstream_names(net):
    keys = set(net.state_dict())
    for i in (0, 24):
        for l in (1, 2, 3, 4):
            for leaf in ("weight", "bias"):
                assert "atlasnet.decoder.%d.conv%d.%s" % (i, l, leaf) in keys
        for l in (1, 2, 3):
            for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
                assert "atlasnet.decoder.%d.bn%d.%s" % (i, l, leaf) in keys
    assert "atlasnet.decoder.25.conv1.weight" not in keys
    assert not any("reg_grid" in k for k in keys)
    assert not any(k.startswith("chamferdistance") for k in keys) and hasattr(net, "chamferdistance")
    assert list(net.chamferdistance.parameters()) == []


def test_parameter_count(net):
    from prifit_amd.models.pointnet2_part_seg_msg import get_model
    assert sum(p.numel() for p in net.parameters()) == 2462720
    assert sum(p.numel() for p in get_model(50).parameters()) == 1757470
    assert sum(p.numel() for p in net.atlasnet.decoder[3].parameters()) == 28210
    shapes = {k: tuple(v.shape) for k, v in net.atlasnet.decoder[0].state_dict().items()}
    assert shapes["conv1.weight"] == (130, 130, 1) and shapes["conv2.weight"] == (65, 130, 1)
    assert shapes["conv3.weight"] == (32, 65, 1) and shapes["conv4.weight"] == (3, 32, 1)


def test_extra_layers_still_raises():
    from prifit_amd.models.pointnet2_part_seg_msg import get_model
    with pytest.raises(NotImplementedError):
        get_model(50, extra_layers=True)
    with pytest.raises(NotImplementedError):
        get_model(50, reconstruct=True, extra_layers=True)


def test_constructor_arguments():
    from prifit_amd.models.reconstruction import AtlasNet, PointGenCon
    a = AtlasNet(num_charts=2, num_points=9)
    assert a.grid_size == 3 and len(a.decoder) == 2 and tuple(a.reg_grid.shape) == (1, 2, 9)
    grid, g = ac.grid_of(9)
    assert g == 3 and np.array_equal(a.reg_grid[0].numpy(), grid)
    assert PointGenCon(bottleneck_size=130).conv3.weight.shape == (32, 65, 1)
    for bad in (0, 1, 3):
        with pytest.raises(ValueError):
            AtlasNet(num_points=bad)


def test_compat_alias():
    import prifit_amd.compat as compat
    assert "models.reconstruction" in compat.install()
    import importlib
    mod = importlib.import_module("models.reconstruction")
    assert mod is sys.modules["prifit_amd.models.reconstruction"]
    for name in ("PointGenCon", "AtlasNet", "ChamferDistance"):
        assert hasattr(mod, name)


def test_header_declares_entry_points():
    from prifit_amd import _lib
    sigs = _lib._signatures()
    assert len(sigs["prifit_atlas_workspace_floats"]) == 4
    assert len(sigs["prifit_atlas_fwd"]) == 12 and len(sigs["prifit_atlas_bwd"]) == 14
    assert _lib._declared()["prifit_atlas_workspace_floats"] == "long long"
    assert _lib.abi_version() >= 400


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("B,C,npts,seed", ac.GOLDEN_CASES)
def test_restatement_matches_reference(golden, B, C, npts, seed):
    """the fp64 restatement against the reference's own fp64 run, 1e-10 relative per tensor"""
    G = golden("atlas_decoder")
    tag = "%d_%d_%d|" % (B, C, npts)
    z, target = ac.make_inputs(seed, B)
    res = ac.evaluate(ac.make_state(seed, C), z, target, npts, C, torch.float64)
    assert res["out"].shape == G[tag + "out"].shape == (B, C * int(np.sqrt(npts)) ** 2, 3)
    assert rel(res["out"], G[tag + "out"]) < 1e-10
    assert rel(res["loss"], G[tag + "loss"]) < 1e-10
    assert rel(res["gz"], G[tag + "gz"]) < 1e-10
    mom, want = ac.grad_moments(res, C), G[tag + "grad_moments"]
    # the biases in front of a batch-statistics BatchNorm have a gradient of rounding noise on both sides: their sums of
    # squares are compared on the scale of the weight gradient of the same layer
    for a, name in enumerate(ac.PARAM_ORDER):
        scale = np.abs(want[a - 1 if name in ("conv1.bias", "conv2.bias", "conv3.bias") else a]).max()
        assert np.abs(mom[a] - want[a]).max() <= 1e-10 * scale, name
    for l in (1, 2, 3):
        for leaf in ("running_mean", "running_var"):
            assert rel(res["decoder.0.bn%d.%s" % (l, leaf)], G[tag + "bn%d.%s" % (l, leaf)]) < 1e-10


def test_restatement_matches_reference_eval(golden):
    B, C, npts, seed = ac.GOLDEN_EVAL
    z, _ = ac.make_inputs(seed, B)
    L = ac.leaves(ac.make_state(seed, C), torch.float64)
    with torch.no_grad():
        out, _ = ac.decoder(L, torch.from_numpy(z).double(), npts, C, training=False)
    assert rel(out.numpy(), golden("atlas_decoder")["eval|out"]) < 1e-10

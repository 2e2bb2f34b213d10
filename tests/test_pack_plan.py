"""CPU: `pack_plan(net)` is re-entrant -- a forward of a net inside its own forward (activation checkpointing, embed() inside
forward) must hand the outer forward its packed weights back.  Needs the library's pure query entry points only."""
import torch
import torch.nn as nn

from prifit_amd.models import pointnet_util as pu


def test_pack_plan_nested_for_the_same_net(hiplib):
    net = nn.Conv2d(6, 8, 1)
    w = net.weight.reshape(8, 6)
    cols = (3, 4, 5, 0, 1, 2, -1, -1)
    with pu.pack_plan(net) as outer:
        marker = torch.zeros(1)
        outer.results[(id(net.weight), cols)] = marker          # what the outer forward's one launch produced
        with pu.pack_plan(net) as inner:
            assert inner is outer and pu._active_plan is outer
            assert inner.results == {}                          # the inner forward starts on its own results
        assert pu._active_plan is outer
        assert outer.lookup(w, cols) is marker                  # the outer forward goes on: no AttributeError, its own results
        assert outer.lookup(w, (0, 1, 2, 3, 4, 5, -1, -1)) is None and len(outer.sites) == 1   # a new site joins the plan
    assert pu._active_plan is None and outer.results is None
    assert outer.lookup(w, cols) is None                        # outside any forward: a miss, not an exception

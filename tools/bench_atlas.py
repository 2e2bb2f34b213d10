"""Times the AtlasNet decoder + reconstruction loss, forward and backward, at B = 24, N = 2048, 25 charts of 11 x 11 points:
the chart-batched HIP path (models/reconstruction.py) against the same network written as plain torch modules here.
Prints device launches and milliseconds per iteration for both.

    python tools/bench_atlas.py [--B 24] [--N 2048] [--charts 25] [--iters 20]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from prifit_amd.models.reconstruction import AtlasNet, ChamferDistance  # noqa: E402


class TorchChart(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1, self.conv2, self.conv3, self.conv4 = (nn.Conv1d(130, 130, 1), nn.Conv1d(130, 65, 1), nn.Conv1d(65, 32, 1),
                                                          nn.Conv1d(32, 3, 1))
        self.bn1, self.bn2, self.bn3 = nn.BatchNorm1d(130), nn.BatchNorm1d(65), nn.BatchNorm1d(32)

    def forward(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        x = F.relu(self.bn3(self.conv3(x)))
        return torch.tanh(self.conv4(x))


class TorchAtlas(nn.Module):
    def __init__(self, charts, grid):
        super().__init__()
        self.decoder = nn.ModuleList([TorchChart() for _ in range(charts)])
        self.grid = grid

    def forward(self, z):
        B, P = z.shape[0], self.grid.shape[1]
        x = torch.cat([self.grid.unsqueeze(0).expand(B, 2, P), z.unsqueeze(2).expand(B, 128, P)], dim=1).contiguous()
        return torch.cat([m(x) for m in self.decoder], dim=2).transpose(1, 2).contiguous()


def torch_loss(out, target):
    d = torch.cdist(out, target) ** 2
    return d.min(dim=2)[0].mean() + d.min(dim=1)[0].mean()


def measure(step, iters):
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    launches = -1
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as e:       # the figure is optional; the time is not
        print("launch count unavailable:", e)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        step()
    t1.record()
    torch.cuda.synchronize()
    return launches, t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=24)
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--charts", type=int, default=25)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    z = torch.from_numpy(rng.standard_normal((a.B, 128)).astype(np.float32)).cuda().requires_grad_(True)
    target = torch.from_numpy((rng.random((a.B, a.N, 3)) * 2 - 1).astype(np.float32)).cuda()
    torch.manual_seed(0)
    ours = AtlasNet(num_charts=a.charts, num_points=128).cuda().train()
    ref = TorchAtlas(a.charts, ours.reg_grid[0].cuda()).cuda().train()
    ref.load_state_dict(ours.state_dict())
    cd = ChamferDistance()

    def step_ours():
        ours.zero_grad(set_to_none=True); z.grad = None
        cd(ours(z), target).backward()

    def step_ref():
        ref.zero_grad(set_to_none=True); z.grad = None
        torch_loss(ref(z), target).backward()

    for name, step in (("hip", step_ours), ("torch", step_ref)):
        n, ms = measure(step, a.iters)
        print("%-6s B=%d N=%d charts=%d: %d device launches, %.3f ms per forward+backward" % (name, a.B, a.N, a.charts, n, ms))


if __name__ == "__main__":
    main()

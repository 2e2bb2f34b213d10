"""AtlasNet decoder and reconstruction loss of the reference's models/reconstruction.py (PointGenCon :8-29, AtlasNet :32-70,
ChamferDistance :157-166) on the MI355X backend: same constructor arguments, sub-module / parameter names (checkpoint
compatible) and output tensors.

Upstream runs the charts one after the other: per chart a [B,130,P] input (128 of its 130 channels a broadcast of z), four 1x1
convolutions and three training-mode BatchNorms -- several hundred small launches each way for 25 charts.  Here all charts go
through csrc/atlas.hip in 5 launches forward and 5 backward, whatever the chart count and B are.  The
per-chart modules only own the parameters; their addresses reach the kernels through a device pointer table, so they stay
ordinary nn.Parameters (views of the flat Adam buffer once FlatAdam owns them).

get_rec_selfsup_loss and the second get_model of the upstream file are not provided."""
import math

import numpy as np
import torch
import torch.nn as nn

from .. import fit_ops
from .._lib import call, cur_stream, ptr, query, require_cuda

LATENT = 128                  # the decoder kernels are built for bottleneck_size = 128 (130 -> 130 -> 65 -> 32 -> 3)
_NPTR = 24                    # pointers per chart in the parameter table (include/prifit_hip.h)
_NPARAM = 28210               # parameters per chart


class PointGenCon(nn.Module):
    """One chart's MLP (upstream :8-29).  Owns the parameters; the arithmetic of all charts runs in AtlasNet.forward."""

    def __init__(self, bottleneck_size=2500):
        self.bottleneck_size = bottleneck_size
        super().__init__()
        self.conv1 = nn.Conv1d(bottleneck_size, bottleneck_size, 1)
        self.conv2 = nn.Conv1d(bottleneck_size, bottleneck_size // 2, 1)
        self.conv3 = nn.Conv1d(bottleneck_size // 2, bottleneck_size // 4, 1)
        self.conv4 = nn.Conv1d(bottleneck_size // 4, 3, 1)
        self.th = nn.Tanh()
        self.bn1 = nn.BatchNorm1d(bottleneck_size)
        self.bn2 = nn.BatchNorm1d(bottleneck_size // 2)
        self.bn3 = nn.BatchNorm1d(bottleneck_size // 4)

    def trainable(self):
        """The parameters in the order of a chart's gradient block (prifit_atlas_bwd)."""
        return [self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias, self.conv3.weight, self.conv3.bias,
                self.conv4.weight, self.conv4.bias, self.bn1.weight, self.bn1.bias, self.bn2.weight, self.bn2.bias,
                self.bn3.weight, self.bn3.bias]

    def table_row(self):
        """The tensors of a chart's row of the parameter table, in the order of include/prifit_hip.h."""
        row = [self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias, self.conv3.weight, self.conv3.bias,
               self.conv4.weight, self.conv4.bias]
        for bn in (self.bn1, self.bn2, self.bn3):
            row += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        return row + [self.bn1.num_batches_tracked, self.bn2.num_batches_tracked, self.bn3.num_batches_tracked]

    def forward(self, x):
        raise NotImplementedError("PointGenCon holds one chart's parameters; the decoder of all charts runs in AtlasNet.forward")


class AtlasDecoderFn(torch.autograd.Function):
    """z [B,128] -> output_points [B, num_charts * P, 3] through csrc/atlas.hip; the trainable parameters of every chart are
    inputs (PointGenCon.trainable() order, chart after chart) so that autograd hands them their gradients."""

    @staticmethod
    def forward(ctx, net, z, *params):
        require_cuda(z)
        if z.dtype != torch.float32 or z.dim() != 2 or z.shape[1] != LATENT:
            raise ValueError("AtlasNet: z [B,%d] float32 expected, got %s %s" % (LATENT, tuple(z.shape), z.dtype))
        z = z.contiguous()
        C, P, B = net.nb_primitives, net.grid_size * net.grid_size, z.shape[0]
        training = bool(net.training)
        if training and B * P < 2:
            raise ValueError("AtlasNet: training-mode BatchNorm needs more than one value per channel")
        table, grid = net._table(z.device), net._grid(z.device)
        bn = net.decoder[0].bn1
        out = torch.empty(B, C * P, 3, dtype=torch.float32, device=z.device)
        ws = torch.empty(query("prifit_atlas_workspace_floats", C, B, P, 0), dtype=torch.float32, device=z.device)
        call("prifit_atlas_fwd", ptr(table), ptr(z), ptr(grid), C, B, P, int(training), float(bn.eps), float(bn.momentum),
             ptr(out), ptr(ws), cur_stream())
        ctx.save_for_backward(z, out, ws, table, grid, *params)
        ctx.meta = (C, B, P, training, [tuple(p.shape) for p in params[:14]])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        z, out, ws, table, grid = ctx.saved_tensors[:5]
        C, B, P, training, shapes = ctx.meta
        dev = z.device
        gz = torch.empty_like(z)
        gparams = torch.empty(C, _NPARAM, dtype=torch.float32, device=dev)
        scratch = torch.empty(query("prifit_atlas_workspace_floats", C, B, P, 1), dtype=torch.float32, device=dev)
        call("prifit_atlas_bwd", ptr(table), ptr(z), ptr(grid), C, B, P, int(training), ptr(gout.contiguous()), ptr(out),
             ptr(ws), ptr(scratch), ptr(gz), ptr(gparams), cur_stream())
        grads, off = [], 0
        for shape in shapes:
            n = math.prod(shape)
            col = gparams[:, off:off + n]
            grads.append([col[c].view(shape) for c in range(C)])
            off += n
        return (None, gz) + tuple(grads[i][c] for c in range(C) for i in range(14))


class AtlasNet(nn.Module):
    """upstream :32-70: `num_charts` MLPs, each mapping a regular g x g grid of the unit square (g = int(sqrt(num_points)))
    plus the latent z to g * g points."""

    def __init__(self, bottleneck_size=128, num_charts=25, num_points=128):
        super().__init__()
        if bottleneck_size != LATENT:
            raise NotImplementedError("AtlasNet: the decoder kernels are built for bottleneck_size = %d, got %r"
                                      % (LATENT, bottleneck_size))
        if num_points < 4:
            raise ValueError("AtlasNet: num_points >= 4 needed (a grid of at least 2 x 2), got %r" % (num_points,))
        if num_charts < 1:
            raise ValueError("AtlasNet: num_charts >= 1 needed, got %r" % (num_charts,))
        self.nb_primitives = num_charts
        self.num_points = num_points
        self.decoder = nn.ModuleList([PointGenCon(bottleneck_size=2 + bottleneck_size) for _ in range(num_charts)])
        g = int(np.sqrt(num_points))
        self.grid_size = g
        grid = np.indices((g, g)).T.reshape(-1, 2).T.astype("float32") / (g - 1)      # point n: (n % g, n // g) / (g - 1)
        self.reg_grid = torch.from_numpy(grid).unsqueeze(0)       # plain attribute as upstream: not in the state_dict
        self._tab = (None, None)
        self._grid_dev = None

    def _grid(self, device):
        if self._grid_dev is None or self._grid_dev.device != device:
            self._grid_dev = self.reg_grid[0].to(device).contiguous()
        return self._grid_dev

    def _table(self, device):
        """Device table of the parameter and buffer addresses, uploaded again only when one of them moved (FlatAdam adopting
        the parameters, module.to())."""
        addrs = []
        for m in self.decoder:
            row = m.table_row()
            for t in row:
                if t.device != device or not t.is_contiguous() or (t.dtype != torch.float32 and t.dtype != torch.int64):
                    raise RuntimeError("AtlasNet: parameters and buffers must be contiguous tensors on %s" % (device,))
            addrs += [t.data_ptr() for t in row] + [0] * (_NPTR - len(row))
        key = tuple(addrs)
        if self._tab[0] != key:
            self._tab = (key, torch.tensor(addrs, dtype=torch.int64).to(device))
        return self._tab[1]

    def forward(self, z):
        params = [p for m in self.decoder for p in m.trainable()]
        return AtlasDecoderFn.apply(self, z, *params)


class ChamferDistance(nn.Module):
    """upstream :157-166: mean over all B * N of the squared distance to the nearest y + mean over all B * M of the squared
    distance to the nearest x.  The [B,N,M] matrix is replaced by two exact searches (fit_ops.ChamferNNFn)."""

    def forward(self, x, y):
        d_xy = fit_ops.ChamferNNFn.apply(x, y)[0]
        d_yx = fit_ops.ChamferNNFn.apply(y, x)[0]
        return d_xy.mean() + d_yx.mean()

"""Call surface of the loss-side helpers of the reference's src/utils.py: the point-set Chamfer distances chamfer_distance
(:271-294), chamfer_distance_one_side (:297-321), chamfer_distance_single_shape (:324-358), chamfer_distance_kdtree (:361-381)
and analytic_chamfer_distance (:384-426).  Upstream's [N,M] distance matrix and its host KD-tree are both replaced by one exact
nearest-neighbour search on the device, batched over shapes and differentiable (fit_ops.ChamferNNFn, csrc/chamfer.hip; any
exact search agrees up to ties, and ties go to the lowest index); the SDF half runs in the HIP kernels of csrc/fit.hip.

The fused form of analytic_chamfer_distance used by the training step (sampling + search in one kernel, fixed-capacity
parameter tensors) is prifit_amd.convex_loss.analytic_chamfer_distance; this module keeps upstream's list-based
signature for stand-alone callers (fitting.py)."""
import numpy as np
import torch

from .. import fit_ops
from .guard import guard_sqrt


def nearest_index(src, tgt, chunk=4096):
    """index of the exact nearest row of tgt [T,3] for every row of src [S,3] (direct differences, no expansion)."""
    out = []
    with torch.no_grad():
        for i in range(0, src.shape[0], chunk):
            d = ((src[i:i + chunk, None, :] - tgt[None, :, :]) ** 2).sum(-1)
            out.append(d.argmin(dim=1))
    return torch.cat(out)


def _points(x):
    """upstream :278-282: numpy clouds go to the device as float32; tensors are taken as they are (device tensors only)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x.astype(np.float32)).cuda()
    return x if x.dtype == torch.float32 else x.float()


def nn_d2(a, b, na=None, nb=None):
    """[B,NA] squared distance from every row of a [B,NA,3] to its nearest row of b [B,NB,3] (na / nb: live rows per shape;
    dead rows give 0), differentiable in both."""
    return fit_ops.ChamferNNFn.apply(a, b, na, nb)[0]


def pack_clouds(clouds):
    """list of [n_i,3] device tensors -> ([len, max n_i, 3] zero-padded, [len] int32 counts on the device, [len] float counts)."""
    pts = torch.nn.utils.rnn.pad_sequence([_points(c) for c in clouds], batch_first=True)
    cnt = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int32, device=pts.device)
    return pts, cnt, cnt.to(torch.float32)


def chamfer_distance(pred, gt, sqrt=False):
    """upstream :271-294: pred [B,N,3], gt [B,M,3] -> mean over shapes of (mean_n min_m d + mean_m min_n d) / 2 with d the
    squared distance, or guard_sqrt of it (clamp at 1e-5, then sqrt: monotone, so it is applied to the minima)."""
    pred, gt = _points(pred), _points(gt)
    d_pg, d_gp = nn_d2(pred, gt), nn_d2(gt, pred)
    if sqrt:
        d_pg, d_gp = guard_sqrt(d_pg), guard_sqrt(d_gp)
    return torch.mean(d_pg.mean(1) + d_gp.mean(1)) / 2.0


def chamfer_distance_one_side(pred, gt, side=1):
    """upstream :297-321: side 0 = every pred point to its nearest gt point (mean over N), side 1 = every gt point to its
    nearest pred point (mean over M); then the mean over shapes.  Upstream leaves any other `side` undefined."""
    pred, gt = _points(pred), _points(gt)
    if side == 0:
        d = nn_d2(pred, gt)
    elif side == 1:
        d = nn_d2(gt, pred)
    else:
        raise ValueError("chamfer_distance_one_side: side must be 0 or 1, got %r" % (side,))
    return torch.mean(d.mean(1))


def chamfer_distance_single_shape(pred, gt, one_side=False, sqrt=False, reduce=True):
    """upstream :324-358: pred [N,3], gt [M,3].  one_side: every gt point to its nearest pred point ([M], or its mean);
    otherwise (pred -> gt [N] + gt -> pred [M]) / 2, of the means when `reduce`, else of the vectors themselves, which
    needs N == M as upstream's broadcast does."""
    pred, gt = _points(pred), _points(gt)
    if not one_side and not reduce and pred.shape[0] != gt.shape[0]:
        raise ValueError("chamfer_distance_single_shape(reduce=False): two-sided form adds an [N] and an [M] vector, "
                         "N = %d, M = %d" % (pred.shape[0], gt.shape[0]))
    p, g = pred.unsqueeze(0), gt.unsqueeze(0)
    fin = guard_sqrt if sqrt else (lambda d: d)
    cd2 = fin(nn_d2(g, p)[0])
    if one_side:
        return torch.mean(cd2, 0) if reduce else cd2
    cd1 = fin(nn_d2(p, g)[0])
    if reduce:
        cd1, cd2 = torch.mean(cd1), torch.mean(cd2)
    return (cd1 + cd2) / 2.0


def chamfer_distance_kdtree(source_points, target_points, sqrt=False):
    """upstream :361-381: source_points [B,S,3], target_points [B,T,3] -> mean over shapes of
    (mean_t |t - NN_source(t)|^2 + mean_s |s - NN_target(s)|^2) / 2.  One search per direction for the whole batch."""
    s, t = _points(source_points), _points(target_points)
    d_st, d_ts = nn_d2(t, s), nn_d2(s, t)
    if sqrt:
        d_st, d_ts = torch.sqrt(d_st), torch.sqrt(d_ts)
    return ((d_st.mean(1) + d_ts.mean(1)) / 2.0).mean()


def pack_params(ellipsoid_params_batch, device):
    """list[B] of list[K_b] of (r[3], V[3,3], c[3]) -> fixed-capacity (r, V, c, valid) tensors, differentiable."""
    from ..convex_loss import EllipseParams
    if isinstance(ellipsoid_params_batch, EllipseParams):
        p = ellipsoid_params_batch
        return p.r, p.V, p.c, p.valid
    B = len(ellipsoid_params_batch)
    KM = fit_ops.slots_for(max([len(prm) for prm in ellipsoid_params_batch] + [1]))
    rows_r, rows_V, rows_c = [], [], []
    valid = torch.zeros(B, KM, dtype=torch.int32, device=device)
    for b, prm in enumerate(ellipsoid_params_batch):
        valid[b, :len(prm)] = 1
        pad = KM - len(prm)
        rows_r.append(torch.stack([p[0] for p in prm] + [torch.ones(3, device=device)] * pad))
        rows_V.append(torch.stack([p[1] for p in prm] + [torch.eye(3, device=device)] * pad))
        rows_c.append(torch.stack([p[2] for p in prm] + [torch.zeros(3, device=device)] * pad))
    return torch.stack(rows_r), torch.stack(rows_V), torch.stack(rows_c), valid


def analytic_chamfer_distance(ellipsoid_params_batch, source_points, target_points, cuboid=False):
    """upstream :384-426: per shape (mean_s |s - NN_target(s)|^2 + mean_t (min_k |sdf_k(t)|)^2) / 2, averaged over the
    shapes that have source points; zeros(1) when none has (:421-423)."""
    dev = target_points.device
    r, V, c, valid = pack_params(ellipsoid_params_batch, dev)
    M = target_points.shape[1]
    sdf_ts = fit_ops.SdfLossFn.apply(target_points.contiguous(), r, V, c, valid, cuboid) / M     # [B]
    live = [b for b in range(target_points.shape[0]) if torch.is_tensor(source_points[b])]
    if not live:
        return torch.zeros(1, requires_grad=True, device=dev)
    src, ns, nsf = pack_clouds([source_points[b] for b in live])
    sel = torch.tensor(live, device=dev)
    d_st = nn_d2(src, _points(target_points)[sel], na=ns).sum(1) / nsf          # ragged mean: dead rows hold 0
    return ((d_st + sdf_ts[sel]) / 2.0).mean()


# ---------------------------------------------------------------------------------------------------------------------
# Visualisation names of src/utils.py:51-81 (out of scope as features): the trainer and testing.py import
# them by name (train_partseg_shapenet.py:6, testing.py:2, fitting.py:3,13), so they resolve here and do the file-less part of
# their job: no open3d, nothing is drawn.
# ---------------------------------------------------------------------------------------------------------------------
def save_point_cloud(filename, data):
    """src/utils.py:51-52: `np.savetxt(filename, data, delimiter=" ")`."""
    import numpy as np
    np.savetxt(filename, data.detach().cpu().numpy() if torch.is_tensor(data) else data, delimiter=" ")


def visualize_point_cloud(points, normals=[], colors=[], file="", viz=False):   # noqa: B006 (the reference's signature)
    """src/utils.py:55-72 builds an open3d point cloud, optionally draws and writes it.  Here: returns the arrays it was
    given as a dict (nothing is drawn; `viz=True` raises -- there is no display path in this package)."""
    if viz:
        raise NotImplementedError("visualize_point_cloud(viz=True): visualisation is out of scope (no open3d on this path)")
    return {"points": points, "normals": normals, "colors": colors}


def visualize_point_cloud_from_labels(points, labels, COLORS=None, normals=None, viz=False):
    """src/utils.py:75-81: colours the points by label and hands them to visualize_point_cloud."""
    import numpy as np
    lab = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if COLORS is None:
        COLORS = np.random.rand(500, 3)
    return visualize_point_cloud(points, colors=COLORS[lab.astype(np.int64)], normals=normals if normals is not None else [], viz=viz)

"""Part-segmentation evaluation: the metrics of the reference's testing.evaluation
(testing.py:49-249) computed batched on the device instead of per-shape / per-label numpy loops.

    ev = SegmentationEvaluator()                     # 50 parts, 16 categories (testing.py:30-39)
    ev.update(seg_pred [B,N,50] logits, target [B,N])
    ev.compute() -> {'accuracy', 'class_avg_accuracy', 'class_avg_iou', 'instance_avg_iou', 'category_iou': {...}}

    evaluation(args, epoch, classifier, metrics)     # testing.py:49, the reference's signature (train_partseg_shapenet.py:487)
    evaluate_loader(model, loader, ...)              # the loop of testing.py:110-137 around a model and any iterable of batches

Rules kept from the reference: the category of a shape is that of its first target label (:142); the prediction
is the arg-max over that category's parts only (:143-144); a part absent from both prediction and target counts
as IoU 1 (:203-204); a shape's IoU is the mean over its category's parts; class_avg_iou averages the per-category
means, instance_avg_iou averages all shapes (:226-240).

On the device the counts behind all of that come from ONE kernel launch per batch (csrc/seg_metrics.hip): update()
copies nothing to the host and does not synchronise, compute() makes a single transfer.  A label without a part, or a shape
whose first label has no category -- where the reference stops with a KeyError -- makes compute() raise ValueError."""
import importlib
import os

import numpy as np
import torch

seg_classes = {'Airplane': [0, 1, 2, 3], 'Bag': [4, 5], 'Cap': [6, 7], 'Car': [8, 9, 10, 11],
               'Chair': [12, 13, 14, 15], 'Earphone': [16, 17, 18], 'Guitar': [19, 20, 21], 'Knife': [22, 23],
               'Lamp': [24, 25, 26, 27], 'Laptop': [28, 29], 'Motorbike': [30, 31, 32, 33, 34, 35], 'Mug': [36, 37],
               'Pistol': [38, 39, 40], 'Rocket': [41, 42, 43], 'Skateboard': [44, 45, 46], 'Table': [47, 48, 49]}
classes = ['Airplane', 'Bag', 'Cap', 'Car', 'Chair', 'Earphone', 'Guitar', 'Knife', 'Lamp', 'Laptop', 'Motorbike',
           'Mug', 'Pistol', 'Rocket', 'Skateboard', 'Table']


def to_categorical(y, num_classes):
    """1-hot encodes a tensor (testing.py:42-47), on y's device."""
    return torch.eye(num_classes, device=y.device)[y]


class SegmentationEvaluator:
    """fused=True (default): float32 device logits with at most 64 parts are counted by one kernel launch per batch
    (ops.seg_metrics) and nothing is read back before compute(); fused=False, the CPU and every other input keep the torch path."""
    _SLAB_SHAPES = 1024          # shapes per zeroed count buffer of the kernel path (one fill per that many, not one per batch)

    def __init__(self, num_part=50, categories=None, fused=True):
        self.categories = categories if categories is not None else seg_classes
        self.names = list(self.categories.keys())
        self.num_part = num_part
        self.fused = fused
        cat_of_label = torch.full((num_part,), -1, dtype=torch.long)
        for ci, name in enumerate(self.names):
            cat_of_label[self.categories[name]] = ci
        self.cat_of_label = cat_of_label
        self._table = None                                  # its int32 device copy, uploaded on the first device seen
        self.reset()

    def reset(self):
        self.correct = 0
        self.seen = 0
        self.bad = 0
        self.seen_class = torch.zeros(self.num_part, dtype=torch.long)
        self.correct_class = torch.zeros(self.num_part, dtype=torch.long)
        self.shape_iou, self.shape_cat = [], []
        # kernel path: the running totals, the zeroed count buffers batches are carved from ([buffer, words used]), and per
        # batch (its place in shape_iou / shape_cat, its buffer's number, its first word, B): compute() folds them into the
        # fields above, which hold the kernel path's share only after that
        self._totals, self._slabs, self._pending = None, [], []

    @torch.no_grad()
    def predict(self, seg_pred, target):
        """arg-max restricted to the parts of each shape's category (testing.py:141-144)."""
        col = self.cat_of_label.to(seg_pred.device)
        cat = col[target[:, 0]]                                            # [B]
        allowed = col.view(1, 1, -1) == cat.view(-1, 1, 1)                 # [B,1,P]
        return seg_pred.masked_fill(~allowed, float('-inf')).argmax(dim=-1), cat

    @torch.no_grad()
    def update(self, seg_pred, target):
        B, N, P = seg_pred.shape
        if self.fused and seg_pred.is_cuda and seg_pred.dtype == torch.float32 and P == self.num_part and P <= 64 and B * N:
            return self._update_fused(seg_pred, target)
        target = target.long()
        pred, cat = self.predict(seg_pred, target)
        hit = pred == target
        self.correct += int(hit.sum())
        self.seen += B * N
        self.seen_class += torch.bincount(target.reshape(-1), minlength=P).cpu()
        self.correct_class += torch.bincount(target[hit], minlength=P).cpu()
        oh_p = torch.nn.functional.one_hot(pred, P)
        oh_t = torch.nn.functional.one_hot(target, P)
        inter = (oh_p & oh_t).sum(dim=1).double()                          # [B,P]
        union = (oh_p | oh_t).sum(dim=1).double()
        part_iou = torch.where(union == 0, torch.ones_like(union), inter / union.clamp(min=1.0))
        in_cat = (self.cat_of_label.to(seg_pred.device).view(1, -1) == cat.view(-1, 1)).double()
        self.shape_iou.append(((part_iou * in_cat).sum(dim=1) / in_cat.sum(dim=1)).cpu())
        self.shape_cat.append(cat.cpu())
        return pred

    def _update_fused(self, seg_pred, target):
        """One launch, no device-to-host copy, no synchronisation: the batch's shape_cat [B], inter and uni [B,P] stay on the
        device in a zeroed buffer shared by many batches, the batch totals are added to one persistent tensor."""
        from . import ops
        B, N, P = seg_pred.shape
        dev = seg_pred.device
        if self._totals is not None and self._totals.device != dev:
            self._fold()
        if self._table is None or self._table.device != dev:
            self._table = self.cat_of_label.to(torch.int32).to(dev)
        if self._totals is None:
            self._totals = torch.zeros(2 + 2 * P, dtype=torch.int64, device=dev)
        words = B * (1 + 2 * P)
        if not self._slabs or self._slabs[-1][1] + words > self._slabs[-1][0].numel():
            self._slabs.append([torch.zeros(max(self._SLAB_SHAPES, 4 * B) * (1 + 2 * P), dtype=torch.int32, device=dev), 0])
        slab, off = self._slabs[-1]
        w = slab[off:off + words]
        pred = torch.empty(B, N, dtype=torch.int64, device=dev)
        ops.seg_metrics(seg_pred, target, self._table, True, self._totals,
                        out=(pred, w[:B], w[B:B + B * P].view(B, P), w[B + B * P:].view(B, P)))
        self._pending.append((len(self.shape_iou), len(self._slabs) - 1, off, B))
        self._slabs[-1][1] = off + words
        self.shape_iou.append(None)                          # this batch's place in the order of the shapes
        self.shape_cat.append(None)
        self.seen += B * N
        return pred

    def _fold(self):
        """The single transfer of the kernel path: the totals and every pending batch's counts in one copy; from the integer
        counts the float64 per-shape IoU of testing.py:176-204 (np.mean over the category's parts, an absent part = 1)."""
        if self._totals is None:
            return
        P = self.num_part
        host = torch.cat([self._totals.view(torch.int32)] + [slab[:used] for slab, used in self._slabs]).cpu().numpy()
        totals = host[:2 * (2 + 2 * P)].view(np.int64)
        first = np.cumsum([2 * (2 + 2 * P)] + [used for _, used in self._slabs])       # first word of every buffer in `host`
        col = self.cat_of_label.numpy()
        for place, k, off, B in self._pending:
            w = host[first[k] + off:first[k] + off + B * (1 + 2 * P)]
            cat = w[:B].astype(np.int64)
            inter = w[B:B + B * P].reshape(B, P).astype(np.float64)
            union = w[B + B * P:].reshape(B, P).astype(np.float64)
            part_iou = np.where(union == 0, 1.0, inter / np.maximum(union, 1.0))
            iou = np.full(B, np.nan)                          # (a shape without a category: nan, as the torch path's 0 / 0)
            for ci in np.unique(cat[cat >= 0]):
                rows = np.nonzero(cat == ci)[0]
                iou[rows] = np.mean(np.ascontiguousarray(part_iou[np.ix_(rows, np.nonzero(col == ci)[0])]), axis=1)
            self.shape_iou[place] = torch.from_numpy(iou)
            self.shape_cat[place] = torch.from_numpy(cat)
        self.correct += int(totals[0])
        self.bad += int(totals[1])
        self.seen_class += torch.from_numpy(totals[2:2 + P].copy())
        self.correct_class += torch.from_numpy(totals[2 + P:].copy())
        self._totals, self._slabs, self._pending = None, [], []

    def compute(self):
        self._fold()
        if self.bad:
            raise ValueError("SegmentationEvaluator: %d point(s) carry a label outside [0, %d) or belong to a shape whose first "
                             "label has no category (the reference stops with a KeyError)" % (self.bad, self.num_part))
        iou = torch.cat(self.shape_iou) if self.shape_iou else torch.zeros(0, dtype=torch.float64)
        cat = torch.cat(self.shape_cat) if self.shape_cat else torch.zeros(0, dtype=torch.long)
        per_cat = {}
        for ci, name in enumerate(self.names):
            sel = iou[cat == ci]
            per_cat[name] = float(sel.mean()) if sel.numel() else float('nan')
        seen = self.seen_class.double()
        with np.errstate(invalid='ignore', divide='ignore'):
            class_acc = np.mean((self.correct_class.double() / seen).numpy())   # nan if a part never occurs (:229-230)
        present = [v for v in per_cat.values() if not np.isnan(v)]
        return {'accuracy': self.correct / float(max(self.seen, 1)),
                'class_avg_accuracy': float(class_acc),
                # mean over categories (:226,:234); categories without shapes are left out, which equals the
                # reference whenever every category occurs (it would produce nan otherwise)
                'class_avg_iou': float(np.mean(present)) if present else float('nan'),
                'instance_avg_iou': float(iou.mean()) if iou.numel() else float('nan'),
                'category_iou': per_cat}


DATA_ROOT = 'ShapeSelfSup/dataset/shapenetcore_partanno_segmentation_benchmark_v0_normal'   # testing.py:72, relative to the cwd


def evaluation(args, epoch=0, classifier=None, metrics={}, loader=None):   # noqa: B006 (the reference's signature)
    """testing.py:49-249 under the reference's signature: `evaluation(args, epoch, classifier, metrics)` as the trainer calls
    it after every epoch (train_partseg_shapenet.py:487), `evaluation(args)` as `python testing.py` does (:253-255).

    args: the namespace of args_parser.py -- eval_split, npoint, normal, batch_size, num_classes, num_parts, category, seed and,
    when `classifier` is None, model / pretrained_model (+ dgcnn_k, reconstruct) to build and load one (:96-110).  The test
    split is read from DATA_ROOT below the current directory (:72-77) unless `loader` is given.  The forward keywords of
    :139 (quantile, msc_iterations, max_num_clusters, alpha, beta, if_cuboid, embed, seed) are taken from `args` where present.
    Returns `metrics` -- the running best, updated in place when the class-average mIoU did not fall (:241-247) -- like the
    reference; the metrics of THIS evaluation are left in `evaluation.last`."""
    from . import data as D
    if getattr(args, "gpu", None) is not None:
        os.environ["CUDA_VISIBLE_DEVICES"] = args.gpu              # :55-56
    if loader is None:
        ds = D.PartNormalDataset(root=DATA_ROOT, npoints=args.npoint, split=args.eval_split, normal_channel=args.normal)
        loader = torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=False, num_workers=0)
        print("The number of test data is: %d" % len(ds))
    if classifier is None:
        if getattr(args, "pretrained_model", None) is None:
            raise ValueError("evaluation(args): no classifier given and args.pretrained_model is not set")
        MODEL = importlib.import_module(args.model)
        if 'dgcnn' in args.model:
            classifier = MODEL.get_model(args.num_parts, normal_channel=args.normal, k=args.dgcnn_k).cuda()
        else:
            classifier = MODEL.get_model(args.num_parts, normal_channel=args.normal).cuda()
        ckpt = torch.load(args.pretrained_model, map_location="cuda")
        state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in ckpt['model_state_dict'].items()}
        classifier.load_state_dict(state)                        # (upstream wraps in DataParallel first: 'module.' keys)
    fwd = {k: getattr(args, k) for k in ("quantile", "msc_iterations", "max_num_clusters", "alpha", "beta", "if_cuboid",
                                          "embed", "seed") if hasattr(args, k)}
    test_metrics = evaluate_loader(classifier, loader, num_classes=args.num_classes, num_part=args.num_parts,
                                   category=bool(args.category), metrics=metrics if metrics != {} else None, epoch=epoch, **fwd)
    evaluation.last = test_metrics
    if metrics != {}:
        print('Best test Accuracy: {:6f}, Best Epoch: {},  Best Class avg mIOU: {:6f}, Best Instance avg mIOU: {:6f}, Best Loss: {:6f}'
              .format(metrics['best_acc'], metrics['best_epoch'], metrics['best_class_avg_miou'],
                      metrics['best_instance_avg_miou'], metrics['best_chamfer_loss']))
    print('%sAccuracy: %f  Class avg mIOU: %f   Instance avg mIOU: %f, Loss: %f' % (
        ('Epoch %d test ' % (epoch + 1)) if metrics != {} else 'Test ', test_metrics['accuracy'], test_metrics['class_avg_iou'],
        test_metrics['instance_avg_iou'], test_metrics['chamfer_loss']))
    return metrics


@torch.no_grad()
def evaluate_loader(classifier, loader, num_classes=16, num_part=50, category=True, device=None, metrics=None, epoch=0,
                    **forward_kwargs):
    """testing.py:110-249 for a model of this package: loader yields (points [B,N,C], label [B,1], target [B,N]).
    Returns the test metrics; if `metrics` (the running best, :241-247) is given it is updated in place."""
    device = device if device is not None else next(classifier.parameters()).device
    ev = SegmentationEvaluator(num_part)
    was_training = classifier.training
    classifier.eval()
    chamfer = []
    for points, label, target in loader:
        points = torch.as_tensor(points).float().to(device).transpose(2, 1).contiguous()
        label = torch.as_tensor(label).long().to(device)
        target = torch.as_tensor(target).long().to(device)
        # (the reference passes the one-hot label whatever args.category says, :139: its `category_label` of :131-134 is
        # computed and never used; `category` is kept in the signature for the same reason)
        out = classifier(points, to_categorical(label, num_classes), include_convex_loss=False, evaluation=True, **forward_kwargs)
        seg_pred = out[0]
        if len(out) >= 5 and torch.is_tensor(out[4]):
            chamfer.append(out[4].float().mean())             # a device scalar: read back with the others, after the loop
        ev.update(seg_pred, target)
    classifier.train(was_training)
    test_metrics = ev.compute()
    test_metrics['chamfer_loss'] = float(np.mean(torch.stack(chamfer).cpu().double().numpy())) if chamfer else 0.0
    if metrics:
        if metrics['best_class_avg_miou'] <= test_metrics['class_avg_iou']:
            metrics.update(best_chamfer_loss=test_metrics['chamfer_loss'], best_epoch=epoch + 1,
                           best_acc=test_metrics['accuracy'], best_class_avg_miou=test_metrics['class_avg_iou'],
                           best_instance_avg_miou=test_metrics['instance_avg_iou'])
    return test_metrics

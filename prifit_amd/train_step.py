"""The training iteration of the hot path: what
train_partseg_shapenet.py:252-259, :321-340, :372-399, :436-451, :467-475 does around the model, for one
process per GPU.

    tr = Trainer(model)                       # Adam(lr, betas .9/.999, eps 1e-8, weight_decay) as upstream :252-259
    tr = Trainer(model, optimizer="SGD")      # any other name: SGD(lr, momentum 0.9), upstream's `else:` at :260-261
    tr.set_epoch(epoch)                       # lr / BatchNorm-momentum schedule, upstream :325-334
    loss, acc = tr.supervised_step(points, target)              # upstream :372-399
    ss = tr.selfsup_step(chamfer_points, quantile=.05, ...)     # upstream :436-451
    ss = tr.selfsup_step(chamfer_points, rotation_z=True, ...)  # + the augmentation flags of pretrain_partseg_shapenet.py:321-351
    val = tr.selfsup_validate(val_batches, ...)                 # its per-epoch validation pass, :377-402
    hist = tr.init_classifier(batches)        # `--init_cls`, upstream :56-99 / :302-305: fit conv2 alone on the frozen network
    tr.save(path) / tr.load(path)             # checkpoint dict of upstream :467-475
    tr.finish()                               # REQUIRED after the last step under torch.distributed: the deferred
                                              # has-gradient check of the final exchange (ddp.FlatGradBucket.flush)

The augmentation (random per-shape scale in [0.8, 1.25] and shift in [-0.1, 0.1], provider.py:278-303) runs
on the device.  Gradients are exchanged with `FlatGradBucket` when torch.distributed is initialised."""
import numpy as np
import os

import torch
import torch.nn.functional as F

from .ddp import FlatGradBucket

LEARNING_RATE_CLIP = 1e-5      # upstream :285
MOMENTUM_ORIGINAL = 0.1        # upstream :286
MOMENTUM_DECAY = 0.5           # upstream :287


def random_scale_shift(points, generator=None, scale_low=0.8, scale_high=1.25, shift_range=0.1):
    """provider.py:278-303 on a [B,N,3+] device tensor (first three channels), one scale and shift per shape."""
    B = points.shape[0]
    dev = points.device
    scales = torch.empty(B, 1, 1, device=dev).uniform_(scale_low, scale_high, generator=generator)
    shifts = torch.empty(B, 1, 3, device=dev).uniform_(-shift_range, shift_range, generator=generator)
    out = points.clone()
    out[:, :, 0:3] = out[:, :, 0:3] * scales + shifts
    return out


class SpeculativeRunner:
    """Run a forward+backward closure with fit_ops.speculative() (no mid-step host read-back); if the clustering
    verdict, read once everything is enqueued, says a quantile-doubling retry was needed, put the BatchNorm
    buffers back, clear the gradients and run the closure again the synchronous way."""

    def __init__(self, model):
        # one list per dtype: _foreach_copy_ then runs as a single multi-tensor kernel per list instead of one
        # copy per buffer (BatchNorm statistics are fp32, the batch counters int64)
        groups = {}
        for b in model.buffers():
            groups.setdefault(b.dtype, []).append(b)
        self.bufs = list(groups.values())
        self.snap = [[torch.empty_like(b) for b in g] for g in self.bufs]
        self.model = model
        self.fallbacks = 0
        self.runs = 0
        # set by a caller that wants the NEXT run to go through the fall-back once whatever its verdict (bench.py's first
        # warm-up step: the first fall-back of a process grows the caching allocator by ~4 GB, 0.2 s of hipMalloc)
        self.force_next = False

    def run(self, fn, reset):
        from . import fit_ops

        for dst, src in zip(self.snap, self.bufs):
            torch._foreach_copy_(dst, src)
        # python-side state the forward mutates: the entropy weight schedule `beta *= 0.99` per convex-loss forward
        # (models/pointnet2_part_seg_msg.py:96-99) must advance once per ACCEPTED step, not once per attempt
        beta = getattr(self.model, "beta", None)
        rng = torch.cuda.get_rng_state() if torch.cuda.is_available() else None
        with fit_ops.speculative() as spec:
            out = fn()
        self.runs += 1
        forced, self.force_next = self.force_next, False
        if spec.ok() and not forced:
            return out
        self.fallbacks += 1
        for dst, src in zip(self.bufs, self.snap):
            torch._foreach_copy_(dst, src)
        if beta is not None:
            self.model.beta = beta
        if rng is not None:
            torch.cuda.set_rng_state(rng)   # dropout masks / random tables of the retried step = those of the first try
        reset()
        return fn()


class _Backbone(torch.nn.Module):
    """`net.embed_features` as a module of its own (what make_graphed_callables captures): parameters = the network's."""

    def __init__(self, net, fps_start):
        super().__init__()
        self.net, self.fps_start = net, fps_start

    def forward(self, xyz, cls_label):
        return self.net._embed_features_eager(xyz, cls_label, self.fps_start)


def graph_backbone(net, xyz, cls_label, fps_start):
    """Capture the backbone of `net` (everything up to `feat`: set abstraction, feature propagation, conv1 + bn1 --
    upstream models/pointnet2_part_seg_msg.py:64-88 -- forward AND backward) into two HIP graphs and install it as
    `net.embed_features`: ~300 of a step's ~440 launches then cost the host one graph launch each way.  The shapes are
    static and nothing in there reads back to the host, the kernels only enqueue on the current stream (include/
    prifit_hip.h), so the capture is `torch.cuda.make_graphed_callables` as is; the fit path stays eager (its
    cluster-count verdict is read on the host, SpeculativeRunner).  Static inputs: `xyz` / `cls_label` of these shapes
    (other tensors are copied in), `fps_start` = these very tensors.  BatchNorm buffers are put back after the warm-up
    iterations of the capture.  Returns the graphed callable; `net.embed_features` replays it in training mode with
    gradients enabled and falls back to the eager backbone (`net._embed_features_eager`) otherwise -- an eval / no_grad
    forward must not replay a training-mode graph (batch statistics, running-stat updates)."""
    from . import arena
    if not hasattr(net, "_embed_features_eager"):
        net._embed_features_eager = net.embed_features
    bufs = [b for b in net.buffers()]
    snap = [b.clone() for b in bufs]
    was_enabled = arena._ENABLED
    arena._ENABLED = False          # zero-filled tensors inside the graphs are the graphs' own (re-zeroed at every replay)
    try:
        graphed = torch.cuda.make_graphed_callables(_Backbone(net, fps_start), (xyz, cls_label), num_warmup_iters=2,
                                                    allow_unused_input=True)
    finally:
        arena._ENABLED = was_enabled
        with torch.no_grad():
            for b, s_ in zip(bufs, snap):
                b.copy_(s_)

    shape = (tuple(xyz.shape), tuple(cls_label.shape))

    def embed_features(xyz_, cls_, fps_start_=None):
        same_start = fps_start_ is None or fps_start_ is fps_start or (
            len(fps_start_) == len(fps_start) and all(a is b for a, b in zip(fps_start_, fps_start)))
        if (not net.training or not torch.is_grad_enabled() or (tuple(xyz_.shape), tuple(cls_.shape)) != shape
                or not same_start):
            return net._embed_features_eager(xyz_, cls_, fps_start_)
        return graphed(xyz_, cls_)

    net.embed_features = embed_features
    return graphed


def init_classifier(model, batches, epochs=500, lr=0.1, momentum=0.5, augment=True, log=None):
    """`--init_cls` (args_parser.py:43): after a pre-trained checkpoint is loaded, fit only the last layer (conv2, 128 ->
    num_part) by logistic regression -- train_init_class, train_partseg_shapenet.py:56-99: the network in eval mode for the
    whole of it, SGD(conv2.parameters(), lr=0.1, momentum=0.5), 500 epochs, scale + shift augmentation per batch.
    Here the network is FROZEN (inference.freeze: folded BatchNorm, no autograd) and an iteration is one frozen forward up
    to fp1's rows, one launch pair for loss + conv2's gradient (FrozenPartSeg.probe_step) and one FlatSGD launch.
    batches: a re-iterable (list, DataLoader) of (points [B,N,3(+3)] channels-last, label, target [B,N] int64) as the
    reference's loader yields them; label = the category, integers [B] / [B,1] or one-hot floats [B,16] / [B,1,16] (None:
    zeros, as supervised_step); an optional fourth element is the sampling's fps_start, as supervised_step takes it (default:
    drawn per call).  log: optional callable (epoch, mean loss, mean accuracy).
    -> {"loss": [...], "acc": [...]}: per epoch the mean over the batches of the loss and of correct / points (the
    reference's init_cls_loss / init_cls_acc), read back ONCE per epoch.
    Nothing but conv2 changes: no BatchNorm buffer, no other parameter, not the trainer's optimizer state (its moments for
    conv2 stay as they are, as the reference's Adam's do); conv2's parameters stay in the storage the trainer's optimizer
    steps.  Per-rank: nothing is exchanged (6,450 parameters; every rank fits its own shard's layer unless the caller
    broadcasts).  Networks without a frozen form (SSG, DGCNN) raise inference.freeze's TypeError."""
    from . import inference
    from .optim import FlatSGD
    frozen = model.refresh() if isinstance(model, inference.FrozenPartSeg) else inference.freeze(model)
    conv2 = frozen._source.conv2
    params = [conv2.weight, conv2.bias]
    home = [p.data for p in params]                    # FlatSGD re-homes p.data into a buffer of its own: put back below
    had_grad = [p.grad for p in params]
    opt = FlatSGD(params, lr=lr, momentum=momentum)
    hist = {"loss": [], "acc": []}
    dev = conv2.weight.device
    try:
        for epoch in range(epochs):
            stats, points_seen = [], []
            for points, label, target, *more in batches:
                fps_start = more[0] if more else None
                points = points.to(dev, torch.float32)
                B, N, _ = points.shape
                if augment:
                    points = random_scale_shift(points)
                xyz = points.transpose(2, 1).contiguous()
                if label is None:
                    onehot = torch.zeros(B, 1, 16, device=dev)
                else:
                    label = torch.as_tensor(label).to(dev)
                    if label.dtype.is_floating_point and label.numel() == B * 16:
                        onehot = label.reshape(B, 1, 16).float()
                    else:
                        onehot = F.one_hot(label.reshape(B).long(), 16).reshape(B, 1, 16).float()
                stats.append(frozen.probe_step(xyz, onehot, torch.as_tensor(target).to(dev).long(), fps_start=fps_start))
                points_seen.append(B * N)
                opt.step()
            if not stats:
                raise ValueError("init_classifier: no batches")
            s = torch.stack(stats).cpu()               # the epoch's one read-back
            loss = float(s[:, 0].mean())
            acc = float((s[:, 2] / torch.tensor(points_seen, dtype=torch.float32)).mean())
            hist["loss"].append(loss)
            hist["acc"].append(acc)
            if log is not None:
                log(epoch, loss, acc)
    finally:
        with torch.no_grad():
            for p, h, g in zip(params, home, had_grad):
                h.copy_(p.data)
                p.data = h
                p.grad = g
        frozen.refresh()
    return hist


class Trainer:
    def __init__(self, model, num_part=50, learning_rate=0.001, decay_rate=1e-4, lr_decay=0.5, step_size=20, lmbda=1.0,
                 fused_adam=True, strict_seen=False, optimizer="Adam"):
        # one process per GPU: this rank's own cores and capped CPU thread pools (prifit_amd/hostcfg.py; a single process is
        # left alone, and a launcher that already did it -- bench.py -- makes this a no-op)
        from . import hostcfg
        self.host = hostcfg.apply_from_env()
        self.model = model
        self.num_part = num_part
        self.lr0, self.lr_decay, self.step_size, self.lmbda = learning_rate, lr_decay, step_size, lmbda
        # one launch per step over a flat parameter buffer on the GPU (prifit_amd/optim.py; PRIFIT_FLAT_ADAM=0 / fused_adam=False:
        # torch's optimizer, the A/B arm); host tensors (the gloo tests of the exchange logic) take torch's
        on_gpu = next(model.parameters()).is_cuda
        flat = on_gpu and fused_adam and os.environ.get("PRIFIT_FLAT_ADAM", "1") != "0"
        if optimizer != "Adam":
            # upstream :260-261: every other `--optimizer` is SGD(lr, momentum=0.9), without weight decay; the same flat / torch split
            if flat:
                from .optim import FlatSGD
                self.optimizer = FlatSGD(model.parameters(), lr=learning_rate, momentum=0.9)
            else:
                self.optimizer = torch.optim.SGD(model.parameters(), lr=learning_rate, momentum=0.9)
        elif flat:
            from .optim import FlatAdam
            self.optimizer = FlatAdam(model.parameters(), lr=learning_rate, betas=(0.9, 0.999), eps=1e-08, weight_decay=decay_rate)
        else:
            self.optimizer = torch.optim.Adam(model.parameters(), lr=learning_rate, betas=(0.9, 0.999), eps=1e-08,
                                              weight_decay=decay_rate, fused=bool(fused_adam and on_gpu))
        # strict_seen: ranks may disagree on which parameters get a gradient (see ddp.FlatGradBucket._adopt)
        self.bucket = FlatGradBucket(model, strict_seen=strict_seen)
        self._next = None          # the batch prepared by prefetch_selfsup
        # DataParallel replicates module 0's parameters and buffers onto every GPU at each forward
        # (train_partseg_shapenet.py:248-250); with one process per GPU the ranks start from rank 0's model instead
        self.bucket.broadcast_parameters(0)
        self.speculative = SpeculativeRunner(model) if next(model.parameters()).is_cuda else None
        self.epoch = 0
        self.train_acc = 0.0
        self.frozen = None         # inference.FrozenPartSeg of the model, built by init_classifier

    # ------------------------------------------------------------------ schedule (upstream :325-334)
    def set_epoch(self, epoch):
        self.epoch = epoch
        lr = max(self.lr0 * (self.lr_decay ** (epoch // self.step_size)), LEARNING_RATE_CLIP)
        for group in self.optimizer.param_groups:
            group["lr"] = lr
        momentum = max(MOMENTUM_ORIGINAL * (MOMENTUM_DECAY ** (epoch // self.step_size)), 0.01)
        for m in self.model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.momentum = momentum
        return lr, momentum

    def _apply(self, loss):
        if loss is not None:
            loss.backward()
        self.bucket.allreduce()
        if getattr(self.optimizer, "takes_grads", False):  # FlatAdam / FlatSGD: hand over the gradient list the exchange just read
            self.optimizer.step(grads=self.bucket.grads())
        else:
            self.optimizer.step()

    # ------------------------------------------------------------------ supervised step (upstream :372-399)
    def supervised_step(self, points, target, category_label=None, augment=True, fps_start=None):
        """points [B,N,3(+3)] channels-last, target [B,N] int64 part labels."""
        B, N, _ = points.shape
        if augment:
            points = random_scale_shift(points)
        xyz = points.transpose(2, 1).contiguous()
        if category_label is None:
            category_label = torch.zeros(B, 1, 16, device=points.device)
        self.bucket.zero()
        self.model.train()
        out = self.model(xyz, category_label, include_convex_loss=False, fps_start=fps_start)
        seg_pred = out[0].contiguous().view(-1, self.num_part)
        tgt = target.view(-1)
        loss = F.cross_entropy(seg_pred, tgt)      # get_loss: CE on log-probabilities (upstream msg:137-144)
        self._apply(loss)
        with torch.no_grad():
            acc = (seg_pred.argmax(1) == tgt).float().mean()
        return loss.detach(), acc

    # ------------------------------------------------------------------ self-supervised step (upstream :436-451)
    def _selfsup_batch(self, chamfer_points, npoint, augment, subset, rotation_z=False, rotation_z_45=False,
                       random_anisotropic_scale=False, fused_augment=False):
        """Augmentation + the random `npoint`-subset that is the model input (upstream :439-441), channels-first.

        With one of the four flags set this is the batch preparation of pretrain_partseg_shapenet.py:321-351 -- its
        `--rotation_z`, `--rotation_z_45`, `--random_anisotropic_scale` (args_parser.py) and, with fused_augment alone, just scale
        and shift -- as ONE 3x4 matrix per shape and ONE launch (provider.compose_affine / affine_batch, csrc/augment.hip).  The
        parameters are drawn on the host with `np.random`, each by the reference function's own call and in the script's order
        for its `chamfer_points` array: scale (B), shift (B,3), anisotropic scale (B,1,3), one `uniform()` angle per shape, one
        `randint(1, 8)` per shape, then `choice(M, npoint, replace=False)`.  The draws the script spends on its `points` array
        (:319-320, :324, :332, :336) are NOT made: that array is overwritten by the subset of `chamfer_points` at :351, so a seeded
        run follows the script's law, not its `np.random` stream position."""
        B, M, _ = chamfer_points.shape
        if rotation_z or rotation_z_45 or random_anisotropic_scale or fused_augment:
            if not augment:
                raise ValueError("rotation_z / rotation_z_45 / random_anisotropic_scale / fused_augment are augmentations: "
                                 "they cannot be combined with augment=False")
            from . import provider
            scale = np.random.uniform(0.8, 1.25, B)                                                   # provider.py:300
            shift = np.random.uniform(-0.1, 0.1, (B, 3))                                              # :286
            aniso = np.random.uniform(0.8, 1.25, [B, 1, 3]) if random_anisotropic_scale else None     # :314
            ang1 = np.array([np.random.uniform() * 2 * np.pi for _ in range(B)]) if rotation_z else None      # :97
            ang2 = np.array([np.random.randint(1, 8) * np.pi / 4 for _ in range(B)]) if rotation_z_45 else None   # :118
            if subset is None:
                subset = np.random.choice(M, npoint, replace=False)
            return provider.affine_batch(chamfer_points, provider.compose_affine(scale, shift, aniso, ang1, ang2), subset)
        if augment:
            chamfer_points = random_scale_shift(chamfer_points)
        cham = chamfer_points.transpose(2, 1).contiguous()
        if subset is None:
            subset = torch.from_numpy(np.random.choice(M, npoint, replace=False)).to(cham.device)
        return cham, cham[:, :, subset].contiguous()

    def prefetch_selfsup(self, chamfer_points, npoint=2048, augment=True, subset=None, fps_start=None, rotation_z=False,
                         rotation_z_45=False, random_anisotropic_scale=False, fused_augment=False):
        """Prepare the NEXT self-supervised batch now -- augmentation and subset, what a DataLoader worker does upstream --
        and start its farthest-point sampling behind the backbone forward of the step that runs next (`model.sample_ahead`
        through the `after_backbone` hook: the sampling chain depends on the coordinates alone, is 640 serial rounds on one
        workgroup per shape, and there it runs beside the matrix-bound mean-shift kernels instead of at the head of its
        own step; same indices as in-line sampling).  The following `selfsup_step()` WITHOUT `chamfer_points` consumes it.
        Models without `sample_ahead` (DGCNN) only get the batch prepared.  The four augmentation flags: `_selfsup_batch`."""
        if self._next is not None:
            raise RuntimeError("prefetch_selfsup: the batch of an earlier prefetch has not been consumed by a "
                               "selfsup_step() yet -- a second prefetch would drop it (its augmentation and RNG draw spent)")
        cham, points = self._selfsup_batch(chamfer_points, npoint, augment, subset, rotation_z, rotation_z_45,
                                           random_anisotropic_scale, fused_augment)
        nxt = {"cham": cham, "points": points, "ahead": None, "fps_start": fps_start}
        self._next = nxt
        if points.is_cuda and hasattr(self.model, "sample_ahead"):
            def hook():
                self.model.after_backbone = None
                if self._next is nxt and nxt["ahead"] is None:
                    nxt["ahead"] = self.model.sample_ahead(points, fps_start)
            self.model.after_backbone = hook

    def selfsup_step(self, chamfer_points=None, npoint=2048, quantile=0.01, msc_iterations=20, max_num_clusters=25,
                     augment=True, subset=None, rotation_z=False, rotation_z_45=False, random_anisotropic_scale=False,
                     fused_augment=False, **loss_kwargs):
        """chamfer_points [B,M,3]: the model input is a random `npoint`-subset of them (upstream :441).
        chamfer_points=None: the batch prepared by `prefetch_selfsup` (the flags then belong to that call).
        rotation_z / rotation_z_45 / random_anisotropic_scale: the pre-training script's augmentation flags, fused_augment: the
        one-launch preparation for scale and shift alone -- see `_selfsup_batch`; all off: the torch-operator path."""
        if chamfer_points is None:
            if self._next is None:
                raise RuntimeError("selfsup_step() without chamfer_points needs a prefetch_selfsup(...) before it")
            nxt, self._next = self._next, None
            if getattr(self.model, "after_backbone", None) is not None and nxt["ahead"] is None:
                self.model.after_backbone = None      # no step ran in between: sample in line
            cham, points = nxt["cham"], nxt["points"]
            start = nxt["ahead"] if nxt["ahead"] is not None else nxt["fps_start"]
            if start is not None:
                loss_kwargs = dict(loss_kwargs, fps_start=start)
        else:
            cham, points = self._selfsup_batch(chamfer_points, npoint, augment, subset, rotation_z, rotation_z_45,
                                               random_anisotropic_scale, fused_augment)
        B = cham.shape[0]
        category_label = torch.zeros(B, 1, 16, device=cham.device)
        self.bucket.zero()
        self.model.train()

        def fwd_bwd():
            out = self.model(points, category_label, chamfer_points=cham, include_convex_loss=True, quantile=quantile,
                             msc_iterations=msc_iterations, max_num_clusters=max_num_clusters, **loss_kwargs)
            ss_loss = torch.mean(out[3]) * self.lmbda
            ss_loss.backward()
            return ss_loss

        if self.speculative is not None:
            ss_loss = self.speculative.run(fwd_bwd, self.bucket.zero)
        else:
            ss_loss = fwd_bwd()
        self._apply(None)
        return ss_loss.detach()

    # ------------------------------------------------------------------ classifier-layer pre-training (upstream :56-99, :302-305)
    def init_classifier(self, batches, epochs=500, lr=0.1, momentum=0.5, augment=True, log=None):
        """`--init_cls`: fit conv2 alone on the frozen form of `self.model` -- see the module's init_classifier.  Leaves the
        trainer's optimizer state, every other parameter and every BatchNorm buffer as they are.  The frozen form is kept
        as `self.frozen` (re-folded from the live model at every call and once more at the end)."""
        from . import inference
        if self.frozen is None or self.frozen._source is not self.model:
            self.frozen = inference.freeze(self.model)
        return init_classifier(self.frozen, batches, epochs, lr, momentum, augment, log)

    # ------------------------------------------------------------------ validation (pretrain_partseg_shapenet.py:377-402)
    def selfsup_validate(self, batches, npoint=2048, quantile=0.01, msc_iterations=20, max_num_clusters=25, subset=None,
                         **loss_kwargs):
        """The per-epoch validation pass of the pre-training script (:379-401): the model in eval mode under no_grad, no
        augmentation, per batch [B,M,3] a random `npoint`-subset (`np.random.choice`, or `subset` for every batch when given)
        as the model input; returns the mean over the batches of mean(out[3]) as a Python float (the script's `avg_val_loss`).
        No optimizer step, no gradient exchange -- local to this rank; the model goes back into the mode it was in.  As
        upstream, every forward with the convex loss advances the model's entropy-weight schedule (`beta *= 0.99`)."""
        was_training = self.model.training
        self.model.eval()
        total, count = 0.0, 0
        try:
            with torch.no_grad():
                for chamfer_points in batches:
                    cham, points = self._selfsup_batch(chamfer_points, npoint, False, subset)
                    category_label = torch.zeros(cham.shape[0], 1, 16, device=cham.device)
                    out = self.model(points, category_label, chamfer_points=cham, include_convex_loss=True, quantile=quantile,
                                     msc_iterations=msc_iterations, max_num_clusters=max_num_clusters, **loss_kwargs)
                    total += torch.mean(out[3]).item()
                    count += 1
        finally:
            self.model.train(was_training)
        if count == 0:
            raise ValueError("selfsup_validate: no batches")
        return total / count

    # ------------------------------------------------------------------ checkpoints (upstream :467-475, :263-274)
    def finish(self):
        """After the last optimizer step: the deferred has-gradient check of the final exchange (ddp.FlatGradBucket.flush)."""
        self.bucket.flush()

    def sync_buffers(self):
        """COLLECTIVE: rank 0's BatchNorm statistics win on every rank ("replica 0" of DataParallel).  Every rank enters it,
        so it also runs the deferred has-gradient check of the last exchange first: the documented pattern
        `sync_buffers(); if rank == 0: write_checkpoint()` can then not persist a model taken after a divergent step."""
        self.bucket.flush()
        self.bucket.sync_buffers(0)

    def write_checkpoint(self, path, extra=None):
        """Local, no communication: the checkpoint dict of upstream :467-475 -- safe under `if rank == 0:`.  extra: a dict
        merged into it, e.g. the `selfsup_loss` / `val_loss` keys of the pre-training script's checkpoints
        (pretrain_partseg_shapenet.py:431-437)."""
        state = {"epoch": self.epoch, "train_acc": self.train_acc, "model_state_dict": self.model.state_dict(),
                 "optimizer_state_dict": self.optimizer.state_dict()}
        if extra is not None:
            state.update(extra)
        torch.save(state, path)

    def save(self, path, extra=None):
        """sync_buffers() + write_checkpoint() on rank 0.  COLLECTIVE under torch.distributed: EVERY rank must call it
        (a caller that guards it with `if rank == 0:` would leave rank 0 alone in the broadcast -- such a caller uses
        write_checkpoint, after a sync_buffers() that all ranks entered)."""
        import torch.distributed as dist
        self.bucket.flush()
        self.sync_buffers()
        if dist.is_initialized() and dist.get_rank() != 0:
            return
        self.write_checkpoint(path, extra)

    def load(self, path):
        ck = torch.load(path, map_location="cpu")
        self.model.load_state_dict(ck["model_state_dict"])
        self.optimizer.load_state_dict(ck["optimizer_state_dict"])
        self.epoch = ck["epoch"]
        self.bucket.broadcast_parameters(0)
        return ck


def train_init_class(classifier, criterion, trainDataLoader, num_classes, num_part, num_epoch=500):
    """train_partseg_shapenet.py:56-99 with the reference's signature (plus the epoch count it hard-codes): pre-train the
    classifier layer `conv2` of `classifier` by logistic regression on the frozen network and return the classifier in train
    mode.  `criterion` must be the part-segmentation get_loss (cross-entropy on the log-probabilities): the fused loss is that
    one.  The reference unpacks three values from a model that returns five (:78) and cannot run as written; this runs what it
    states.  Sits on Trainer.init_classifier; `classifier` may be a Trainer (its model is pre-trained) or a model."""
    from .models import pointnet2_part_seg_msg as _msg
    if criterion is not None and not isinstance(criterion, _msg.get_loss):
        raise TypeError("train_init_class: the fused loss is models.pointnet2_part_seg_msg.get_loss, got %s" % type(criterion).__name__)
    if num_classes != 16:
        raise ValueError("train_init_class: the part-segmentation network takes a 16-way category one-hot, got num_classes=%d" % num_classes)
    trainer = classifier if isinstance(classifier, Trainer) else None
    model = trainer.model if trainer is not None else classifier
    if model.conv2.weight.shape[0] != num_part:
        raise ValueError("train_init_class: conv2 has %d outputs, num_part=%d" % (model.conv2.weight.shape[0], num_part))
    init_classifier(model, trainDataLoader, epochs=num_epoch)
    return model.train()

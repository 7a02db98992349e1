"""Evaluating a model over a section of a data set — the reference's nn/metrics/eval_utils.py (eval_metrics /
_eval_metrics_per_loader: called at the end of train.py, per folder by evaluation_scripts/on_test_set.py, per noise level by
noise_levels.py) — with everything between the first batch and the result on the device:

    ev = Evaluator(model, sampler)                       # sampler: staging.MeshPointSampler, for batches given as garment indices
    result = ev.run(batches, groups=folder_of_garment, seed=0)       # {'full_loss': ..., 'pattern_loss': ..., 'corr_rotation_l2': None, ...}
    ev.pooled                                            # {group or 'all': {quality key: value or None}}

Per batch: draw (optional) -> model.predict -> loss.accumulate, i.e. the launches of the prediction and of the loss plus ONE launch
of ops.EvalAccumulator, which applies the reference's rule on the device — per key the mean of the per-batch values, a batch whose
value is None left out of both the sum and the count; the sums are sequential fp32 adds in batch order, as `sum(list)` over 0-d
float32 arrays is.  No host read per batch; ONE at the end (the accumulator's state; with a table of per-garment records, a second
small tensor read along with it).

The reference's number depends on the batch size and on the ragged last batch (a mean of per-batch means, and of per-batch Nones).
`.pooled` is the batch-independent one for the quality metrics: the per-garment records the quality kernels write are kept in one
table for the whole set (ops.quality_metrics' `part`) and folded by ops.quality_pool per group and overall, bit for bit as one
batch of those garments would be.

capture=True replays the per-batch body from a hipGraph, captured once per distinct batch size (at most two: the full one and the
ragged last one; further sizes run eagerly) after `warmup` eager batches of that size, with the inputs copied into static buffers and
the decoders' host-drawn start states fed through graph.HostDrawn.  The eager batches are batches of the run, so the generator
draws, and with them the results, are those of capture=False bit for bit.  DESIGN.md section 5.39."""
import numpy as np
import torch

from . import graph
from . import metrics
from . import ops

MAX_CAPTURED_SIZES = 2


def _unwrap(model):
    """the model behind a DistributedHotPath / DataParallel-style wrapper (eval_utils.py:19)"""
    return model.module if hasattr(model, 'module') and hasattr(model.module, 'loss') else model


def _to_device(obj, device):
    if torch.is_tensor(obj):
        return obj.to(device)
    if isinstance(obj, dict):
        return {k: _to_device(v, device) for k, v in obj.items()}
    raise TypeError('a batch is (features or index tensor, ground truth tensor or dict of tensors); got %s' % type(obj).__name__)


def _like(obj):
    if obj is None or torch.is_tensor(obj):
        return None if obj is None else torch.empty_like(obj)
    return {k: torch.empty_like(v) for k, v in obj.items()}


def _flat(obj):
    return [obj] if torch.is_tensor(obj) else [obj[k] for k in obj]


class _Captured:
    """the per-batch body of one batch size: `warmup` eager batches, one capture, replays"""

    def __init__(self, device, warmup):
        self.host = graph.HostDrawn(device)
        self.eager_left = warmup
        self.graph = None
        self.static = None           # (x, ground truth, records) the captured body reads / writes


class Evaluator:
    def __init__(self, model, sampler=None, epoch=1000, capture=False, route='auto', warmup=2):
        """model: a model of this package in eval mode (or its DistributedHotPath wrapper: each rank evaluates what it is given);
        sampler: staging.MeshPointSampler (pattern models) or StitchPairSampler — needed when batches carry garment indices;
        epoch: the epoch the loss is evaluated at (which terms and quality components are on); route: model.predict's;
        capture / warmup: module docstring."""
        self.model = _unwrap(model)
        self.loss = getattr(self.model, 'loss', None)
        if not isinstance(self.loss, (metrics.ComposedPatternLoss, metrics.ComposedLoss)):
            raise TypeError('Evaluator serves models whose loss is ComposedPatternLoss or ComposedLoss (got %s)'
                            % type(self.loss).__name__)
        if route not in ops.EDGE_PREDICT_ROUTES:
            raise ValueError('unknown route %r (choose from %s)' % (route, ops.EDGE_PREDICT_ROUTES))
        self.sampler, self.epoch, self.capture, self.route = sampler, epoch, bool(capture), route
        self.warmup = max(int(warmup), 1)
        self.pooled = None
        self.accumulator = None
        self.table = None
        self._bodies = {}
        self._stream = None

    # ---- the per-batch body: what a capture records ----------------------------------------------------------------------------------
    def _body(self, x, gt, records):
        if x.is_floating_point():
            feats = x
        else:
            if self.sampler is None:
                raise ValueError('a batch of garment indices needs a sampler')
            drawn = self.sampler.sample(x)
            feats = drawn[0]
            if isinstance(self.loss, metrics.ComposedLoss):
                gt = drawn[1]                                   # the pair rows' labels are drawn with them
            self._worst.copy_(torch.minimum(self._worst, self.sampler.status.min()))
        if gt is None:
            raise ValueError('a batch without ground truth: only a pair sampler (garment indices in, rows and labels out) supplies its own')
        preds = self.model.predict(feats, route=self.route) if isinstance(self.loss, metrics.ComposedPatternLoss) \
            else self.model.predict(feats)
        self.loss.accumulate(preds, dict(gt) if isinstance(gt, dict) else gt, self.accumulator, epoch=self.epoch, records=records)

    def _replayed(self, x, gt, records):
        B = x.shape[0]
        cb = self._bodies.get(B)
        if cb is None:
            if len(self._bodies) >= MAX_CAPTURED_SIZES:
                return self._body(x, gt, records)
            cb = self._bodies[B] = _Captured(x.device, self.warmup)
        ops.HOST_DRAWN = cb.host
        try:
            cb.host.begin_step()
            if cb.eager_left > 0:
                cb.eager_left -= 1
                return self._body(x, gt, records)
            if cb.static is None:
                cb.static = (torch.empty_like(x), _like(gt), None if records is None else torch.zeros_like(records))
            sx, sgt, srec = cb.static
            dst, src = [sx] + (_flat(sgt) if sgt is not None else []), [x] + (_flat(gt) if gt is not None else [])
            if len(dst) != len(src) or any(d.shape != s.shape or d.dtype != s.dtype for d, s in zip(dst, src)):
                raise RuntimeError('Evaluator: batches of one size must have one layout (a captured body is one fixed shape)')
            for d, s in zip(dst, src):
                d.copy_(s, non_blocking=True)
            if cb.graph is None:
                g = torch.cuda.CUDAGraph()
                cb.host.capturing = True
                try:
                    with torch.cuda.graph(g, stream=self._stream):
                        self._body(sx, sgt, srec)
                finally:
                    cb.host.capturing = False
                cb.graph = g
                self.captures += 1
            cb.host.cursor = 0
            cb.graph.replay()
            self.replays += 1
            if records is not None:
                records.copy_(srec, non_blocking=True)
        finally:
            ops.HOST_DRAWN = None

    # ---- a pass over the set -----------------------------------------------------------------------------------------------------------
    def run(self, batches, groups=None, n_groups=None, seed=None, total=None):
        """batches: an iterable of (features or integer garment index [B], ground truth) — ground truth a dict of tensors for the
        pattern models, the labels for the pair classifier (None when the sampler draws them) — or a dict folder -> such an iterable
        (the reference's dict of loaders: one accumulator row per folder, the result a dict of dicts).
        groups: an integer [G] tensor or sequence, the group 0 .. n_groups-1 of every garment in visiting order, for the `.pooled`
        breakdown (an id outside that range: no group); n_groups defaults to the largest id + 1, which costs a host read of its own
        when `groups` lives on the device.  seed: sampler.reseed(seed, 0) first — two runs with one seed see the same clouds.
        total: the garments of the whole pass, the rows of the table of per-garment records.  With `total` or `groups` (whose length
        it is) the batches are consumed as they come, one at a time; with neither, a pattern model's batches are first collected
        into lists to count their garments — a loader is then held whole, so give `total` for a pass over a real data section.
        -> {'full_loss': ..., key: np.float32 or None}, the reference's rule (eval_utils.py:35-76)."""
        if self.model.training:
            raise RuntimeError('Evaluator.run evaluates the eval-mode model: call .eval() first (eval_utils.py:17)')
        if seed is not None and self.sampler is None:
            raise ValueError('Evaluator.run: seed= reseeds the sampler, and there is none')
        folders = list(batches.items()) if isinstance(batches, dict) else [(None, batches)]
        if not folders:
            raise ValueError('Evaluator.run: no batch to evaluate')
        device = next(self.model.parameters()).device
        if device.type != 'cuda':
            raise RuntimeError('Evaluator.run evaluates a model on the MI355X (its parameters live on %s); there is no CPU path' % device)
        pattern = isinstance(self.loss, metrics.ComposedPatternLoss)
        keys, gates = self.loss.eval_keys(self.epoch)
        with_table = pattern and self.loss.with_quality_eval and bool(self.loss.q_components)
        if groups is not None:
            groups = torch.as_tensor(groups)
            if total is not None and int(total) != groups.numel():
                raise ValueError('Evaluator.run: total = %d, but groups names %d garments' % (total, groups.numel()))
            total = groups.numel()
        if with_table and total is None:
            folders = [(name, list(it)) for name, it in folders]
            total = sum(b[0].shape[0] for _, bs in folders for b in bs)
        G = int(total) if with_table else 0
        if with_table and G < 1:
            raise ValueError('Evaluator.run: no batch to evaluate')
        self.accumulator = acc = ops.EvalAccumulator(keys, gates, slots=len(folders), device=device)
        self.table = torch.zeros(G, ops.QUALITY_WS_DOUBLES, device=device, dtype=torch.float64) if with_table else None
        self._worst = torch.zeros(1, device=device, dtype=torch.int32)
        self.captures = self.replays = 0
        self.pooled = self.pooled_counts = None
        self._bodies = {}            # a captured body holds this run's accumulator and the sampler's settings: captured per run
        outer = torch.cuda.current_stream(device)
        if self.capture and self._stream is None:
            self._stream = torch.cuda.Stream(device=device)
        stream = self._stream if self.capture else outer
        pooled_dev = None
        with torch.no_grad(), torch.cuda.stream(stream):
            if stream != outer:
                stream.wait_stream(outer)
            if seed is not None:
                self.sampler.reseed(seed, 0)
            g0 = n_batches = 0
            for row, (_, bs) in enumerate(folders):
                acc.set_slot(row)
                for x, gt in bs:
                    x = x.to(device)
                    gt = _to_device(gt, device) if gt is not None else None
                    if with_table and g0 + x.shape[0] > G:
                        raise ValueError('Evaluator.run: more garments than the %d that total / groups announced' % G)
                    records = self.table[g0:g0 + x.shape[0]] if with_table else None
                    (self._replayed if self.capture else self._body)(x, gt, records)
                    g0 += x.shape[0]
                    n_batches += 1
            if n_batches == 0:
                raise ValueError('Evaluator.run: no batch to evaluate')
            if with_table:
                if g0 != G:
                    raise ValueError('Evaluator.run: %d garments were visited, total / groups announced %d' % (g0, G))
                pooled_dev = self._pool(groups, n_groups, device)
            if stream != outer:
                outer.wait_stream(stream)
        rows = acc.read(along=[self._worst] + list(pooled_dev or ()))       # THE host read: the pooled rows and the status ride along
        worst = int(acc.last_along[0][0])
        if pooled_dev is not None:
            self.pooled = self._pooled_dicts(*acc.last_along[1:])
        if self.sampler is not None and worst < 0:
            raise ValueError('Evaluator.run: the sampler met a garment it cannot draw from (status %d: -1 nothing to draw, -2 an '
                             'index outside the set)' % worst)
        if isinstance(batches, dict):
            return {name: rows[i] for i, (name, _) in enumerate(folders)}
        return rows[0]

    def _pool(self, groups, n_groups, device):
        """-> ops.quality_pool of this run's table: (out fp32 [n_groups + 1, 14], counts int32 [n_groups + 1, 4]) on the device"""
        loss = self.loss
        flags = loss._quality_flags(self.epoch >= loss.config['epoch_with_stitches'])
        if groups is None:
            n_groups = 0
        else:
            if groups.dim() != 1 or groups.is_floating_point() or groups.dtype == torch.bool:
                raise ValueError('groups must be an integer [G] tensor: one id per garment in visiting order')
            if n_groups is None:
                n_groups = max(int(groups.max()) + 1, 0)
            groups = groups.to(device=device, dtype=torch.int32).contiguous()
        return ops.quality_pool(self.table, groups, int(n_groups), loss.max_pattern_size, loss.max_panel_len, flags)

    def _pooled_dicts(self, vals, cnts):
        """the rows of ops.quality_pool (on the host: fp32 [rows, 14], int32 [rows, 4]) as dicts {group or 'all': {quality key: value}}, None by the count rules of the loss dict
        (ops.QUALITY_GATES)"""
        present = [k[0] for k in self.accumulator.keys if k[0] in ops.QUALITY_KEYS]
        self.pooled_counts = cnts
        rows = vals.shape[0]
        return {('all' if r == rows - 1 else r): {
            k: (None if k in ops.QUALITY_GATES and cnts[r, ops.QUALITY_GATES[k]] <= 0 else vals[r, ops.QUALITY_KEYS.index(k)])
            for k in present} for r in range(rows)}


def eval_metrics(model, batches, sampler=None, **kw):
    """The reference's shortcut (eval_utils.py:12-32): model.eval(), quality evaluation forced on, no_grad, the wrapped module of a
    multi-GPU wrapper; batches as Evaluator.run takes them (a dict of folders -> a dict of dicts).  Keywords epoch / capture / route /
    warmup go to the Evaluator, groups / n_groups / seed to run."""
    inner = _unwrap(model)
    inner.eval()
    if hasattr(inner.loss, 'with_quality_eval'):
        inner.loss.with_quality_eval = True
    run_kw = {k: kw.pop(k) for k in ('groups', 'n_groups', 'seed', 'total') if k in kw}
    with torch.no_grad():
        return Evaluator(inner, sampler, **kw).run(batches, **run_kw)

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
draws, and with them the results, are those of capture=False bit for bit.  DESIGN.md section 5.39.

FrameworkEvaluator / eval_framework run both stages in one pass (the reference's evaluation_scripts/on_test_set.py -st ... -corr):
the same first stage, then every prediction decoded, placed and handed to the edge-pair classifier, scored per garment and folded
on the device — again one host read per set.  DESIGN.md section 5.42."""
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
    def _begin_pass(self, slots, G, with_table, device, accumulate=True):
        """the state of a fresh pass: the accumulator of `slots` rows and the table of G per-garment records (neither with
        accumulate=False: a caller that only wants predict_batch), the sampler's worst status, the captured bodies"""
        if accumulate:
            keys, gates = self.loss.eval_keys(self.epoch)
            self.accumulator = ops.EvalAccumulator(keys, gates, slots=slots, device=device)
        else:
            self.accumulator = None
        self.table = torch.zeros(G, ops.QUALITY_WS_DOUBLES, device=device, dtype=torch.float64) if with_table else None
        self._worst = torch.zeros(1, device=device, dtype=torch.int32)
        self.captures = self.replays = 0
        self.pooled = self.pooled_counts = None
        self._bodies = {}            # a captured body holds this run's accumulator and the sampler's settings: captured per run

    def predict_batch(self, x, gt):
        """the first half of the per-batch body: the clouds drawn when x holds garment indices (the sampler's worst status kept on
        the device), then model.predict -> (predictions, ground truth: the sampler's labels for the pair classifier)"""
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
        return preds, gt

    def _body(self, x, gt, records):
        preds, gt = self.predict_batch(x, gt)
        self.loss.accumulate(preds, dict(gt) if isinstance(gt, dict) else gt, self.accumulator, epoch=self.epoch, records=records)
        return preds

    def _close_pass(self, rows, worst, pooled_host, what='Evaluator.run'):
        """after the host read: `.pooled` from the pooled rows that rode along, the sampler's worst status looked at once -> rows"""
        if pooled_host is not None:
            self.pooled = self._pooled_dicts(*pooled_host)
        if self.sampler is not None and worst < 0:
            raise ValueError('%s: the sampler met a garment it cannot draw from (status %d: -1 nothing to draw, -2 an '
                             'index outside the set)' % (what, worst))
        return rows

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
        self._begin_pass(len(folders), G, with_table, device)
        acc = self.accumulator
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
        self._close_pass(rows, int(acc.last_along[0][0]), acc.last_along[1:] if pooled_dev is not None else None)
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


FRAMEWORK_LABELS = ('ground_truth', 'tags')


class FrameworkEvaluator:
    """Both stages over a section of a data set — the reference's nn/evaluation_scripts/on_test_set.py -st ... -corr — in one pass with
    ONE host read: the pattern model's predictions are decoded to sewing patterns with the ground-truth stitches propagated onto them
    (Garment3DPatternFullDataset.save_prediction_batch / _pred_to_pattern, nn/data/datasets.py:675-693, 731-767), placed in 3D, and the
    edge-pair classifier is scored on all edge pairs of every usable pattern, one garment per "batch" of the reference's rule
    (GarmentStitchPairsDataset._clean_datapoint_list :1134-1159, nn/metrics/eval_utils.py:35-76), once for all usable patterns
    ('stitch': the reference's test_preds_full / test_preds) and once for those with the right number of panels ('stitch_corr':
    test_corr_full / test_corr).

        ev = FrameworkEvaluator(pattern_model, stitch_model, data_config, stitch_data_stats, sampler)
        result = ev.run(batches, groups=folder_of_garment, seed=0)
        # {'shape': Evaluator's dict, 'stitch': {...}, 'stitch_corr': {...}, 'skipped': {reason: garments}}
        ev.pooled        # {group or 'all': {'stitch': {...}, 'stitch_corr': {...}, 'counts': {...}}}: independent of the batching
        ev.records       # the device table, one record per garment (ops.FRAMEWORK_RECORD)

    Per batch, no host read: draw (optional) -> pattern_model.predict -> loss.accumulate (shape_metrics: the first stage's own
    result from the same prediction, exactly Evaluator's) -> ops.pattern_decode -> place -> stitch_model.evaluate_stitches on the
    decoded pattern's label stitches -> ops.FrameworkAccumulator.add.  labels='ground_truth' gives the decode gt['stitches'] (all S
    entries: the reference walks them all and skips (0, 0)); labels='tags' pairs the predicted stitch tags, which is what the
    reference is left with when it cannot propagate ground truth (:676-680).  DESIGN.md section 5.42."""

    def __init__(self, pattern_model, stitch_model, data_config, stitch_data_stats, sampler=None, labels='ground_truth', route='auto',
                 stitch_route='auto', shape_metrics=True, epoch=1000):
        if labels not in FRAMEWORK_LABELS:
            raise ValueError('unknown labels %r (choose from %s)' % (labels, FRAMEWORK_LABELS))
        if route not in ops.EDGE_PREDICT_ROUTES:
            raise ValueError('unknown route %r (choose from %s)' % (route, ops.EDGE_PREDICT_ROUTES))
        if stitch_route not in ops.STITCH_PAIRS_ROUTES:
            raise ValueError('unknown stitch_route %r (choose from %s)' % (stitch_route, ops.STITCH_PAIRS_ROUTES))
        self.model, self.stitch_model = _unwrap(pattern_model), _unwrap(stitch_model)
        if not isinstance(getattr(self.model, 'loss', None), metrics.ComposedPatternLoss):
            raise TypeError('FrameworkEvaluator: the first model must predict patterns (a loss of ComposedPatternLoss; got %s)'
                            % type(getattr(self.model, 'loss', None)).__name__)
        if not hasattr(self.stitch_model, 'evaluate_stitches'):
            raise TypeError('FrameworkEvaluator: the second model must be the edge-pair classifier (StitchOnEdge3DPairs; got %s)'
                            % type(self.stitch_model).__name__)
        for k in ('f_shift', 'f_scale'):
            if k not in stitch_data_stats:
                raise ValueError('FrameworkEvaluator: stitch_data_stats has no %r' % k)
        if 'standardize' not in data_config:
            raise ValueError("FrameworkEvaluator: data_config has no 'standardize'")
        self.data_config, self.stitch_data_stats = data_config, stitch_data_stats
        self.sampler, self.labels, self.route, self.stitch_route, self.epoch = sampler, labels, route, stitch_route, epoch
        # the first stage is Evaluator's: its draw and predict always, its accumulate and pooling with shape_metrics (`.shape`)
        self.first = Evaluator(self.model, sampler, epoch=epoch, route=route)
        self.shape = self.first if shape_metrics else None
        self.accumulator = self.pooled = self.records = None
        self._slots = 0

    def _check_modes(self, what):
        if self.model.training or self.stitch_model.training:
            raise RuntimeError('%s evaluates the eval-mode models: call .eval() first (eval_utils.py:17)' % what)
        devices = [next(m.parameters()).device for m in (self.model, self.stitch_model)]
        for device in devices:
            if device.type != 'cuda':
                raise RuntimeError('%s evaluates a model on the MI355X (its parameters live on %s); there is no CPU path' % (what, device))
        if devices[0] != devices[1]:
            raise RuntimeError('%s: the pattern model lives on %s, the stitch model on %s; one pass runs on one device'
                               % (what, devices[0], devices[1]))
        return devices[0]

    def _check_gt(self, gt):
        if not isinstance(gt, dict):
            raise ValueError('FrameworkEvaluator: ground truth must be a dict of tensors with \'stitches\' and \'num_panels\'')
        for k in (('stitches', 'num_panels') if self.labels == 'ground_truth' else ('num_panels',)):
            if k not in gt:
                raise ValueError('FrameworkEvaluator: ground truth has no %r' % k)

    # ---- a pass in three calls: begin, add_predictions per batch, finish --------------------------------------------------------------
    def begin(self, total, slots=1):
        """a new pass of `total` garments over `slots` data folders: fresh accumulators (-> the ops.FrameworkAccumulator)"""
        device = self._check_modes('FrameworkEvaluator')
        self.accumulator = ops.FrameworkAccumulator(slots=slots, total=total, device=device)
        self.pooled = self.records = None
        return self.accumulator

    def add_predictions(self, preds, gt, rows=None):
        """one batch of predictions the caller already has (model.predict's dict, or stored predictions: on_test_set.py --pred_path)
        through decode -> place -> classifier -> accumulate; `rows`: fp64 [B, 10] to receive the records instead of the next B rows
        of the pass's table.  No host read.  -> the placed DecodedPatterns"""
        if self.accumulator is None:
            raise RuntimeError('FrameworkEvaluator.add_predictions: call begin(total, slots) first')
        self._check_gt(gt)
        self._check_modes('FrameworkEvaluator.add_predictions')
        from .patterns import DecodedPatterns
        with torch.no_grad():
            stats = self.data_config['standardize']
            if self.labels == 'ground_truth':
                decoded = ops.pattern_decode(preds, stats, stitches=gt['stitches'], num_stitches=None)
            else:
                decoded = ops.pattern_decode(preds, stats, bool(self.data_config.get('explicit_stitch_tags', False)))
            d = DecodedPatterns(decoded).place()
            out, _ = self.stitch_model.evaluate_stitches(d.edges3d, d.num_edges, *d.label_stitches(), self.stitch_data_stats,
                                                         route=self.stitch_route)
            self.accumulator.add(out, d, gt['num_panels'], records=rows)
        return d

    def finish(self, groups=None, n_groups=None, along=()):
        """pool, then THE host read -> one result dict per slot ({'stitch', 'stitch_corr', 'skipped'}); sets .pooled and .records.
        along: device tensors to bring over in the same transfer (-> self.last_along)"""
        acc = self.accumulator
        if acc is None or acc.rows < 1:
            raise ValueError('FrameworkEvaluator: no batch to evaluate')
        if groups is None:
            n_groups = 0
        else:
            groups = torch.as_tensor(groups)
            if groups.dim() != 1 or groups.is_floating_point() or groups.dtype == torch.bool:
                raise ValueError('groups must be an integer [G] tensor: one id per garment in visiting order')
            if groups.numel() != acc.rows:
                raise ValueError('FrameworkEvaluator: %d garments were visited, groups names %d' % (acc.rows, groups.numel()))
            if n_groups is None:
                n_groups = max(int(groups.max()) + 1, 0)
            groups = groups.to(device=acc.device, dtype=torch.int32).contiguous()
        pooled_dev = acc.pool(groups, int(n_groups))
        rows = acc.read(along=list(pooled_dev) + list(along))
        self.last_along = acc.last_along[3:]
        self._set_pooled(*acc.last_along[:3])
        return rows

    def _set_pooled(self, totals, loss, ratios):
        """the rows of FrameworkAccumulator.pool on the host as dicts {group or 'all': {...}}"""
        rows = totals.shape[0]
        self.pooled, self.pooled_raw = {}, (totals, loss, ratios)
        for r in range(rows):
            entry = {name: {k: ratios[r, i, j] for j, k in enumerate(ops.STITCH_EVAL_METRICS)} for i, name in enumerate(ops.FRAMEWORK_SETS)}
            entry['counts'] = {name: dict({k: int(totals[r, i, j]) for j, k in enumerate(ops.FRAMEWORK_TOTALS)}, loss_sum=loss[r, i])
                               for i, name in enumerate(ops.FRAMEWORK_SETS)}
            self.pooled['all' if r == rows - 1 else r] = entry
        self.records = self.accumulator.table[:self.accumulator.rows]

    # ---- a pass over the set -------------------------------------------------------------------------------------------------------------
    def run(self, batches, groups=None, n_groups=None, seed=None, total=None):
        """batches, groups, n_groups, seed and total as Evaluator.run takes them (ground truth: a dict with 'stitches' and
        'num_panels' besides what the pattern loss reads).  -> {'shape': Evaluator.run's dict (with shape_metrics), 'stitch': {...},
        'stitch_corr': {...}, 'skipped': {...}}, or a dict folder -> such a dict."""
        device = self._check_modes('FrameworkEvaluator.run')
        if seed is not None and self.sampler is None:
            raise ValueError('FrameworkEvaluator.run: seed= reseeds the sampler, and there is none')
        folders = list(batches.items()) if isinstance(batches, dict) else [(None, batches)]
        if not folders:
            raise ValueError('FrameworkEvaluator.run: no batch to evaluate')
        if groups is not None:
            groups = torch.as_tensor(groups)
            if total is not None and int(total) != groups.numel():
                raise ValueError('FrameworkEvaluator.run: total = %d, but groups names %d garments' % (total, groups.numel()))
            total = groups.numel()
            if n_groups is None and groups.dim() == 1 and not groups.is_floating_point() and groups.numel():
                n_groups = max(int(groups.max()) + 1, 0)            # once for both stages' pooling (a host read when on the device)
        if total is None:
            folders = [(name, list(it)) for name, it in folders]
            total = sum(b[0].shape[0] for _, bs in folders for b in bs)
        G = int(total)
        if G < 1:
            raise ValueError('FrameworkEvaluator.run: no batch to evaluate')
        acc = self.begin(G, len(folders))
        first, shape = self.first, self.shape is not None
        with_table = shape and first.loss.with_quality_eval and bool(first.loss.q_components)
        first._begin_pass(len(folders), G if with_table else 0, with_table, device, accumulate=shape)
        with torch.no_grad():
            if seed is not None:
                self.sampler.reseed(seed, 0)
            g0 = 0
            for row, (_, bs) in enumerate(folders):
                acc.set_slot(row)
                if shape:
                    first.accumulator.set_slot(row)
                for x, gt in bs:
                    x = x.to(device)
                    gt = _to_device(gt, device) if gt is not None else None
                    self._check_gt(gt)
                    B = x.shape[0]
                    if g0 + B > G:
                        raise ValueError('FrameworkEvaluator.run: more garments than the %d that total / groups announced' % G)
                    if shape:
                        preds = first._body(x, gt, first.table[g0:g0 + B] if with_table else None)
                    else:
                        preds, _ = first.predict_batch(x, gt)
                    self.add_predictions(preds, gt)
                    g0 += B
            if g0 != G:
                raise ValueError('FrameworkEvaluator.run: %d garments were visited, total / groups announced %d' % (g0, G))
            shape_pooled = list(first._pool(groups, n_groups, device)) if with_table else []
            shape_state = [first.accumulator.state] if shape else []
        rows = self.finish(groups, n_groups, along=[first._worst] + shape_state + shape_pooled)      # THE host read
        shape_rows = first.accumulator.parse(self.last_along[1]) if shape else None
        first._close_pass(shape_rows, int(self.last_along[0][0]), self.last_along[2:4] if with_table else None,
                          what='FrameworkEvaluator.run')
        if shape:
            for r, s_ in zip(rows, shape_rows):
                r['shape'] = s_
        rows = [{k: r[k] for k in ('shape', 'stitch', 'stitch_corr', 'skipped') if k in r} for r in rows]
        if isinstance(batches, dict):
            return {name: rows[i] for i, (name, _) in enumerate(folders)}
        return rows[0]


def eval_framework(pattern_model, stitch_model, data_config, stitch_data_stats, batches, sampler=None, **kw):
    """The two-stage pass in one call (on_test_set.py -st ... -corr): both models to eval mode, the first stage's quality evaluation
    forced on as eval_metrics does, no_grad.  Keywords labels / route / stitch_route / shape_metrics / epoch go to the
    FrameworkEvaluator, groups / n_groups / seed / total to run.  -> FrameworkEvaluator.run's result."""
    inner, stitch = _unwrap(pattern_model), _unwrap(stitch_model)
    inner.eval()
    stitch.eval()
    if hasattr(inner.loss, 'with_quality_eval'):
        inner.loss.with_quality_eval = True
    run_kw = {k: kw.pop(k) for k in ('groups', 'n_groups', 'seed', 'total') if k in kw}
    with torch.no_grad():
        return FrameworkEvaluator(inner, stitch, data_config, stitch_data_stats, sampler, **kw).run(batches, **run_kw)


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

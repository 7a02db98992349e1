"""Evaluation on the device: the quality metrics and their accumulator (quality_metrics, quality_pool, EvalAccumulator), a
prediction decoded to a sewing pattern and placed in 3D (pattern_decode, pattern_place), and the accumulator of the two-stage
framework (FrameworkAccumulator).  Reached as ops.X: ops.py re-exports every name of __all__.  The scoring of the stitch classifier
itself (stitch_pairs_eval, STITCH_EVAL_*) is in ops_stitch, with the classifier."""
import numpy as np
import torch

from . import _lib as L
from ._opbase import F32, F64, _dev_check, _row_stride, _view_strides
from .ops_stitch import STITCH_EVAL_COUNTS, STITCH_EVAL_METRICS

__all__ = ['QM_DISCRETE', 'QM_SHAPE', 'QM_ROT', 'QM_TR', 'QM_STITCH', 'QM_FREE', 'QM_TAG_STATS', 'QUALITY_KEYS',
           'QUALITY_WS_DOUBLES', 'quality_stats', 'quality_metrics', 'quality_pool', 'QUALITY_GATES', 'EVAL_MAX_KEYS',
           'EVAL_MAX_SOURCES', 'EvalAccumulator', 'PATTERN_DECODE_KEYS', 'PATTERN_MAX_EDGES', 'PATTERN_MAX_WIDTH',
           'tags_to_stitches', 'pattern_decode', 'PATTERN_PLACE_KEYS', 'PATTERN_PLACE_INPUTS', 'PLACE_BAD_QUAT',
           'pattern_place', 'FRAMEWORK_EVAL_KEYS', 'FRAMEWORK_SKIP_REASONS', 'FRAMEWORK_SETS', 'FRAMEWORK_RECORD',
           'FRAMEWORK_TOTALS', 'FRAMEWORK_MAX_PANELS', 'FrameworkAccumulator']


QM_DISCRETE, QM_SHAPE, QM_ROT, QM_TR, QM_STITCH, QM_FREE, QM_TAG_STATS = 1, 2, 4, 8, 16, 32, 64
QUALITY_KEYS = ('num_panels_accuracy', 'num_edges_accuracy', 'corr_num_edges_accuracy', 'panel_shape_l2',
                'corr_panel_shape_l2', 'rotation_l2', 'corr_rotation_l2', 'translation_l2', 'corr_translation_l2',
                'stitch_precision', 'stitch_recall', 'corr_stitch_precision', 'corr_stitch_recall', 'free_edge_acc')
QUALITY_WS_DOUBLES = 16          # include/gpe_hip.h: `part` holds B * 16 doubles


def quality_stats(ol_stats, rot_stats=None, tr_stats=None, tag_stats=None):
    """The 72-float host array `stats_host` of the quality entry points (include/gpe_hip.h), from the {'shift', 'scale'} stats
    of the outlines / rotations / translations / stitch tags.  The pad vector, its isclose tolerance and the loop-closure
    threshold are formed with torch fp32 arithmetic, as nn/metrics/metrics.py:107-109 and torch.isclose form them."""
    import ctypes
    v = [0.0] * 72
    sh = torch.tensor(ol_stats['shift'], dtype=F32)
    sc = torch.tensor(ol_stats['scale'], dtype=F32)
    pad = -sh / sc
    tol = 0.07 + (1e-5 * pad).abs()                 # torch.isclose(atol=0.07, rtol=1e-5) against the pad vector
    thr = torch.tensor([3, 3]) / sc[:2]             # 3 cm per coordinate
    v[0:4], v[4:8], v[8:12], v[12:16], v[16:18] = sh.tolist(), sc.tolist(), pad.tolist(), tol.tolist(), thr.tolist()
    for base, st in ((24, rot_stats), (40, tr_stats), (56, tag_stats)):
        if st is not None:
            s_, c_ = [float(x) for x in st['shift']], [float(x) for x in st['scale']]
            if len(s_) > 8:
                raise ValueError('quality metrics support feature widths <= 8 (got %d)' % len(s_))
            v[base:base + len(s_)], v[base + 8:base + 8 + len(c_)] = s_, c_
    return (ctypes.c_float * 72)(*v)


def quality_metrics(flags, stats, B, P, Lp, outlines=None, gt_outlines=None, num_edges=None, num_panels=None, rotations=None,
                    gt_rotations=None, translations=None, gt_translations=None, stitch_tags=None, free_logits=None,
                    stitches=None, nums=None, gt_free_mask=None, part=None):
    """ComposedPatternLoss quality metrics (nn/metrics/composed_loss.py:365-424) in <= 3 launches, no host read:
    -> (out fp32 [14] in the order of QUALITY_KEYS, counts int32 [4]: contributors of the corr_ slots, include/gpe_hip.h).
    `flags` selects the components (QM_*), `stats` is quality_stats(...).  Predictions are the strided views of the decoders'
    outputs; ground truth is what the loss matched (order / origin), any dtype (converted on the device).
    `part`: a caller-owned workspace for the per-pattern records, fp64 [B, 16] — B rows of a larger table that quality_pool folds
    later with the same flags; the default is a private one."""
    ref = outlines if outlines is not None else free_logits
    _dev_check(ref)
    dev = ref.device
    if part is None:
        part = torch.empty(B * QUALITY_WS_DOUBLES, device=dev, dtype=torch.float64)
    else:
        _quality_table(part, 'quality_metrics: part', B)
        if part.device != dev:
            raise ValueError('quality_metrics: part lives on %s, the predictions on %s' % (part.device, dev))
    out = torch.empty(len(QUALITY_KEYS), device=dev, dtype=F32)
    counts = torch.empty(4, device=dev, dtype=torch.int32)
    main = flags & (QM_DISCRETE | QM_SHAPE | QM_ROT | QM_TR)
    if main:
        need_ol = flags & (QM_DISCRETE | QM_SHAPE)
        ol = outlines.detach() if need_ol else None
        sb, sp, sl = _view_strides(ol) if need_ol else (0, 0, 0)
        gto = gt_outlines.float().contiguous() if flags & QM_SHAPE else None
        ne = num_edges.reshape(-1).to(torch.int32).contiguous() if need_ol else None
        npn = num_panels.reshape(-1).to(torch.int32).contiguous() if flags & QM_DISCRETE else None
        rot = rotations.detach() if flags & QM_ROT else None
        tr = translations.detach() if flags & QM_TR else None
        R = rot.shape[-1] if rot is not None else 0
        T = tr.shape[-1] if tr is not None else 0
        for t in (ol, rot, tr):
            if t is not None:
                _dev_check(t)
        L.call('gpe_quality_panels', ol, sb, sp, sl, gto, ne, npn,
               rot, _row_stride(rot, P) if rot is not None else 0,
               gt_rotations.float().contiguous() if rot is not None else None, R,
               tr, _row_stride(tr, P) if tr is not None else 0,
               gt_translations.float().contiguous() if tr is not None else None, T,
               B, P, Lp, main, stats, part)
    st_flags = flags & (QM_STITCH | QM_FREE | QM_TAG_STATS)
    if st_flags & (QM_STITCH | QM_FREE):
        lg = free_logits.detach()
        _dev_check(lg)
        tags = stitch_tags.detach() if flags & QM_STITCH else None
        if tags is not None:
            _dev_check(tags)
        ts = _view_strides(tags) if tags is not None else (0, 0, 0)
        L.call('gpe_quality_stitches', tags, ts[0], ts[1], ts[2], tags.shape[3] if tags is not None else 0,
               lg, lg.stride(0), lg.stride(1), lg.stride(2),
               stitches.long().contiguous() if tags is not None else None,
               nums.reshape(-1).long().contiguous() if tags is not None else None,
               stitches.shape[-1] if tags is not None else 0,
               gt_free_mask.float().contiguous() if flags & QM_FREE else None, B, P, Lp, st_flags, stats, part)
    L.call('gpe_quality_finalize', part, B, P, Lp, flags, out, counts)
    return out, counts


def _quality_table(t, what, rows=None):
    if (not torch.is_tensor(t) or t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != QUALITY_WS_DOUBLES or t.shape[0] < 1
            or not t.is_contiguous() or (rows is not None and t.shape[0] != rows)):
        raise ValueError('%s must be a contiguous fp64 [%s, %d] tensor (got %s %s)'
                         % (what, 'G' if rows is None else rows, QUALITY_WS_DOUBLES, getattr(t, 'dtype', type(t).__name__),
                            tuple(getattr(t, 'shape', ()))))
    if not t.is_cuda:
        raise RuntimeError('gpe ops need tensors on the MI355X (got a %s table); there is no CPU path' % t.device)


def quality_pool(table, group, n_groups, P, Lp, flags):
    """The per-garment records of a whole data set (the `part` rows quality_metrics wrote, fp64 [G, 16]) folded per group and
    overall: -> (out fp32 [n_groups + 1, 14], counts int32 [n_groups + 1, 4]).  Row g is bit for bit what quality_metrics returns
    for the garments of group g alone, in table order, as one batch; the last row covers all garments.  group: int32 [G] on the
    device (an id outside 0 .. n_groups-1 belongs to no group), or None with n_groups = 0.  One launch (include/gpe_hip_eval.h
    gpe_eval_pool), no host read."""
    _quality_table(table, 'quality_pool: table')
    G = table.shape[0]
    if isinstance(n_groups, bool) or not isinstance(n_groups, int) or not 0 <= n_groups <= 65535:
        raise ValueError('quality_pool: n_groups must be an integer in 0 .. 65535 (got %r)' % (n_groups,))
    if group is None:
        if n_groups:
            raise ValueError('quality_pool: %d groups need a group id per garment' % n_groups)
    elif (not torch.is_tensor(group) or group.dtype != torch.int32 or tuple(group.shape) != (G,) or group.device != table.device
          or not group.is_contiguous()):
        raise ValueError('quality_pool: group must be a contiguous int32 [%d] tensor on the device of the table' % G)
    out = torch.empty(n_groups + 1, len(QUALITY_KEYS), device=table.device, dtype=F32)
    counts = torch.empty(n_groups + 1, 4, device=table.device, dtype=torch.int32)
    L.call('gpe_eval_pool', table, group, G, n_groups, int(P), int(Lp), int(flags), out, counts)
    return out, counts


# QUALITY_KEYS index -> the contributor count (of the int32 [4] counts) that must be positive for the key to have a value; the other
# keys always have one (corr_num_edges_accuracy included: the reference averages its 0 / 0 NaN in).  metrics._main_quality_metrics /
# _stitch_quality_metrics apply these rules on the host, EvalAccumulator and Evaluator.pooled on the device / after the one read.
QUALITY_GATES = {'corr_panel_shape_l2': 1, 'corr_rotation_l2': 0, 'corr_translation_l2': 0, 'corr_stitch_precision': 2,
                 'corr_stitch_recall': 2}
EVAL_MAX_KEYS, EVAL_MAX_SOURCES = 64, 4


class EvalAccumulator:
    """The reference's evaluation rule (nn/metrics/eval_utils.py:35-76: per key the mean of the per-batch values, a batch whose value is
    None skipped) kept on the device: one launch per batch (include/gpe_hip_eval.h gpe_eval_add), ONE host read at the end.

        acc = EvalAccumulator([('full_loss', 3, 0), ('pattern_loss', 0, 1), ('corr_rotation_l2', 2, 6)], {'corr_rotation_l2': 0})
        for ...: acc.add(loss_vec, None, quality_vec, misc_vec, counts=counts)
        result = acc.read()[0]             # {'full_loss': np.float32, ..., 'corr_rotation_l2': np.float32 or None}

    keys: (name, source, index) per key, in the order of the result dict: the value of `name` in a batch is sources[source][index].
    gates: {name: j} — the key is counted in a batch iff counts[j] > 0 (counts: quality_metrics' int32 [4]); other keys always.
    slots: rows of accumulators (one per data folder); `.slot` is the device word that names the row the next add() goes to, set by
    set_slot(i) as a queued copy — a captured add() serves every row."""

    def __init__(self, keys, gates=None, slots=1, device='cuda'):
        import ctypes
        keys, gates = [tuple(k) for k in keys], dict(gates or {})
        if not 1 <= len(keys) <= EVAL_MAX_KEYS:
            raise ValueError('EvalAccumulator: 1 .. %d keys (got %d)' % (EVAL_MAX_KEYS, len(keys)))
        if isinstance(slots, bool) or not isinstance(slots, int) or slots < 1:
            raise ValueError('EvalAccumulator: slots must be a positive integer (got %r)' % (slots,))
        names = [k[0] for k in keys]
        if len(set(names)) != len(names) or set(gates) - set(names):
            raise ValueError('EvalAccumulator: key names must be distinct and every gate must name a key')
        packed = []
        for name, src, idx in keys:
            g = gates.get(name)
            if not (0 <= src < EVAL_MAX_SOURCES and 0 <= idx < 256 and (g is None or 0 <= g < 4)):
                raise ValueError('EvalAccumulator: key %r: source 0 .. 3, index 0 .. 255, gate 0 .. 3 (got %r, %r, %r)' % (name, src, idx, g))
            packed.append(idx | (src << 8) | ((0 if g is None else g + 1) << 16))
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('gpe ops need tensors on the MI355X (got device %s); there is no CPU path' % self.device)
        self.keys, self.names, self.gated, self.slots = keys, names, bool(gates), slots
        self.n_sources = 1 + max(k[1] for k in keys)
        self._need = [1 + max([k[2] for k in keys if k[1] == s], default=-1) for s in range(self.n_sources)]
        self._packed = (ctypes.c_int32 * len(packed))(*packed)
        K = len(keys)
        # one allocation, one read: sum [slots, K] as its fp32 bits | cnt [slots, K] | batches [slots] | status [1]
        self.state = torch.zeros(2 * slots * K + slots + 1, device=self.device, dtype=torch.int32)
        self.sum = self.state[:slots * K].view(F32).view(slots, K)
        self.cnt = self.state[slots * K:2 * slots * K].view(slots, K)
        self.batches = self.state[2 * slots * K:2 * slots * K + slots]
        self.status = self.state[-1:]
        self.slot = torch.zeros(1, device=self.device, dtype=torch.int32)
        self._slot_host = torch.arange(slots, dtype=torch.int32).pin_memory()      # sources of set_slot's queued one-word copies

    def reset(self):
        """sums, counts, batches and the status back to zero, the slot word to row 0 (queued; no device read)"""
        self.state.zero_()
        self.slot.zero_()

    def set_slot(self, i):
        """the following add() calls go to row i: a queued copy from pinned memory, no device read"""
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < self.slots:
            raise ValueError('EvalAccumulator.set_slot: row 0 .. %d (got %r)' % (self.slots - 1, i))
        self.slot.copy_(self._slot_host[i:i + 1], non_blocking=True)

    def add(self, *sources, counts=None):
        """one batch: sources[s] is the fp32 device vector the keys of source s index (None where no key refers to it)"""
        if len(sources) > EVAL_MAX_SOURCES or len(sources) < self.n_sources:
            raise ValueError('EvalAccumulator.add: %d .. %d source vectors (got %d)' % (self.n_sources, EVAL_MAX_SOURCES, len(sources)))
        args = []
        for s in range(EVAL_MAX_SOURCES):
            t = sources[s] if s < len(sources) else None
            need = self._need[s] if s < self.n_sources else 0
            if t is None:
                if need:
                    raise ValueError('EvalAccumulator.add: source %d is None but keys refer to it' % s)
                args += [None, 0]
                continue
            if not torch.is_tensor(t) or t.dtype != F32 or t.dim() != 1 or not t.is_contiguous() or t.numel() < need or t.numel() > 256:
                raise ValueError('EvalAccumulator.add: source %d must be a contiguous fp32 vector of %d .. 256 values (got %s %s)'
                                 % (s, need, getattr(t, 'dtype', type(t).__name__), tuple(getattr(t, 'shape', ()))))
            _dev_check(t)
            args += [t.detach(), t.numel()]
        if self.gated and counts is None:
            raise ValueError('EvalAccumulator.add: gated keys need the contributor counts')
        if counts is not None and (counts.dtype != torch.int32 or counts.numel() != 4 or not counts.is_contiguous() or not counts.is_cuda):
            raise ValueError('EvalAccumulator.add: counts must be a contiguous int32 [4] device tensor')
        L.call('gpe_eval_add', *args, len(sources), counts, self._packed, len(self.keys), self.sum, self.cnt, self.batches, self.slot,
               self.slots, self.status)

    def read(self, along=()):
        """THE host read -> one dict per row: np.float32(sum) / np.float32(cnt) per key, None where the key was never counted (the
        reference's None for an empty list).  `.last_sums` / `.last_counts` / `.last_batches` keep what was read.  along: further
        device tensors of fp32 / int32 to bring over in the same transfer; `.last_along` holds them as numpy arrays of their own
        dtype and shape, in order."""
        along = [t.detach() for t in along]
        if any(t.dtype not in (F32, torch.int32) or t.device != self.state.device for t in along):
            raise ValueError('EvalAccumulator.read: along takes fp32 / int32 tensors on the accumulator\'s device')
        parts = [self.state] + [t.contiguous().view(torch.int32).reshape(-1) for t in along]
        host = (torch.cat(parts) if along else self.state).cpu().numpy()
        edges = np.cumsum([p.numel() for p in parts])
        self.last_along = [host[a:b].view(np.float32 if t.dtype == F32 else np.int32).reshape(tuple(t.shape))
                           for a, b, t in zip(edges[:-1], edges[1:], along)]
        return self.parse(host[:edges[0]])

    def parse(self, host):
        """read()'s result from `.state` as it arrived on the host (int32 numpy): for a caller that brought the state over in a
        transfer of its own (evaluation.FrameworkEvaluator reads it along with the second stage's accumulator)"""
        K, S = len(self.keys), self.slots
        if host[-1]:
            raise RuntimeError('EvalAccumulator: an add() met a slot word outside 0 .. %d and was dropped' % (S - 1))
        sums = host[:S * K].view(np.float32).reshape(S, K)
        cnts = host[S * K:2 * S * K].reshape(S, K)
        self.last_sums, self.last_counts, self.last_batches = sums, cnts, host[2 * S * K:2 * S * K + S]
        return [{n: (np.float32(sums[s, k]) / np.float32(cnts[s, k]) if cnts[s, k] else None) for k, n in enumerate(self.names)}
                for s in range(S)]


# -------------------------------------------------------------------------------------------------
# a prediction decoded to a sewing pattern (csrc/gpe_pattern_decode.hip)
# -------------------------------------------------------------------------------------------------
PATTERN_DECODE_KEYS = ('num_edges', 'edge_slot', 'num_verts', 'closed', 'new_panel_id', 'num_panels', 'vertices', 'curvature',
                       'rotations', 'translations', 'curved', 'stitches', 'num_stitches', 'stitch_flags', 'first_invalid')
PATTERN_MAX_EDGES, PATTERN_MAX_WIDTH = 1024, 8          # include/gpe_hip.h gpe_pattern_decode: P * L, and R / T / D


def _pattern_decode_stats(data_stats, widths, explicit_stitch_tags):
    """the 64-double host array `stats_host` of gpe_pattern_decode from data_config['standardize'] (Python floats are doubles: the
    statistics reach the kernel as the reference's numpy sees them)"""
    import ctypes
    v = [0.0] * 64
    for base, key in ((0, 'outlines'), (16, 'rotations'), (32, 'translations'), (48, 'stitch_tags')):
        if key == 'stitch_tags' and not explicit_stitch_tags:
            continue
        sh = [float(x) for x in data_stats['gt_shift'][key]]
        sc = [float(x) for x in data_stats['gt_scale'][key]]
        if len(sh) != widths[key] or len(sc) != widths[key]:
            raise ValueError('pattern_decode: %d statistics for %r of width %d' % (len(sh), key, widths[key]))
        v[base:base + len(sh)], v[base + 8:base + 8 + len(sc)] = sh, sc
    return (ctypes.c_double * 64)(*v)


def _edge_views(stitch_tags, free_edges_mask, name):
    """checks of the tag / logit views shared by pattern_decode and tags_to_stitches -> (B, P, L, D)"""
    _dev_check(stitch_tags)
    _dev_check(free_edges_mask)
    if stitch_tags.dim() != 4 or free_edges_mask.shape != stitch_tags.shape[:3]:
        raise ValueError('%s: stitch_tags [B,P,L,D] and free_edges_mask [B,P,L] expected (got %s, %s)'
                         % (name, tuple(stitch_tags.shape), tuple(free_edges_mask.shape)))
    B, P, Lp, D = stitch_tags.shape
    if not (1 <= P * Lp <= PATTERN_MAX_EDGES) or not (1 <= D <= PATTERN_MAX_WIDTH) or B < 1:
        raise ValueError('%s: 1 <= P * L <= %d edge slots and a tag width of 1 .. %d are supported (got P = %d, L = %d, D = %d)'
                         % (name, PATTERN_MAX_EDGES, PATTERN_MAX_WIDTH, P, Lp, D))
    return B, P, Lp, D


def tags_to_stitches(stitch_tags, free_edges_mask):
    """Garment3DPatternFullDataset.tags_to_stitches (nn/data/datasets.py:917-968) for a batch, one launch, no host read:
    stitch_tags [B,P,L,D] and the free-edge logits [B,P,L] (strided views are fine) -> (stitches int32 [B,2,S] of pattern-level
    edge ids in the order the reference appends them, zero tails; num_stitches int32 [B]) with S = P * L // 2."""
    B, P, Lp, D = _edge_views(stitch_tags, free_edges_mask, 'tags_to_stitches')
    tags, lg = stitch_tags.detach(), free_edges_mask.detach()
    dev = tags.device
    S = P * Lp // 2
    stitches = torch.empty(B, 2, S, device=dev, dtype=torch.int32)
    nums = torch.empty(B, device=dev, dtype=torch.int32)
    L.call('gpe_tags_to_stitches', tags, *_view_strides(tags), D, lg, lg.stride(0), lg.stride(1), lg.stride(2), B, P, Lp,
           stitches if S else None, nums)
    return stitches, nums


def pattern_decode(preds, data_stats, explicit_stitch_tags=False, stitches=None, num_stitches=None):
    """Garment3DPatternFullDataset._pred_to_pattern (nn/data/datasets.py:731-767) up to the pattern's numbers, for a batch, one launch,
    no host read: un-standardise in fp64, drop padding rows and empty panels, walk the edge loops to vertices, pair the stitch tags
    (or take `stitches` [B,2,S'] with optional `num_stitches` [B], any integer dtype, instead) and check every stitch against the
    panels it names.  `preds` is a model's output dict (strided views are fine), `data_stats` is data_config['standardize'].
    -> dict of device tensors, PATTERN_DECODE_KEYS (layouts: include/gpe_hip.h gpe_pattern_decode)."""
    ol, rot, tr = preds['outlines'].detach(), preds['rotations'].detach(), preds['translations'].detach()
    for t in (ol, rot, tr):
        _dev_check(t)
    if ol.dim() != 4 or ol.shape[3] != 4:
        raise ValueError('pattern_decode: outlines [B,P,L,4] expected (got %s)' % (tuple(ol.shape),))
    B, P, Lp = ol.shape[:3]
    R, T = rot.shape[-1], tr.shape[-1]
    if not (1 <= P * Lp <= PATTERN_MAX_EDGES) or not (1 <= R <= PATTERN_MAX_WIDTH) or not (1 <= T <= PATTERN_MAX_WIDTH) or B < 1:
        raise ValueError('pattern_decode: 1 <= P * L <= %d edge slots and rotation / translation widths of 1 .. %d are supported '
                         '(got P = %d, L = %d, R = %d, T = %d)' % (PATTERN_MAX_EDGES, PATTERN_MAX_WIDTH, P, Lp, R, T))
    dev = ol.device
    widths = {'outlines': 4, 'rotations': R, 'translations': T}
    if stitches is None:
        tags, lg = preds['stitch_tags'].detach(), preds['free_edges_mask'].detach()
        if _edge_views(tags, lg, 'pattern_decode')[:3] != (B, P, Lp):
            raise ValueError('pattern_decode: stitch_tags %s do not match outlines %s' % (tuple(tags.shape), tuple(ol.shape)))
        widths['stitch_tags'] = tags.shape[3]
        t_args = (tags, *_view_strides(tags), tags.shape[3], lg, lg.stride(0), lg.stride(1), lg.stride(2), None, None)
        S = P * Lp // 2
    else:
        if not stitches.is_cuda:
            raise RuntimeError('gpe ops need tensors on the MI355X (got %s stitches); there is no CPU path' % stitches.device)
        if stitches.dim() != 3 or stitches.shape[0] != B or stitches.shape[1] != 2 or stitches.shape[2] < 1 or \
                stitches.dtype.is_floating_point:
            raise ValueError('pattern_decode: stitches of integer dtype [B,2,S >= 1] expected (got %s %s)'
                             % (stitches.dtype, tuple(stitches.shape)))
        S = stitches.shape[2]
        given = stitches.to(torch.int32).contiguous()
        nums = num_stitches.to(dev).reshape(B).to(torch.int32).contiguous() if num_stitches is not None else None
        explicit_stitch_tags = False
        t_args = (None, 0, 0, 0, 0, None, 0, 0, 0, given, nums)
    stats = _pattern_decode_stats(data_stats, widths, explicit_stitch_tags)
    i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)                       # noqa: E731
    f64 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)                     # noqa: E731
    o = {'num_edges': i32(B, P), 'edge_slot': i32(B, P, Lp), 'num_verts': i32(B, P), 'closed': i32(B, P), 'new_panel_id': i32(B, P),
         'num_panels': i32(B), 'vertices': f64(B, P, Lp + 1, 2), 'curvature': f64(B, P, Lp, 2), 'rotations': f64(B, P, R),
         'translations': f64(B, P, T), 'curved': i32(B, P, Lp), 'stitches': i32(B, 2, S), 'num_stitches': i32(B),
         'stitch_flags': i32(B, S), 'first_invalid': i32(B)}
    L.call('gpe_pattern_decode', ol, *_view_strides(ol), rot, _row_stride(rot, P), R, tr, _row_stride(tr, P), T, *t_args,
           B, P, Lp, S, 1 if explicit_stitch_tags else 0, stats,
           *[o[k] if o[k].numel() else None for k in PATTERN_DECODE_KEYS])
    return o


# the panels of a decoded prediction placed in 3D (csrc/gpe_pattern_place.hip)
PATTERN_PLACE_KEYS = ('rot_matrix', 'translation', 'top_mid', 'vertices3d', 'edges3d', 'place_flags')
PATTERN_PLACE_INPUTS = ('num_edges', 'num_verts', 'vertices', 'curvature', 'curved', 'rotations', 'translations')
PLACE_BAD_QUAT = 1                                      # include/gpe_hip_place.h GPE_PLACE_BAD_QUAT


def pattern_place(decoded):
    """The step between the two prediction stages (NNSewingPattern._3D_edges_per_panel, nn/data/pattern_converter.py:517-552, and the
    inverse of the universal translation, :281-288) for a batch, one launch, no host read: `decoded` is pattern_decode's dict (or
    anything with its PATTERN_PLACE_INPUTS).  Per non-empty panel, in fp64: the rotation matrix of the normalised quaternion, the
    bounding-box side midpoint that lies highest in 3D (`top_mid`), the translation of the panel's origin, the vertices in 3D, and
    the compact fp32 edge rows `edges3d` [B,P,L,8] that stitch_pairs takes with `num_edges`.
    -> dict of device tensors, PATTERN_PLACE_KEYS (layouts: include/gpe_hip_place.h gpe_pattern_place)."""
    t = {k: decoded[k] for k in PATTERN_PLACE_INPUTS}
    for v in t.values():
        if not v.is_cuda:
            raise RuntimeError('gpe ops need tensors on the MI355X (got a %s tensor); there is no CPU path' % v.device)
    if t['curved'].dim() != 3:
        raise ValueError('pattern_place: curved [B,P,L] expected (got %s)' % (tuple(t['curved'].shape),))
    B, P, Lp = t['curved'].shape
    if t['rotations'].shape[-1] != 4 or t['translations'].shape[-1] != 3:
        raise ValueError('pattern_place: quaternions (rotation width 4) and 3D translations (width 3) are placed (got widths %d, %d)'
                         % (t['rotations'].shape[-1], t['translations'].shape[-1]))
    if not (1 <= P * Lp <= PATTERN_MAX_EDGES) or B < 1:
        raise ValueError('pattern_place: 1 <= P * L <= %d edge slots are supported (got P = %d, L = %d)' % (PATTERN_MAX_EDGES, P, Lp))
    shapes = {'num_edges': (B, P), 'num_verts': (B, P), 'vertices': (B, P, Lp + 1, 2), 'curvature': (B, P, Lp, 2),
              'curved': (B, P, Lp), 'rotations': (B, P, 4), 'translations': (B, P, 3)}
    for k, shape in shapes.items():
        want = torch.int32 if k in ('num_edges', 'num_verts', 'curved') else F64
        if tuple(t[k].shape) != shape or t[k].dtype != want:
            raise ValueError('pattern_place: %s of %s %s expected (got %s %s)' % (k, want, shape, t[k].dtype, tuple(t[k].shape)))
        t[k] = t[k].detach().contiguous()
    dev = t['curved'].device
    o = {'rot_matrix': torch.empty(B, P, 3, 3, device=dev, dtype=F64), 'translation': torch.empty(B, P, 3, device=dev, dtype=F64),
         'top_mid': torch.empty(B, P, device=dev, dtype=torch.int32),
         'vertices3d': torch.empty(B, P, Lp + 1, 3, device=dev, dtype=F64),
         'edges3d': torch.empty(B, P, Lp, 8, device=dev, dtype=F32), 'place_flags': torch.empty(B, P, device=dev, dtype=torch.int32)}
    L.call('gpe_pattern_place', *[t[k] for k in PATTERN_PLACE_INPUTS], B, P, Lp, *[o[k] for k in PATTERN_PLACE_KEYS])
    return o


# the edge-pair classifier scored on predicted patterns over a whole set (csrc/gpe_framework_eval.hip)
FRAMEWORK_EVAL_KEYS = ('full_loss', 'edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall',
                       'selected_precision', 'selected_recall')              # include/gpe_hip_framework.h, in the kernel's order
FRAMEWORK_SKIP_REASONS = ('bad_rotation', 'no_stitches', 'no_pairs', 'wrong_panel_count')       # states 1, 2, 3; counted but not corr
FRAMEWORK_SETS = ('stitch', 'stitch_corr')
FRAMEWORK_RECORD = ('state', 'corr', 'loss_sum') + STITCH_EVAL_COUNTS + ('num_selected',)
FRAMEWORK_TOTALS = STITCH_EVAL_COUNTS + ('num_selected', 'garments')
FRAMEWORK_MAX_PANELS = 64


class FrameworkAccumulator:
    """Step 3 of the reference's on_test_set.py -st ... -corr kept on the device: which garments of a batch count
    (GarmentStitchPairsDataset._clean_datapoint_list, nn/data/datasets.py:1134-1159), their per-garment values folded as
    _eval_metrics_per_loader folds batches of one garment (nn/metrics/eval_utils.py:35-76), for all counted garments ('stitch') and
    for those with the right number of panels ('stitch_corr').  One launch per batch (include/gpe_hip_framework.h
    gpe_framework_eval_add), ONE host read at the end.  It mirrors EvalAccumulator:

        acc = FrameworkAccumulator(slots=len(folders), total=garments, device='cuda')
        for ...: acc.add(stitch_pairs_eval's dict, DecodedPatterns after place(), gt_num_panels)
        totals, loss, ratios = acc.pool(groups, n_groups)        # device tensors, batch-independent
        rows = acc.read()                                        # [{'stitch': {...}, 'stitch_corr': {...}, 'skipped': {...}}] per slot

    `.table` fp64 [total, 10] keeps one record per garment in visiting order (FRAMEWORK_RECORD); `.rows` counts the garments seen."""

    def __init__(self, slots=1, total=1, device='cuda'):
        if isinstance(slots, bool) or not isinstance(slots, int) or slots < 1:
            raise ValueError('FrameworkAccumulator: slots must be a positive integer (got %r)' % (slots,))
        if isinstance(total, bool) or not isinstance(total, int) or not 1 <= total <= 0x7fffffff:
            raise ValueError('FrameworkAccumulator: total must be the number of garments of the pass, 1 .. 2^31 - 1 (got %r)' % (total,))
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('gpe ops need tensors on the MI355X (got device %s); there is no CPU path' % self.device)
        K = len(FRAMEWORK_EVAL_KEYS)
        self.slots, self.total, self.rows = slots, total, 0
        # one allocation, one read: sum [2, slots, K] as its fp32 bits | cnt [2, slots] | skipped [slots, 4] | status [1]
        self.state = torch.zeros(2 * slots * K + 2 * slots + 4 * slots + 1, device=self.device, dtype=torch.int32)
        self.device = self.state.device                        # with its index: what the batches' tensors are compared with
        a, b = 2 * slots * K, 2 * slots * K + 2 * slots
        self.sum = self.state[:a].view(F32).view(2, slots, K)
        self.cnt = self.state[a:b].view(2, slots)
        self.skipped = self.state[b:b + 4 * slots].view(slots, 4)
        self.status = self.state[-1:]
        self.table = torch.zeros(total, len(FRAMEWORK_RECORD), device=self.device, dtype=F64)
        self.slot = torch.zeros(1, device=self.device, dtype=torch.int32)
        self._slot_host = torch.arange(slots, dtype=torch.int32).pin_memory()      # sources of set_slot's queued one-word copies

    def reset(self):
        """sums, counters, the table and the status back to zero, the slot word to row 0 (queued; no device read)"""
        self.state.zero_()
        self.table.zero_()
        self.slot.zero_()
        self.rows = 0

    def set_slot(self, i):
        """the following add() calls go to row i: a queued copy from pinned memory, no device read"""
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < self.slots:
            raise ValueError('FrameworkAccumulator.set_slot: row 0 .. %d (got %r)' % (self.slots - 1, i))
        self.slot.copy_(self._slot_host[i:i + 1], non_blocking=True)

    def add(self, eval_out, decoded, gt_num_panels, records=None):
        """one batch: eval_out is stitch_pairs_eval's dict ('counts', 'loss_sum', 'num_stitches'), decoded the placed DecodedPatterns
        (or a dict with 'num_stitches', 'first_invalid', 'num_panels', 'num_edges', 'place_flags'), gt_num_panels integer [B].
        records: the fp64 [B, 10] rows to write instead of the next B rows of `.table` (a captured add() writes static rows)."""
        get = (lambda k: getattr(decoded, k)) if not isinstance(decoded, dict) else decoded.__getitem__
        try:
            counts, loss_sum, n_sel = eval_out['counts'], eval_out['loss_sum'], eval_out['num_stitches']
            dec = {k: get(k) for k in ('num_stitches', 'first_invalid', 'num_panels', 'num_edges', 'place_flags')}
        except (KeyError, AttributeError) as e:
            raise ValueError('FrameworkAccumulator.add: %s is missing (eval_out: ops.stitch_pairs_eval\'s dict; decoded: a placed '
                             'DecodedPatterns)' % e)
        if not torch.is_tensor(counts) or counts.dim() != 2 or counts.shape[1] != 6 or counts.dtype != torch.int32:
            raise ValueError('FrameworkAccumulator.add: counts must be int32 [B, 6] (got %s %s)'
                             % (getattr(counts, 'dtype', type(counts).__name__), tuple(getattr(counts, 'shape', ()))))
        B = counts.shape[0]
        ne = dec['num_edges']
        if B < 1 or ne.dim() != 2 or ne.shape[0] != B or not 1 <= ne.shape[1] <= FRAMEWORK_MAX_PANELS:
            raise ValueError('FrameworkAccumulator.add: num_edges [B = %d, 1 <= P <= %d] expected (got %s)'
                             % (B, FRAMEWORK_MAX_PANELS, tuple(ne.shape)))
        P = ne.shape[1]
        if not torch.is_tensor(loss_sum) or loss_sum.dtype != F64 or tuple(loss_sum.shape) != (B,):
            raise ValueError('FrameworkAccumulator.add: loss_sum must be fp64 [%d]' % B)
        if not torch.is_tensor(gt_num_panels) or gt_num_panels.is_floating_point() or gt_num_panels.dtype == torch.bool \
                or gt_num_panels.numel() != B:
            raise ValueError('FrameworkAccumulator.add: gt_num_panels must be an integer [%d] tensor' % B)
        shapes = {'num_selected': (B,), 'num_stitches': (B,), 'first_invalid': (B,), 'num_panels': (B,), 'num_edges': (B, P),
                  'place_flags': (B, P)}
        t = dict(dec, num_selected=n_sel)
        for k, shape in shapes.items():
            if not torch.is_tensor(t[k]) or t[k].dtype != torch.int32 or tuple(t[k].shape) != shape:
                raise ValueError('FrameworkAccumulator.add: %s must be int32 %s (got %s %s)'
                                 % (k, shape, getattr(t[k], 'dtype', type(t[k]).__name__), tuple(getattr(t[k], 'shape', ()))))
        own = records is None
        if own:
            if self.rows + B > self.total:
                raise ValueError('FrameworkAccumulator.add: more garments than the %d that total announced' % self.total)
            records = self.table[self.rows:self.rows + B]
        elif (not torch.is_tensor(records) or records.dtype != F64 or tuple(records.shape) != (B, len(FRAMEWORK_RECORD))
              or not records.is_contiguous()):
            raise ValueError('FrameworkAccumulator.add: records must be a contiguous fp64 [%d, %d] tensor' % (B, len(FRAMEWORK_RECORD)))
        for v in [counts, loss_sum, gt_num_panels, records] + list(t.values()):
            if v.device != self.device:
                if not v.is_cuda:
                    raise RuntimeError('gpe ops need tensors on the MI355X (got a %s tensor); there is no CPU path' % v.device)
                raise ValueError('FrameworkAccumulator.add: a tensor lives on %s, the accumulator on %s' % (v.device, self.device))
        gtp = gt_num_panels.detach().reshape(B).to(torch.int32).contiguous()
        L.call('gpe_framework_eval_add', counts.contiguous(), loss_sum.contiguous(), t['num_selected'].contiguous(),
               t['num_stitches'].contiguous(), t['first_invalid'].contiguous(), t['num_panels'].contiguous(), gtp,
               t['num_edges'].contiguous(), t['place_flags'].contiguous(), B, P, self.sum, self.cnt, self.skipped, records, self.slot,
               self.slots, self.status)
        if own:
            self.rows += B

    def pool(self, groups=None, n_groups=0, table=None):
        """the records of the garments seen so far (or `table`, fp64 [G, 10]) folded per group and overall, independent of the
        batching: -> (totals int64 [n_groups + 1, 2, 8] FRAMEWORK_TOTALS, loss fp64 [n_groups + 1, 2], ratios fp32
        [n_groups + 1, 2, 6] STITCH_EVAL_METRICS) on the device; axis 1 is FRAMEWORK_SETS.  groups: int32 [G] on the device (an id
        outside 0 .. n_groups-1 belongs to no group), or None with n_groups = 0.  One launch, no host read."""
        if table is None:
            if self.rows < 1:
                raise ValueError('FrameworkAccumulator.pool: no garment has been added')
            table = self.table[:self.rows]
        elif (not torch.is_tensor(table) or table.dtype != F64 or table.dim() != 2 or table.shape[1] != len(FRAMEWORK_RECORD)
              or table.shape[0] < 1 or not table.is_contiguous()):
            raise ValueError('FrameworkAccumulator.pool: table must be a contiguous fp64 [G, %d] tensor' % len(FRAMEWORK_RECORD))
        G = table.shape[0]
        if isinstance(n_groups, bool) or not isinstance(n_groups, int) or not 0 <= n_groups <= 65535:
            raise ValueError('FrameworkAccumulator.pool: n_groups must be an integer in 0 .. 65535 (got %r)' % (n_groups,))
        if groups is None:
            if n_groups:
                raise ValueError('FrameworkAccumulator.pool: %d groups need a group id per garment' % n_groups)
        elif (not torch.is_tensor(groups) or groups.dtype != torch.int32 or tuple(groups.shape) != (G,)
              or groups.device != table.device or not groups.is_contiguous()):
            raise ValueError('FrameworkAccumulator.pool: groups must be a contiguous int32 [%d] tensor on the device of the table' % G)
        if not table.is_cuda:
            raise RuntimeError('gpe ops need tensors on the MI355X (got a %s table); there is no CPU path' % table.device)
        dev = table.device
        totals = torch.empty(n_groups + 1, 2, len(FRAMEWORK_TOTALS), device=dev, dtype=torch.int64)
        loss = torch.empty(n_groups + 1, 2, device=dev, dtype=F64)
        ratios = torch.empty(n_groups + 1, 2, len(STITCH_EVAL_METRICS), device=dev, dtype=F32)
        L.call('gpe_framework_eval_pool', table, groups, G, n_groups, totals, loss, ratios)
        return totals, loss, ratios

    def read(self, along=()):
        """THE host read -> one dict per row: {'stitch': {key: value}, 'stitch_corr': {key: value}, 'skipped': {reason: int}} with
        value = np.float32(sum) / np.float32(cnt), None where no garment of the set was counted (the reference's None for an empty
        list).  `.last_sums` [2, slots, 7] / `.last_counts` [2, slots] / `.last_skipped` [slots, 4] keep what was read.  along:
        further device tensors of fp32 / int32 / fp64 / int64 to bring over in the same transfer; `.last_along` holds them as numpy
        arrays of their own dtype and shape, in order."""
        kinds = {F32: np.float32, torch.int32: np.int32, F64: np.float64, torch.int64: np.int64}
        along = [t.detach() for t in along]
        if any(t.dtype not in kinds or t.device != self.state.device for t in along):
            raise ValueError('FrameworkAccumulator.read: along takes fp32 / int32 / fp64 / int64 tensors on the accumulator\'s device')
        parts = [self.state] + [t.contiguous().view(torch.int32).reshape(-1) for t in along]
        host = (torch.cat(parts) if along else self.state).cpu().numpy()
        edges = np.cumsum([p.numel() for p in parts])
        self.last_along = [host[a:b].view(kinds[t.dtype]).reshape(tuple(t.shape)) for a, b, t in zip(edges[:-1], edges[1:], along)]
        return self.parse(host[:edges[0]])

    def parse(self, host):
        """read()'s result from `.state` as it arrived on the host (int32 numpy): for a caller that brought the state over in a
        transfer of its own (evaluation.FrameworkEvaluator reads it along with the first stage's accumulator)"""
        K, S = len(FRAMEWORK_EVAL_KEYS), self.slots
        host = np.ascontiguousarray(host, dtype=np.int32).reshape(-1)
        if host.size != self.state.numel():
            raise ValueError('FrameworkAccumulator.parse: %d words expected (got %d)' % (self.state.numel(), host.size))
        if host[-1]:
            raise RuntimeError('FrameworkAccumulator: an add() met a slot word outside 0 .. %d and was dropped' % (S - 1))
        a, b = 2 * S * K, 2 * S * K + 2 * S
        sums, cnts, skipped = host[:a].view(np.float32).reshape(2, S, K), host[a:b].reshape(2, S), host[b:b + 4 * S].reshape(S, 4)
        self.last_sums, self.last_counts, self.last_skipped = sums, cnts, skipped
        rows = []
        for s in range(S):
            row = {name: {k: (np.float32(sums[i, s, j]) / np.float32(cnts[i, s]) if cnts[i, s] else None)
                          for j, k in enumerate(FRAMEWORK_EVAL_KEYS)} for i, name in enumerate(FRAMEWORK_SETS)}
            row['skipped'] = {r: int(skipped[s, j]) for j, r in enumerate(FRAMEWORK_SKIP_REASONS)}
            rows.append(row)
        return rows

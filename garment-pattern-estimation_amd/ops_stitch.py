"""The edge-pair stitch classifier around its kernels: stitch recovery over all pairs (stitch_pairs, stitch_pairs_eval), the pair
loss of its training step (pair_class_loss) and the sampler of its training rows (stitch_pairs_sample).  Reached as ops.X: ops.py
re-exports every name of __all__.

The one leaf that calls the hot path (the dense Linear and BatchNorm glue of ops.py), hence the import from .ops below; that is
safe because the package imports ops first (see the re-export at the end of ops.py).  Reads no switch of ops.py.
_stitch_ldw lives in _opbase (the edge predictor in ops.py uses it too), _int32 / _int_tensor as well (the mesh sampler shares them)."""
import torch

from . import _lib as L
from ._opbase import F32, _dev_check, _int32, _int_tensor, _rows2d, _stitch_ldw, _ticket, round_up
from .ops import bn_from_running, dense_mlp, fold_bias, linear_raw, pack_weight

__all__ = ['STITCH_PAIRS_MAX_PANELS', 'STITCH_PAIRS_MAX_EDGES', 'STITCH_PAIRS_ROUTES', 'stitch_pairs_on_menu',
           'STITCH_EVAL_METRICS', 'STITCH_EVAL_COUNTS', 'stitch_pairs', 'stitch_pairs_eval', 'PAIR_LOSS_METRICS',
           'PAIR_LOSS_COUNTS', 'PAIR_LOSS_SLOTS', 'PairClassLossFn', 'pair_class_loss', 'STITCH_SAMPLE_MAX_EDGES',
           'STITCH_SAMPLE_MAX_ROWS', 'stitch_sample_resident', 'stitch_sample_state', 'stitch_pairs_sample']


# -------------------------------------------------------------------------------------------------
# stitch recovery from the edge-pair classifier (forward only)
# -------------------------------------------------------------------------------------------------
STITCH_PAIRS_MAX_PANELS, STITCH_PAIRS_MAX_EDGES = 32, 16
STITCH_PAIRS_ROUTES = ('auto', 'fused', 'rows')
_STITCH_ROWS_BUDGET = 1 << 19              # pair rows the generic route materialises per dense-MLP call


def stitch_pairs_on_menu(mlp):
    """can csrc/gpe_stitch_pairs.hip's fused kernel run this MLP?  (1 - 4 equally wide Linear layers in front of the output Linear,
    width <= 256 and a multiple of 4, an even number <= 32 of input features)"""
    blocks = [mlp[i] for i in range(len(mlp))]
    n = len(blocks) - 1
    if not 1 <= n <= 4 or blocks[-1][0].weight.shape[0] != 1:
        return False
    H, K0 = blocks[0][0].weight.shape
    if H > 256 or H % 4 or K0 % 2 or K0 > 32:
        return False
    return all(tuple(b[0].weight.shape) == (H, H) for b in blocks[1:-1]) and blocks[-1][0].weight.shape[1] == H


def _stitch_row_off(e, Lm, E):
    q, r = divmod(e, Lm)
    return Lm * q * E - Lm * Lm * (q * (q + 1) // 2) + r * (E - (q + 1) * Lm)


_STITCH_STAT_CONSTS = {}     # (device, shift, scale) -> (1 / scale, - shift / scale) on the device, read-only


def _stitch_stat_consts(shift, scale, dev):
    """the two vectors that fold the pair rows' standardisation into the first Linear.  They come from host numbers, and a copy from
    the host cannot be captured: a call with statistics seen before (a warm-up call, as for every lazily built state) reuses the
    tensors of the first, so that stitch_pairs is legal inside a stream capture (model.predict_garment)."""
    key = (dev, tuple(shift), tuple(scale))
    hit = _STITCH_STAT_CONSTS.get(key)
    if hit is None:
        hit = (torch.tensor([1.0 / s for s in scale], device=dev, dtype=F32),
               torch.tensor([-sh / sc for sh, sc in zip(shift, scale)], device=dev, dtype=F32))
        if len(_STITCH_STAT_CONSTS) < 16:       # a kept pair is never dropped (another stream may still read it); past 16 sets: as before
            _STITCH_STAT_CONSTS[key] = hit
    return hit


def _stitch_fused(edges, ne, blocks, shift, scale, table, dense, ev=None):
    """the store-free route: per-edge projections [A | Bv] of the first Linear (standardisation folded in), then one launch that
    classifies every pair from them (ev: the workspaces of an evaluating pass, _stitch_eval_ws)"""
    B, P, Lm, Fe = edges.shape
    dev = edges.device
    n = len(blocks) - 1
    H = blocks[0][0].weight.shape[0]
    W1, b1 = blocks[0][0].weight, blocks[0][0].bias
    inv, off = _stitch_stat_consts(shift, scale, dev)
    ab = torch.empty(B * P * Lm, 2 * H, device=dev, dtype=F32)
    rows = _rows2d(edges.view(-1, Fe))
    linear_raw(rows, pack_weight(W1[:, :Fe], col_scale=inv[:Fe]), fold_bias(W1, b1, off), B * P * Lm, H, Fe, (ab, 2 * H, 0, 0))
    linear_raw(rows, pack_weight(W1[:, Fe:], col_scale=inv[Fe:]), None, B * P * Lm, H, Fe, (ab[:, H:], 2 * H, 0, 0))
    ldw = _stitch_ldw(H)
    wpk = torch.zeros((n - 1) * (H + 1) * ldw + H + 4, device=dev, dtype=F32)
    # f16x3: two-term fp16 planes of the hidden layers' folded weights, one power of two per layer (its amax word)
    h3 = L.get_math() == 'f16x3' and H <= 224 and n > 1
    KP = round_up(H, 32)
    planes = torch.empty((n - 1) * KP * ldw, device=dev, dtype=F32) if h3 else None
    words = torch.empty(n - 1, device=dev, dtype=torch.int32) if h3 else None
    st = None
    for l, blk in enumerate(blocks):
        bn = blk[2]
        if l > 0:
            W, b = blk[0].weight, blk[0].bias
            if l < n:
                o = (l - 1) * (H + 1) * ldw
                L.call('gpe_stitch_pairs_pack', W, W.stride(0), H, H, st[2], wpk[o:], ldw)
                L.call('gpe_fold_bias', W, W.stride(0), H, H, b, st[3], wpk[o + H * ldw:])
                if h3:
                    L.call('gpe_absmax', wpk[o:], ldw, H, ldw, words[l - 1:])
                    L.call('gpe_stitch_pairs_planes', wpk[o:], H, ldw, words[l - 1:], planes[(l - 1) * KP * ldw:])
            else:
                o = (n - 1) * (H + 1) * ldw
                L.call('gpe_stitch_pairs_pack', W, W.stride(0), 1, H, st[2], wpk[o:], 1)
                L.call('gpe_fold_bias', W, W.stride(0), 1, H, b, st[3], wpk[o + H:])
        st = bn_from_running(bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps)
    args = (ab, 2 * H, H, n, wpk, planes, words, st, ne, B, P, Lm, table, dense)
    if ev is None:
        L.call('gpe_stitch_pairs_fwd', *args)
    else:
        n8 = (P * Lm + 7) // 8                  # a slot per 8 x 8 tile position (include/gpe_hip.h)
        ev['slots'], ev['group'] = n8 * n8, n8
        ev['slab'] = torch.zeros(B, n8 * n8, device=dev, dtype=torch.float64)
        L.call('gpe_stitch_pairs_eval_fwd', *args, ev['mask'], ev['slab'], ev['counters'])


def _stitch_rows(edges, ne, mlp, shift, scale, table, dense, ev=None):
    """the generic route: materialised pair rows of a chunk of i-edges -> the dense-MLP kernels (eval) -> the same epilogue"""
    import ctypes
    B, P, Lm, Fe = edges.shape
    E = P * Lm
    sh = (ctypes.c_float * (2 * Fe))(*[float(v) for v in shift])
    sc = (ctypes.c_float * (2 * Fe))(*[float(v) for v in scale])
    last = (P - 1) * Lm                         # the edges of the last panel slot have no later partner
    if ev is not None:
        ev['slots'], ev['group'] = E, Lm        # a slot per i-edge, shared by the chunks
        ev['slab'] = torch.zeros(B, E, device=edges.device, dtype=torch.float64)
    c0 = 0
    while c0 < last:
        c1 = c0 + 1
        while (c1 < last and B * (c1 + 1 - c0) <= 65535
               and B * (_stitch_row_off(c1 + 1, Lm, E) - _stitch_row_off(c0, Lm, E)) <= _STITCH_ROWS_BUDGET):
            c1 += 1
        nrows = _stitch_row_off(c1, Lm, E) - _stitch_row_off(c0, Lm, E)
        rows = torch.empty(B * nrows, 2 * Fe, device=edges.device, dtype=F32)
        L.call('gpe_stitch_pairs_rows', edges, ne, B, P, Lm, Fe, sh, sc, c0, c1, nrows, rows)
        y = dense_mlp(rows, mlp, False)
        if ev is None:
            L.call('gpe_stitch_pairs_reduce', y, y.stride(0), ne, B, P, Lm, c0, c1, nrows, table, dense)
        else:
            L.call('gpe_stitch_pairs_eval_reduce', y, y.stride(0), ne, B, P, Lm, c0, c1, nrows, table, dense, ev['mask'], ev['slab'],
                   ev['counters'])
        c0 = c1


def _stitch_check(edges3d, num_edges, mlp, f_shift, f_scale, route, gt=None):
    """the argument checks of stitch_pairs / stitch_pairs_eval, all before any device check -> (blocks, fused)"""
    if route not in STITCH_PAIRS_ROUTES:
        raise ValueError('unknown route %r (choose from %s)' % (route, STITCH_PAIRS_ROUTES))
    if edges3d.dim() != 4:
        raise ValueError('edges3d must be [B, P, L, Fe] (got %s)' % (tuple(edges3d.shape),))
    B, P, Lm, Fe = edges3d.shape
    if P > STITCH_PAIRS_MAX_PANELS or Lm > STITCH_PAIRS_MAX_EDGES or P * Lm < 2 or B < 1:
        raise ValueError('stitch_pairs handles 1 .. %d panels of 1 .. %d edges (got P = %d, L = %d)'
                         % (STITCH_PAIRS_MAX_PANELS, STITCH_PAIRS_MAX_EDGES, P, Lm))
    blocks = [mlp[i] for i in range(len(mlp))]
    if blocks[0][0].weight.shape[1] != 2 * Fe or len(f_shift) != 2 * Fe or len(f_scale) != 2 * Fe or Fe > 16:
        raise ValueError('the classifier takes %d features per pair, the statistics have %d / %d, the edges %d each (<= 16)'
                         % (blocks[0][0].weight.shape[1], len(f_shift), len(f_scale), Fe))
    if mlp.training:
        raise RuntimeError('stitch_pairs is a prediction path: call .eval() on the model first (BatchNorm running statistics)')
    if tuple(num_edges.shape) != (B, P) or num_edges.is_floating_point() or num_edges.device != edges3d.device:
        raise ValueError('num_edges must be an integer [B, P] tensor on the device of edges3d')
    if gt is not None:
        st, nums = gt
        if (not torch.is_tensor(st) or st.dim() != 3 or tuple(st.shape[:2]) != (B, 2) or st.is_floating_point() or st.is_complex()
                or st.dtype == torch.bool or st.device != edges3d.device):
            raise ValueError('gt_stitches must be an integer [B, 2, S] tensor of edge ids panel * L + edge on the device of edges3d')
        if (not torch.is_tensor(nums) or tuple(nums.shape) != (B,) or nums.is_floating_point() or nums.is_complex()
                or nums.dtype == torch.bool or nums.device != edges3d.device):
            raise ValueError('gt_num_stitches must be an integer [B] tensor on the device of edges3d')
    on_menu = stitch_pairs_on_menu(mlp)
    if route == 'fused' and not on_menu:
        raise ValueError("route='fused' needs 1 - 4 hidden layers of one width <= 256 that is a multiple of 4; use 'auto' or 'rows'")
    return blocks, on_menu and route != 'rows'


STITCH_EVAL_METRICS = ('edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall', 'selected_precision',
                       'selected_recall')
STITCH_EVAL_COUNTS = ('pairs', 'correct', 'true_positives', 'predicted_positives', 'gt_positives', 'selected_tp')


def _stitch_eval_ws(gt_stitches, gt_num_stitches, B, P, Lm, dev):
    """the caller-owned, zeroed workspaces of an evaluating pass (sizes: include/gpe_hip.h) with the label mask filled in"""
    E, S = P * Lm, gt_stitches.shape[2]
    ev = {'mask': torch.zeros(B, E, (E + 31) // 32, device=dev, dtype=torch.int32),
          'counters': torch.zeros(B, 2, device=dev, dtype=torch.int64)}
    # the kernel ignores ids outside 0 .. E - 1 and clamps the counts itself; wider integers are brought into int32's range first
    st, nums = _int32(gt_stitches, -1, E), _int32(gt_num_stitches, 0, S)
    L.call('gpe_stitch_pairs_labels', st if S else None, nums, B, P, Lm, S, ev['mask'])
    return ev


def _stitch_run(edges3d, num_edges, mlp, blocks, fused, f_shift, f_scale, return_logits, gt=None):
    """classify every pair, select; with gt = (gt_stitches, gt_num_stitches) through the evaluating entry points, then finalise"""
    B, P, Lm, Fe = edges3d.shape
    dev = edges3d.device
    E, S = P * Lm, P * Lm // 2
    shift, scale = [float(v) for v in f_shift], [float(v) for v in f_scale]
    with torch.no_grad():
        edges = edges3d.detach().contiguous()
        ne = num_edges.to(torch.int32).contiguous()
        table = torch.zeros(B, E, device=dev, dtype=torch.int64)
        dense = torch.full((B, E, E), float('nan'), device=dev, dtype=F32) if return_logits else None
        ev = _stitch_eval_ws(gt[0], gt[1], B, P, Lm, dev) if gt is not None else None
        if fused:
            _stitch_fused(edges, ne, blocks, shift, scale, table, dense, ev)
        else:
            _stitch_rows(edges, ne, mlp, shift, scale, table, dense, ev)
        stitches = torch.empty(B, 2, S, device=dev, dtype=torch.int32)
        nums = torch.empty(B, device=dev, dtype=torch.int32)
        scores = torch.empty(B, S, device=dev, dtype=F32)
        L.call('gpe_stitch_select', table, B, P, Lm, stitches, nums, scores)
        out = {'stitches': stitches, 'num_stitches': nums, 'scores': scores}
        if return_logits:
            out['logits'] = dense
        if ev is not None:
            loss_sum = torch.empty(B, device=dev, dtype=torch.float64)
            counts = torch.empty(B, 6, device=dev, dtype=torch.int32)
            metrics = torch.empty(6, device=dev, dtype=F32)
            L.call('gpe_stitch_eval_finalize', ev['slab'], ev['slots'], ev['group'], ev['counters'], ev['mask'], stitches, nums, B, P,
                   Lm, loss_sum, counts, metrics)
            out.update(metrics={k: metrics[i] for i, k in enumerate(STITCH_EVAL_METRICS)}, counts=counts, loss_sum=loss_sum)
    return out


def stitch_pairs(edges3d, num_edges, mlp, f_shift, f_scale, route='auto', return_logits=False):
    """Stitches of B garments from the edge-pair classifier `mlp` (net_blocks.MLP([2 Fe, H x n, 1]), eval mode): what the
    reference does at prediction time with NNSewingPattern.all_edge_pairs + stitches_from_pair_classifier
    (nn/data/pattern_converter.py:411-499) with the intended indexing of line 432.

    edges3d [B, P, L, Fe] fp32: un-standardised 3D edges per panel slot; num_edges [B, P] int (0 = panel absent); f_shift / f_scale:
    2 Fe numbers.  -> stitches int32 [B, 2, S] (edge ids panel * L + edge, side 0 = lower panel, ascending (i, j, r, c), zero-padded;
    S = P * L // 2), num_stitches int32 [B], scores fp32 [B, S] (logits) and, with return_logits, the dense logits [B, P*L, P*L]
    (NaN where there is no pair).  No host synchronisation.  route: 'fused' (csrc/gpe_stitch_pairs.hip's store-free kernel; ValueError
    off its menu), 'rows' (materialised rows through the dense-MLP kernels), 'auto' (fused on the menu, rows otherwise)."""
    blocks, fused = _stitch_check(edges3d, num_edges, mlp, f_shift, f_scale, route)
    _dev_check(edges3d)
    return _stitch_run(edges3d, num_edges, mlp, blocks, fused, f_shift, f_scale, return_logits)


def stitch_pairs_eval(edges3d, num_edges, mlp, f_shift, f_scale, gt_stitches, gt_num_stitches, route='auto', return_logits=False):
    """stitch_pairs scored against ground-truth stitches in the same classification pass: the reference's evaluation of this model
    (GarmentStitchPairsDataset with random_pairs_mode False: the labels of all_edge_pairs, nn/data/pattern_converter.py:458-499, into
    ComposedLoss, nn/metrics/composed_loss.py:83-126) without a pair row, a logit or a label stored, and without a host read.

    gt_stitches integer [B, 2, S] (S may be 0): edge ids panel * L + edge of both sides, either orientation, the layout of the stitch
    losses; gt_num_stitches integer [B], clamped to 0 .. S.  Entries with an id outside 0 .. P L - 1 are ignored, duplicates are
    harmless, and an entry that no enumerated pair matches (same panel, absent edge) counts nowhere.
    -> the dict of stitch_pairs plus 'metrics' {name: fp32 device scalar} pooled over the call (STITCH_EVAL_METRICS: the loss is the
    mean over the concatenated pairs; selected_* score the selected stitches; a ratio with denominator 0 is 0), 'counts' int32 [B, 6]
    (STITCH_EVAL_COUNTS) and 'loss_sum' fp64 [B] (the sum of the BCE-with-logits terms per garment).  Bit-reproducible."""
    blocks, fused = _stitch_check(edges3d, num_edges, mlp, f_shift, f_scale, route, (gt_stitches, gt_num_stitches))
    _dev_check(edges3d)
    return _stitch_run(edges3d, num_edges, mlp, blocks, fused, f_shift, f_scale, return_logits, (gt_stitches, gt_num_stitches))


PAIR_LOSS_METRICS = ('edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall')
PAIR_LOSS_COUNTS = ('pairs', 'correct', 'true_positives', 'predicted_positives', 'gt_positives')
PAIR_LOSS_SLOTS = 64          # partial sums of gpe_pair_loss_fwd: part of the result's bits, so a constant and not a device property


def _pair_labels(labels, M):
    """-> (flat labels as the kernel reads them, kind): bool as a uint8 view, uint8 and fp32 as they are, anything else cast once"""
    if labels.numel() != M:
        raise ValueError('pair_class_loss: %d labels for %d logits' % (labels.numel(), M))
    y = labels.reshape(-1)
    if y.dtype == torch.bool:
        return y.contiguous().view(torch.uint8), 0
    if y.dtype == torch.uint8:
        return y.contiguous(), 0
    return (y if y.dtype == F32 else y.to(F32)).contiguous(), 1


class PairClassLossFn(torch.autograd.Function):
    """ComposedLoss (nn/metrics/composed_loss.py:83-126) on the logits of a batch of pair rows: BCEWithLogitsLoss and the counters
    behind edge_pair_class_acc / stitch_precision / stitch_recall in one forward launch, the gradient in one backward launch, no
    host read.  Returns (out [4] fp32 in the order of PAIR_LOSS_METRICS, counts [5] int32 in the order of PAIR_LOSS_COUNTS); only
    out[0] carries gradient.  Nothing the backward reads is overwritten: a second backward over the same graph gives the same."""

    @staticmethod
    def forward(ctx, logits, labels):
        _dev_check(logits)
        if not labels.is_cuda:
            raise RuntimeError('gpe ops need tensors on the MI355X (got %s labels); there is no CPU path' % labels.device)
        dev = logits.device
        x = logits.reshape(-1).contiguous()
        M = x.numel()
        y, kind = _pair_labels(labels, M)
        part = torch.empty(PAIR_LOSS_SLOTS * 4, device=dev, dtype=torch.int64)
        out = torch.empty(4, device=dev, dtype=F32)
        counts = torch.empty(5, device=dev, dtype=torch.int32)
        L.call('gpe_pair_loss_fwd', x, y, kind, M, PAIR_LOSS_SLOTS, part, _ticket(dev), out, counts)
        ctx.rows = (x, y, kind, M)
        ctx.shape = logits.shape
        ctx.mark_non_differentiable(counts)
        return out, counts

    @staticmethod
    def backward(ctx, g, _g_counts):
        x, y, kind, M = ctx.rows
        gx = torch.empty(M, device=x.device, dtype=F32)
        # g[0] is the upstream gradient of the loss (a device scalar: no host sync); the ratios carry none
        L.call('gpe_pair_loss_bwd', x, y, kind, M, g.contiguous(), gx)
        return gx.view(ctx.shape), None


def pair_class_loss(logits, labels, return_counts=False):
    """-> out [4] = (edge_pair_class_loss, edge_pair_class_acc, stitch_precision, stitch_recall) of fp32 device logits against
    labels of the same number of elements (bool / uint8 / fp32 read in place, other types cast once on the device); a ratio with
    an empty denominator is 0.  return_counts: -> (out, counts [5] int32 = rows, correct, true positives, predicted positives,
    ground-truth positives)."""
    out, counts = PairClassLossFn.apply(logits, labels)
    return (out, counts) if return_counts else out


STITCH_SAMPLE_MAX_EDGES, STITCH_SAMPLE_MAX_ROWS = 512, 4096     # P * L and rows per garment of csrc/gpe_stitch_sample.hip


def stitch_sample_resident(edges3d, num_edges, gt_stitches, gt_num_stitches):
    """the resident set of stitch_pairs_sample, checked, with wider integer tensors brought into int32 once:
    edges3d [G, P, L, Fe] fp32, num_edges [G, P], gt_stitches [G, 2, S] (edge ids panel * L + edge), gt_num_stitches [G]"""
    if not torch.is_tensor(edges3d) or edges3d.dim() != 4:
        raise ValueError('edges3d must be [G, P, L, Fe] (got %s)' % (tuple(getattr(edges3d, 'shape', ())),))
    G, P, Lm, Fe = edges3d.shape
    if G < 1 or P < 1 or Lm < 1 or P * Lm > STITCH_SAMPLE_MAX_EDGES or not 1 <= Fe <= 16:
        raise ValueError('stitch_pairs_sample handles garments of 1 .. %d edge slots of 1 .. 16 features (got G = %d, P = %d, L = %d, '
                         'Fe = %d)' % (STITCH_SAMPLE_MAX_EDGES, G, P, Lm, Fe))
    dev = edges3d.device
    _int_tensor(num_edges, (G, P), 'num_edges', dev)
    if not torch.is_tensor(gt_stitches) or gt_stitches.dim() != 3:
        raise ValueError('gt_stitches must be an integer [G, 2, S] tensor of edge ids panel * L + edge on the device of edges3d')
    S = gt_stitches.shape[2]
    _int_tensor(gt_stitches, (G, 2, S), 'gt_stitches', dev)
    _int_tensor(gt_num_stitches, (G,), 'gt_num_stitches', dev)
    _dev_check(edges3d)
    return (edges3d.detach().contiguous(), _int32(num_edges, 0, Lm), _int32(gt_stitches, -1, P * Lm), _int32(gt_num_stitches, 0, S))


def stitch_sample_state(seed, draw, device):
    """{seed, draw} of stitch_pairs_sample as an int64 [2] device tensor (the bit patterns of two unsigned 64-bit numbers)"""
    signed = [v - (1 << 64) if v >= 1 << 63 else v for v in (int(seed) % (1 << 64), int(draw) % (1 << 64))]
    return torch.tensor(signed, dtype=torch.int64).to(device)


def stitch_pairs_sample(edges3d, num_edges, gt_stitches, gt_num_stitches, index, n_stitched, n_non_stitched, f_shift, f_scale,
                        state, ticket, shuffle_pairs=True, shuffle_pairs_order=True):
    """Training pair rows of B garments drawn on the device: what NNSewingPattern.stitches_as_3D_pairs(n_stitched, n_non_stitched,
    shuffle_pairs, shuffle_pairs_order) (nn/data/pattern_converter.py:321-409) followed by FeatureStandartization gives per garment,
    in one launch of csrc/gpe_stitch_sample.hip and with no host read (semantics and random numbers: include/gpe_hip.h).

    The resident set as stitch_sample_resident takes it; index integer [B]: the garment of every batch slot; f_shift / f_scale: 2 Fe
    numbers; state int64 [2] = {seed, draw} on the device (stitch_sample_state), advanced by the launch; ticket: one zeroed int32 of
    the caller's, left zero.  -> rows fp32 [B, R, 2 Fe] (R = n_stitched + n_non_stitched), labels bool [B, R] (a view of the bytes
    ops.pair_class_loss reads in place), status int32 [B] (>= 0 rows that gave up, -1 more valid stitches than n_stitched, -2 index
    outside 0 .. G - 1; such a slot is all zeros)."""
    edges, ne, gt, nums = stitch_sample_resident(edges3d, num_edges, gt_stitches, gt_num_stitches)
    G, P, Lm, Fe = edges.shape
    dev = edges.device
    n_stitched, n_non_stitched = int(n_stitched), int(n_non_stitched)
    R = n_stitched + n_non_stitched
    if n_stitched < 0 or n_non_stitched < 0 or not 1 <= R <= STITCH_SAMPLE_MAX_ROWS:
        raise ValueError('stitch_pairs_sample draws 1 .. %d rows per garment (got %d + %d)' % (STITCH_SAMPLE_MAX_ROWS, n_stitched, n_non_stitched))
    if len(f_shift) != 2 * Fe or len(f_scale) != 2 * Fe:
        raise ValueError('the statistics have %d / %d numbers, the pair rows %d features' % (len(f_shift), len(f_scale), 2 * Fe))
    if shuffle_pairs and Fe != 8:
        raise ValueError('shuffle_pairs reverses edges of the layout [start xyz | end xyz | cx cy]: Fe must be 8 (got %d)' % Fe)
    if not torch.is_tensor(index) or index.dim() != 1 or index.numel() < 1:
        raise ValueError('index must be an integer [B] tensor, B >= 1')
    B = index.numel()
    _int_tensor(index, (B,), 'index', dev)
    if (not torch.is_tensor(state) or state.dtype != torch.int64 or tuple(state.shape) != (2,) or state.device != dev
            or not state.is_contiguous()):
        raise ValueError('state must be a contiguous int64 [2] tensor {seed, draw} on the device of edges3d')
    if not torch.is_tensor(ticket) or ticket.dtype != torch.int32 or ticket.numel() != 1 or ticket.device != dev:
        raise ValueError('ticket must be one zeroed int32 on the device of edges3d')
    import ctypes
    sh = (ctypes.c_float * (2 * Fe))(*[float(v) for v in f_shift])
    sc = (ctypes.c_float * (2 * Fe))(*[float(v) for v in f_scale])
    rows = torch.empty(B, R, 2 * Fe, device=dev, dtype=F32)
    labels = torch.empty(B, R, device=dev, dtype=torch.uint8)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    L.call('gpe_stitch_sample', edges, ne, gt if gt.numel() else None, nums, G, P, Lm, Fe, gt.shape[2], _int32(index, -1, G), B,
           n_stitched, n_non_stitched, (1 if shuffle_pairs else 0) | (2 if shuffle_pairs_order else 0), sh, sc, state, ticket, rows,
           labels, status)
    return rows, labels.view(torch.bool), status

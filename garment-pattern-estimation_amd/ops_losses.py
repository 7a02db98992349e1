"""The pattern and stitch losses around their kernels (SparsemaxLossFn, PatternLossFn, StitchLossFn) and the ground-truth matching
that precedes them (stitch_renumber, panel_shift, origin_match, order_match).  Reached as ops.X: ops.py re-exports every name of
__all__.  SparsemaxFn, the network's own sparsemax, stays in ops.py with the model operators; the pair loss of the stitch
classifier is in ops_stitch."""
import torch

from . import _lib as L
from ._opbase import F32, _dev_check, _row_stride, _view_strides

__all__ = ['SparsemaxLossFn', 'LOSS_SHAPE', 'LOSS_LOOP', 'LOSS_ROT', 'LOSS_TR', 'PatternLossFn', 'STITCH_MAIN',
           'STITCH_HARDNET', 'STITCH_FREE', 'STITCH_SUP', 'StitchLossFn', 'stitch_renumber', 'panel_shift', 'origin_match',
           'order_match']


class SparsemaxLossFn(torch.autograd.Function):
    """entmax.SparsemaxLoss()(x, target) as nn/metrics/composed_loss.py:323-332 calls it: mean over rows of the sparsemax
    Fenchel-Young loss; gradient (sparsemax(x) - onehot(target)) / rows."""

    @staticmethod
    def forward(ctx, x, target):
        _dev_check(x)
        M, W = x.shape
        if x.stride(1) != 1:
            x = x.contiguous()
        tgt = target.to(torch.int32).contiguous()
        if tgt.numel() != M:
            raise ValueError('SparsemaxLoss: %d targets for %d rows' % (tgt.numel(), M))
        gx = torch.empty(M, W, device=x.device, dtype=F32)
        part = torch.empty((M + 255) // 256, device=x.device, dtype=torch.float64)
        loss = torch.empty(1, device=x.device, dtype=F32)
        bad = torch.zeros(1, device=x.device, dtype=torch.int32)
        L.call('gpe_sparsemax_loss', x, x.stride(0), tgt, M, W, gx, W, part, loss, bad)
        if bad.item():
            raise IndexError('SparsemaxLoss: a segmentation label lies outside [0, %d)' % W)
        ctx.save_for_backward(gx)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        gx, = ctx.saved_tensors
        out = torch.empty_like(gx)
        L.call('gpe_scale_dev', gx, g.reshape(1).to(F32).contiguous(), out, gx.numel())
        return out, None


# -------------------------------------------------------------------------------------------------
# loss (the caller-side step right after the path) and its ground-truth matching
# -------------------------------------------------------------------------------------------------
LOSS_SHAPE, LOSS_LOOP, LOSS_ROT, LOSS_TR = 1, 2, 4, 8


class PatternLossFn(torch.autograd.Function):
    """ComposedPatternLoss._main_losses (nn/metrics/composed_loss.py:294-321) + PanelLoopLoss (nn/metrics/losses.py:19-51)
    in one forward and one backward launch.  Returns a [5] tensor {total, shape, loop, rotation, translation}; only
    element 0 carries gradient."""

    @staticmethod
    def forward(ctx, outlines, rotations, translations, gt_ol, gt_rot, gt_tr, num_edges, flags, pad0, pad1, loop_w):
        _dev_check(outlines)
        dev = outlines.device
        B, P, Lp = outlines.shape[:3]
        sb, sp, sl = _view_strides(outlines)
        R = rotations.shape[-1] if rotations is not None else 0
        T = translations.shape[-1] if translations is not None else 0
        rs = _row_stride(rotations, P) if rotations is not None else 0
        ts = _row_stride(translations, P) if translations is not None else 0
        part = torch.empty(B, 4, device=dev, dtype=torch.float64)
        loop_sums = torch.empty(B * P, 2, device=dev, dtype=F32)
        out = torch.empty(5, device=dev, dtype=F32)
        args = (outlines, sb, sp, sl, rotations, rs, translations, ts, gt_ol, gt_rot, gt_tr, num_edges, B, P, Lp, R, T,
                flags, float(pad0), float(pad1), float(loop_w))
        L.call('gpe_pattern_loss_fwd', *args, part, loop_sums, out)
        ctx.args = args
        ctx.loop_sums = loop_sums
        ctx.shapes = (B, P, Lp, R, T)
        ctx.need = (rotations is not None and rotations.requires_grad,
                    translations is not None and translations.requires_grad)
        return out

    @staticmethod
    def backward(ctx, g):
        B, P, Lp, R, T = ctx.shapes
        dev = g.device
        g = g.contiguous()
        g_ol = torch.empty(B, P, Lp, 4, device=dev, dtype=F32)
        g_rot = torch.empty(B, P, R, device=dev, dtype=F32) if ctx.need[0] else None
        g_tr = torch.empty(B, P, T, device=dev, dtype=F32) if ctx.need[1] else None
        # g[0] is the upstream gradient of `total` (a device scalar: no host sync)
        L.call('gpe_pattern_loss_bwd', *ctx.args, ctx.loop_sums, g, g_ol, g_rot, g_tr)
        return g_ol, g_rot, g_tr, None, None, None, None, None, None, None, None


STITCH_MAIN, STITCH_HARDNET, STITCH_FREE, STITCH_SUP = 1, 2, 4, 8


class StitchLossFn(torch.autograd.Function):
    """ComposedPatternLoss._stitch_losses (nn/metrics/composed_loss.py:336-362): PatternStitchLoss (nn/metrics/losses.py:54-180,
    both negative-term variants), the supervised stitch-tag MSE and the free-edge BCE-with-logits in one forward and one
    backward launch.  Returns a [5] tensor {total, similarity, negative, supervised, free}; only element 0 carries gradient.
    stitch_tags [B,P,L,D] and free_logits [B,P,L] are the strided views of the panel decoder's output."""

    @staticmethod
    def forward(ctx, stitch_tags, free_logits, stitches, nums, gt_mask, gt_tags, flags, margin, sup_w):
        ref = stitch_tags if stitch_tags is not None else free_logits
        _dev_check(ref)
        dev = ref.device
        B, P, Lp = ref.shape[:3]
        D = stitch_tags.shape[3] if stitch_tags is not None else 0
        ts = _view_strides(stitch_tags) if stitch_tags is not None else (0, 0, 0)
        ms = (free_logits.stride(0), free_logits.stride(1), free_logits.stride(2)) if free_logits is not None else (0, 0, 0)
        S = stitches.shape[2] if stitches is not None else 0
        part = torch.empty(B, 6, device=dev, dtype=torch.float64)
        out = torch.empty(5, device=dev, dtype=F32)
        args = (stitch_tags, ts[0], ts[1], ts[2], D, free_logits, ms[0], ms[1], ms[2], stitches, nums, S, gt_mask, gt_tags,
                B, P, Lp, flags, float(margin), float(sup_w))
        L.call('gpe_stitch_loss_fwd', *args, part, out)
        ctx.args, ctx.part, ctx.shape = args, part, (B, P, Lp, D)
        ctx.need = (stitch_tags is not None and bool(flags & (STITCH_MAIN | STITCH_SUP)),
                    free_logits is not None and bool(flags & STITCH_FREE))
        return out

    @staticmethod
    def backward(ctx, g):
        B, P, Lp, D = ctx.shape
        dev = g.device
        g = g.contiguous()
        g_tags = torch.empty(B, P, Lp, D, device=dev, dtype=F32) if ctx.need[0] else None
        g_mask = torch.empty(B, P, Lp, device=dev, dtype=F32) if ctx.need[1] else None
        L.call('gpe_stitch_loss_bwd', *ctx.args, ctx.part, g, g_tags, g_mask)
        return g_tags, g_mask, None, None, None, None, None, None, None


def stitch_renumber(stitches, nums, P, Lp, perm=None, lead=None, num_edges=None):
    """composed_loss.py:592-620 (`perm`: the panel-order permutation) and :727-755 (`lead` / `num_edges`: the panel-origin
    shift) applied to the ground-truth stitches [B,2,S] int64 -> a new tensor."""
    B, _, S = stitches.shape
    out = torch.empty_like(stitches)
    L.call('gpe_stitch_renumber', stitches, nums, B, S, P, Lp, perm, lead, num_edges, out)
    return out


def panel_shift(feat, lead, num_edges):
    """composed_loss.py:705-725 `_per_panel_shift` on per-edge ground truth [B,P,L] or [B,P,L,D] (fp32) -> a new tensor."""
    _dev_check(feat)
    feat = feat.contiguous()
    Lp = feat.shape[2]
    D = feat.shape[3] if feat.dim() == 4 else 1
    out = torch.empty_like(feat)
    L.call('gpe_panel_shift', feat, D, lead, num_edges, feat.shape[0] * feat.shape[1], Lp, out)
    return out


def origin_match(outlines, gt_ol, num_edges):
    """composed_loss.py:656-703 `_batch_edge_order_match`: -> (gt outlines with every panel's edge loop shifted to the
    origin that best matches the prediction, leading edge per panel int32 [B*P])."""
    _dev_check(outlines)
    B, P, Lp, D = gt_ol.shape
    sb, sp, sl = _view_strides(outlines)
    out = torch.empty_like(gt_ol)
    lead = torch.empty(B * P, device=gt_ol.device, dtype=torch.int32)
    L.call('gpe_origin_match', outlines.detach(), sb, sp, sl, gt_ol, D, num_edges, B, P, Lp, out, lead)
    return out, lead


def order_match(pred_feat, gt_feat):
    """composed_loss.py:530-570 `_panel_order_match` (the greedy assignment): -> int64 [B, P] permutation of GT panels,
    and a device flag that is non-zero if the matching left a finite distance behind (the reference raises then)."""
    _dev_check(pred_feat)
    B, P, D = pred_feat.shape
    perm = torch.empty(B, P, device=pred_feat.device, dtype=torch.int64)
    fail = torch.zeros(1, device=pred_feat.device, dtype=torch.int32)
    L.call('gpe_order_match', pred_feat.contiguous(), gt_feat.contiguous(), B, P, D, perm, fail)
    return perm, fail

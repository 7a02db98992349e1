"""A prediction decoded to a sewing pattern (Garment3DPatternFullDataset._pred_to_pattern, nn/data/datasets.py:731-767;
tags_to_stitches :917-968; NNSewingPattern.pattern_from_tensors / panel_from_numeric / _edge_dict,
nn/data/pattern_converter.py:118-187, 228-271, 510-515) restated from its definition in plain fp64 numpy, one garment and one panel
at a time — the yardstick of tests/test_pattern_decode_host.py and tests/test_gpu_pattern_decode.py, and the margin check of
scripts/make_pattern_decode_golden.py.

`restate(...)` returns the output tensors of ops.pattern_decode (include/gpe_hip.h gpe_pattern_decode) as numpy arrays and the
smallest relative decision margin it met: the distance of every threshold test (padding rows at 1.5, loop closure at 3, curvature
at 0.01, the sigmoid at 0.5) from its bound, of the odd-count drop from the runner-up logit and of every greedy pairing step from
the next candidate.  Inputs whose margin is below quality_restate.MARGIN may legitimately pair differently with fp32 distances."""
import numpy as np

KEYS = ('num_edges', 'edge_slot', 'num_verts', 'closed', 'new_panel_id', 'num_panels', 'vertices', 'curvature', 'rotations',
        'translations', 'curved', 'stitches', 'num_stitches', 'stitch_flags', 'first_invalid')


def _np(t):
    if t is None:
        return None
    if hasattr(t, 'detach'):
        t = t.detach().cpu()
        if t.dtype.is_floating_point:
            t = t.double()
        return t.numpy()
    return np.asarray(t)


def _rel(a, bound):
    a = np.abs(np.asarray(a, np.float64))
    a = a[np.isfinite(a)]
    return float((np.abs(a - bound) / bound).min()) if a.size else float('inf')


def greedy_pairs(tags, margins):
    """pairs of row indices: the globally closest remaining pair (i < j) first, ties to the smallest (i, j); a non-finite distance
    is never taken, and the pairing stops when nothing else is left.  With a list in `margins`, every step appends the relative
    gap to the next remaining candidate.  Taken rows and columns leave the matrix, which keeps its row-major order."""
    m = len(tags)
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.sqrt(((tags[:, None, :] - tags[None, :, :]) ** 2).sum(-1))
    d[~np.isfinite(d)] = np.inf
    d[np.tril_indices(m)] = np.inf
    alive = np.arange(m)
    pairs = []
    while len(alive) >= 2:
        n = len(alive)
        i, j = divmod(int(np.argmin(d)), n)
        best = d[i, j]
        if not np.isfinite(best):
            break
        if margins is not None:
            second = np.partition(d.ravel(), 1)[1]
            if np.isfinite(second):
                margins.append((second - best) / max(best, 1e-30))
        pairs.append((int(alive[i]), int(alive[j])))
        keep = np.ones(n, bool)
        keep[[i, j]] = False
        d, alive = d[np.ix_(keep, keep)], alive[keep]
    return pairs


def tags_to_stitches(tags, logits, margins, pair_margins=True):
    """one garment: tags [E, D], logits [E] -> list of (edge id, edge id) in the order taken"""
    with np.errstate(over='ignore'):
        sig = 1.0 / (1.0 + np.exp(-logits))
    margins.append(_rel(sig, 0.5))
    ids = np.nonzero(sig <= 0.5)[0]                        # exactly 0.5 rounds to 0 (non-free); NaN is free
    if len(ids) < 2:
        return []
    if len(ids) % 2:
        lg = logits[ids]
        top = np.sort(lg)[::-1]
        if np.isfinite(top[:2]).all():
            margins.append((top[0] - top[1]) / max(abs(top[0]), 1e-30))
        ids = np.delete(ids, int(np.argmax(lg)))
    return [(int(ids[i]), int(ids[j])) for i, j in greedy_pairs(tags[ids], margins if pair_margins else None)]


def decode_panel(rows, margins):
    """rows [L, 4] un-standardised -> None (empty) or (slots, vertices [nv, 2], closed, curvature [n, 2], curved [n]); `kept` per
    row comes back in any case"""
    with np.errstate(invalid='ignore'):
        kept = ~(np.abs(rows) <= 1.5).all(axis=1)
    margins.append(_rel(rows, 1.5))
    slots = np.nonzero(kept)[0]
    if len(slots) < 3:
        return kept, None
    e = rows[slots]
    verts = [np.zeros(2)]
    for k in range(len(e) - 1):
        verts.append(verts[k] + e[k, :2])
    fin = verts[-1] + e[-1, :2]
    margins.append(_rel(fin, 3.0))
    with np.errstate(invalid='ignore'):
        closed = bool((np.abs(fin) <= 3.0).all())
        curved = ~(np.abs(e[:, 2:4]) <= 0.01).all(axis=1)
    if not closed:
        verts.append(fin)
    margins.append(_rel(e[:, 2:4], 0.01))
    return kept, (slots, np.stack(verts), closed, e[:, 2:4], curved)


def restate(preds, data_stats, explicit_stitch_tags=False, stitches=None, num_stitches=None, pair_margins=True, detail=None):
    """-> ({name: array} with the names and layouts of ops.pattern_decode, smallest relative margin).  `data_stats` is
    data_config['standardize']; preds a dict of tensors or arrays.  A dict in `detail` receives the margin's two parts: 'threshold'
    (padding rows, closure, curvature: decided in fp64 by the kernel as well, so the same whatever the margin) and 'pairing' (the
    sigmoid, the odd-count drop and the greedy steps, where the kernel has fp32)."""
    margins, thresholds = [], []
    sh, sc = data_stats['gt_shift'], data_stats['gt_scale']
    un = lambda k: _np(preds[k]) * np.asarray(sc[k], np.float64) + np.asarray(sh[k], np.float64)     # noqa: E731
    ol, rot, tr = un('outlines'), un('rotations'), un('translations')
    B, P, L = ol.shape[:3]
    PL = P * L
    S = PL // 2 if stitches is None else _np(stitches).shape[2]
    o = {'num_edges': np.zeros((B, P), np.int32), 'edge_slot': np.full((B, P, L), -1, np.int32),
         'num_verts': np.zeros((B, P), np.int32), 'closed': np.zeros((B, P), np.int32),
         'new_panel_id': np.full((B, P), -1, np.int32), 'num_panels': np.zeros(B, np.int32),
         'vertices': np.zeros((B, P, L + 1, 2)), 'curvature': np.zeros((B, P, L, 2)), 'rotations': rot, 'translations': tr,
         'curved': np.zeros((B, P, L), np.int32), 'stitches': np.zeros((B, 2, S), np.int32), 'num_stitches': np.zeros(B, np.int32),
         'stitch_flags': np.zeros((B, S), np.int32), 'first_invalid': np.full(B, -1, np.int32)}
    if stitches is None:
        tags = _np(preds['stitch_tags']).reshape(B, PL, -1)
        if explicit_stitch_tags:
            tags = tags * np.asarray(sc['stitch_tags'], np.float64) + np.asarray(sh['stitch_tags'], np.float64)
        logits = _np(preds['free_edges_mask']).reshape(B, PL)
    else:
        given = _np(stitches).astype(np.int64)
        given_num = None if num_stitches is None else _np(num_stitches).reshape(B).astype(np.int64)
    for b in range(B):
        kept_all = np.zeros(PL, bool)
        for p in range(P):
            kept, panel = decode_panel(ol[b, p], thresholds)
            kept_all[p * L:(p + 1) * L] = kept
            if panel is None:
                continue
            slots, verts, closed, curv, curved = panel
            n = len(slots)
            o['num_edges'][b, p], o['num_verts'][b, p], o['closed'][b, p] = n, len(verts), closed
            o['edge_slot'][b, p, :n] = slots
            o['vertices'][b, p, :len(verts)] = verts
            o['curvature'][b, p, :n] = curv
            o['curved'][b, p, :n] = curved
            o['new_panel_id'][b, p] = o['num_panels'][b]
            o['num_panels'][b] += 1
        if stitches is None:
            found = tags_to_stitches(tags[b], logits[b], margins, pair_margins)
        else:
            cnt = S if given_num is None else int(min(max(given_num[b], 0), S))
            found = [(int(given[b, 0, k]), int(given[b, 1, k])) for k in range(cnt)
                     if not (given[b, 0, k] == 0 and given[b, 1, k] == 0)]
        for k, pair in enumerate(found):
            f = 0
            for e in pair:
                pp = e // L if e >= 0 else -1
                if pp < 0 or pp >= P or o['new_panel_id'][b, pp] < 0:
                    f |= 1
                if 0 <= e < PL and not kept_all[e]:
                    f |= 2
            o['stitches'][b, :, k] = pair
            o['stitch_flags'][b, k] = f
            if f & 1 and o['first_invalid'][b] < 0:
                o['first_invalid'][b] = k
        o['num_stitches'][b] = len(found)
    if detail is not None:
        detail.update(threshold=float(min(thresholds, default=np.inf)), pairing=float(min(margins, default=np.inf)))
    return o, float(min(margins + thresholds, default=np.inf))


def host_loop(preds, data_stats, explicit_stitch_tags=False):
    """the same without the sort behind every pairing step's margin: what scripts/pattern_decode_bench.py times as the per-garment
    host loop"""
    return restate(preds, data_stats, explicit_stitch_tags, pair_margins=False)[0]


# ---- deliberate faults on top of quality_restate.make_batch (scripts/make_pattern_decode_golden.py, tests) ----------------------------
def plant_fault(rng, preds, b, kind, data_stats):
    """garment b of a make_batch prediction (float32 tensors, changed in place) gets one fault the decode has to handle:
    'mid_drop'        a row in the middle of a real panel becomes a padding row (the kept rows are compacted);
    'two_rows'        the first panel keeps two rows only: an empty panel in front of real ones (later panels are renumbered);
    'empty_stitch'    two slots of the last panel — empty in every make_batch draw, which fills at most 11 — look stitched and share a tag;
    'dropped_stitch'  a padding row at the end of a real panel and a kept row of another look stitched and share a tag."""
    import torch
    sh = np.asarray(data_stats['gt_shift']['outlines'], np.float64)
    sc = np.asarray(data_stats['gt_scale']['outlines'], np.float64)
    pad = torch.tensor(-sh / sc, dtype=torch.float32)
    ol, tags, logit = preds['outlines'], preds['stitch_tags'], preds['free_edges_mask']
    P, L = ol.shape[1:3]
    un = ol[b].double().numpy() * sc + sh
    n = (~(np.abs(un) <= 1.5).all(-1)).sum(-1)             # kept rows per panel
    D = tags.shape[-1]
    point = torch.tensor(rng.uniform(5, 6, D) * rng.choice([-1, 1], D), dtype=torch.float32)      # away from make_batch's tag cube
    if kind == 'mid_drop':
        p = int(np.argmax(n))
        if n[p] >= 5:
            ol[b, p, 2] = pad
    elif kind == 'two_rows':
        ol[b, 0, 2:] = pad
    elif kind == 'empty_stitch':
        for l in (1, 3):
            logit[b, P - 1, l] = -2.5
            tags[b, P - 1, l] = point + torch.tensor(rng.normal(0, 0.01, D), dtype=torch.float32)
    elif kind == 'dropped_stitch':
        short = [p for p in range(P) if 3 <= n[p] < L]
        if short:
            p = short[0]
            q = 1 if p == 0 else 0
            for pp, l in ((p, L - 1), (q, 0)):
                logit[b, pp, l] = -2.5
                tags[b, pp, l] = point + torch.tensor(rng.normal(0, 0.01, D), dtype=torch.float32)

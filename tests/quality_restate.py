"""The quality metrics of ComposedPatternLoss (nn/metrics/composed_loss.py:365-424, nn/metrics/metrics.py:13-325,
nn/data/datasets.py:917-968) restated from their definitions in vectorised fp64 numpy — the yardstick of
tests/test_quality_host.py and tests/test_gpu_quality.py, and the margin check of scripts/make_quality_golden.py.

`restate(...)` evaluates on the ground truth AFTER the loss's order / origin matching and returns the metric dict (None where
the reference gives None) and the smallest relative decision margin it met: the distance of every threshold test (isclose,
loop closure, sigmoid rounding, the odd-count drop) from its bound and of every greedy pairing step from the runner-up
candidate.  Inputs whose margin is below MARGIN may legitimately decide differently in fp32."""
import numpy as np
import torch

MARGIN = 1e-4


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
    """relative distance of `a` from `bound` (elementwise, fp64)"""
    return np.abs(a - bound) / np.maximum(np.abs(bound), 1e-30)


def _verts(e):
    """[n, 4] un-standardised edges -> [2n+1, 2] outline vertices (origin, then curvature point and end of every edge)"""
    ends = np.cumsum(e[:, :2], axis=0)
    starts = np.vstack([np.zeros((1, 2)), ends[:-1]])
    perp = np.stack([-e[:, 1], e[:, 0]], axis=1)
    curv = starts + e[:, 2:3] * e[:, :2] + e[:, 3:4] * perp
    v = np.empty((2 * len(e) + 1, 2))
    v[0] = 0.0
    v[1::2] = curv
    v[2::2] = ends
    return v - v.mean(axis=0)


def greedy_pairs(tags, margins):
    """pairs of row indices by repeatedly taking the globally closest remaining pair (i < j), ties to the smallest (i, j);
    appends to `margins` the relative gap between every chosen distance and the next remaining candidate"""
    m = len(tags)
    d = np.sqrt(((tags[:, None, :] - tags[None, :, :]) ** 2).sum(-1))
    d[np.tril_indices(m)] = np.inf
    pairs = []
    for _ in range(m // 2):
        flat = np.argmin(d)
        i, j = divmod(int(flat), m)
        best = d[i, j]
        rest = np.sort(d[np.isfinite(d)].ravel())
        if len(rest) > 1:
            margins.append((rest[1] - best) / max(best, 1e-30))
        pairs.append((i, j))
        d[[i, j], :] = np.inf
        d[:, [i, j]] = np.inf
    return pairs


def restate(q_components, epoch, epoch_with_stitches, data_stats, explicit_stitch_tags, preds, gt):
    """-> (metrics dict, smallest relative margin).  `data_stats` is data_config['standardize']; preds / gt are dicts of
    tensors or arrays (gt: the matched ground truth)."""
    q = q_components
    margins = []
    ol_sh = np.asarray(data_stats['gt_shift']['outlines'], np.float32).astype(np.float64)
    ol_sc = np.asarray(data_stats['gt_scale']['outlines'], np.float32).astype(np.float64)
    # the bounds as the reference forms them in fp32
    pad = (-ol_sh.astype(np.float32) / ol_sc.astype(np.float32)).astype(np.float64)
    tol = (np.float32(0.07) + np.abs(np.float32(1e-5) * pad.astype(np.float32))).astype(np.float64)
    thr = (np.float32(3.0) / ol_sc[:2].astype(np.float32)).astype(np.float64)
    out = {}
    ol = _np(preds['outlines'])
    B, P, L = ol.shape[:3]
    ne = _np(gt['num_edges']).reshape(B, P).astype(np.int64)
    correct = None
    if 'discrete' in q:
        num_panels = _np(gt['num_panels']).reshape(B).astype(np.float64)
        dev = np.abs(ol - pad)
        margins.append(_rel(dev, tol).min())
        cnt = (~(dev <= tol).all(-1)).sum(-1)
        loop = np.abs(ol[..., :2].sum(2))
        margins.append(_rel(loop, thr).min())
        cnt = cnt + (loop > thr).any(-1)
        real = cnt >= 3
        correct = real.sum(1) == num_panels
        ratio = (real & (cnt == ne)).sum(1) / num_panels
        out['num_panels_accuracy'] = correct.mean()
        out['num_edges_accuracy'] = ratio.mean()
        out['corr_num_edges_accuracy'] = ratio[correct].mean() if correct.any() else float('nan')
    if 'shape' in q:
        pu = ol * ol_sc + ol_sh
        gu = _np(gt['outlines']) * ol_sc + ol_sh
        errs, corr_errs = [], []
        for b in range(B):
            for p in range(P):
                n = ne[b, p]
                if n < 3:
                    continue
                e = np.sqrt(((_verts(gu[b, p, :n]) - _verts(pu[b, p, :n])) ** 2).sum(-1)).mean()
                errs.append(e)
                if correct is not None and correct[b]:
                    corr_errs.append(e)
        out['panel_shape_l2'] = float(np.mean(errs)) if errs else float('nan')
        out['corr_panel_shape_l2'] = float(np.mean(corr_errs)) if corr_errs else None
    for comp, key, name in (('rotation', 'rotations', 'rotation_l2'), ('translation', 'translations', 'translation_l2')):
        if comp not in q:
            continue
        sh = np.asarray(data_stats['gt_shift'][key], np.float64)
        sc = np.asarray(data_stats['gt_scale'][key], np.float64)
        l2 = np.sqrt((((_np(gt[key]) * sc + sh) - (_np(preds[key]) * sc + sh)) ** 2).sum(-1))
        out[name] = l2.mean()
        out['corr_' + name] = l2[correct].mean() if correct is not None and correct.any() else None
    if epoch >= epoch_with_stitches:
        logits = _np(preds['free_edges_mask']).reshape(B, P * L)
        sig = 1.0 / (1.0 + np.exp(-logits))
        if 'stitch' in q or 'free_class' in q:
            margins.append(_rel(sig, 0.5).min())
        if 'stitch' in q:
            tags = _np(preds['stitch_tags']).reshape(B, P * L, -1)
            if explicit_stitch_tags:
                tags = tags * np.asarray(data_stats['gt_scale']['stitch_tags']) + np.asarray(data_stats['gt_shift']['stitch_tags'])
            st = _np(gt['stitches']).astype(np.int64)
            nst = _np(gt['num_stitches']).reshape(B).astype(np.int64)
            prec, rec, cprec, crec = [], [], [], []
            for b in range(B):
                ids = np.nonzero(sig[b] <= 0.5)[0]
                if len(ids) < 2:
                    prec.append(0.0), rec.append(0.0)
                    continue
                if len(ids) % 2:
                    lg = logits[b, ids]
                    top = np.sort(lg)[::-1]
                    margins.append((top[0] - top[1]) / max(abs(top[0]), 1e-30))
                    ids = np.delete(ids, int(np.argmax(lg)))
                pairs = {tuple(sorted((int(ids[i]), int(ids[j])))) for i, j in greedy_pairs(tags[b, ids], margins)}
                n = nst[b]
                gts = {tuple(sorted((int(st[b, 0, k]), int(st[b, 1, k])))) for k in range(max(0, min(n, st.shape[2])))}
                good = len(pairs & gts)
                pr, rc = good / len(pairs), (good / n if n else 0.0)
                prec.append(pr), rec.append(rc)
                if correct is not None and correct[b]:
                    cprec.append(pr), crec.append(rc)
            out['stitch_precision'] = float(np.sum(prec)) / B
            out['stitch_recall'] = float(np.sum(rec)) / B
            out['corr_stitch_precision'] = float(np.mean(cprec)) if cprec else None
            out['corr_stitch_recall'] = float(np.mean(crec)) if crec else None
        if 'free_class' in q:
            cls = (sig > 0.5).astype(np.float64)
            out['free_edge_acc'] = (cls == _np(gt['free_edges_mask']).reshape(B, P * L).astype(np.float64)).mean()
    out = {k: (None if v is None else float(v)) for k, v in out.items()}
    return out, float(min(margins)) if margins else float('inf')


# ---- garment-shaped inputs (scripts/make_quality_golden.py, tests/test_gpu_quality.py) --------------------------------------
def _loop_cm(rng, n):
    """n edges of a closed, roughly elliptic panel outline in cm + curvature (c0, c1)"""
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    ang += np.arange(n) * 0.05                                          # no two vertices too close
    rx, ry = rng.uniform(15, 50), rng.uniform(15, 50)
    v = np.stack([rx * np.cos(ang), ry * np.sin(ang)], 1)
    e = np.roll(v, -1, 0) - v
    c0 = rng.uniform(0.3, 0.7, n)
    c1 = np.where(rng.uniform(size=n) < 0.5, rng.uniform(-0.2, 0.2, n), 0.0)
    return np.concatenate([e, c0[:, None], c1[:, None]], 1)


def _tag_points(rng, k, D=3, sep=0.6):
    pts = []
    while len(pts) < k:
        c = rng.uniform(-3, 3, D)
        if all(np.linalg.norm(c - p) > sep for p in pts):
            pts.append(c)
    return np.array(pts).reshape(k, D)


def draw_pattern(rng, P, L, S, sh, sc, kind, all_stitches=False):
    """one garment: ground truth (standardised) + prediction.  kind: 'ok', 'pad_real', 'open', 'extra', or stitch specials
    'free0' (no non-free edge), 'free1' (one), 'odd', 'nost' (num_stitches 0 but stitched-looking edges)"""
    pad = -sh / sc
    npan = int(rng.integers(6 if all_stitches else 3, 12))
    ne = np.zeros(P, np.int64)
    ol = np.tile(pad, (P, L, 1))
    for p in range(npan):
        n = int(rng.integers(3, L + 1))
        ne[p] = n
        ol[p, :n] = (_loop_cm(rng, n) - sh) / sc
    pred = ol + rng.normal(0, 0.004, ol.shape)
    if kind == 'pad_real':                   # a padding row of a real panel becomes an edge
        p = int(rng.integers(0, npan))
        if ne[p] < L:
            pred[p, L - 1, :2] += 0.3
    elif kind == 'open':                     # loop opened by ~ 10 cm
        p = int(rng.integers(0, npan))
        pred[p, 0, 0] += 10.0 / sc[0]
    elif kind == 'extra' and npan < P:       # an extra non-empty panel
        n = int(rng.integers(3, L + 1))
        pred[npan, :n] = (_loop_cm(rng, n) - sh) / sc
    # stitches: pairs of distinct real edges, each pair shares a tag point
    edges = [p * L + e for p in range(npan) for e in range(ne[p])]
    rng.shuffle(edges)
    nst = min(S if all_stitches else int(rng.integers(3, S + 1)), len(edges) // 2)
    st = np.zeros((2, S), np.int64)
    st[0, :nst], st[1, :nst] = edges[0:2 * nst:2], edges[1:2 * nst:2]
    free = np.ones(P * L, bool)
    free[st[:, :nst].ravel()] = False
    pts = _tag_points(rng, nst + P * L // 4)
    tags = rng.uniform(-3, 3, (P * L, 3))
    tags[st[0, :nst]] = pts[:nst] + rng.normal(0, 0.01, (nst, 3))
    tags[st[1, :nst]] = pts[:nst] + rng.normal(0, 0.01, (nst, 3))
    logit = np.where(free, rng.uniform(1, 4, P * L), -rng.uniform(1, 4, P * L))
    if kind == 'free0':
        logit = rng.uniform(1, 4, P * L)
    elif kind == 'free1':
        logit = rng.uniform(1, 4, P * L)
        logit[st[0, 0]] = -2.0
    elif kind == 'odd':                      # one stitched edge looks free -> its partner is the odd one
        logit[st[1, 0]] = rng.uniform(1, 4)
    elif kind == 'nost':
        nst = 0
    else:                                    # a free edge (with its own tag point) is mistaken for a stitched one
        if rng.uniform() < 0.5:
            f = int(np.nonzero(free)[0][0])
            logit[f] = -rng.uniform(1, 4)
            tags[f] = pts[nst]
    return dict(ne=ne, num_panels=npan, ol=ol, pred=pred, st=st, nst=nst, free=free.reshape(P, L),
                tags=tags.reshape(P, L, 3), logit=logit.reshape(P, L))


def make_batch(rng, B, P, L, S, data_config, kinds, all_stitches=False):
    sh = np.asarray(data_config['standardize']['gt_shift']['outlines'], np.float32).astype(np.float64)
    sc = np.asarray(data_config['standardize']['gt_scale']['outlines'], np.float32).astype(np.float64)
    pats = [draw_pattern(rng, P, L, S, sh, sc, kinds[b % len(kinds)], all_stitches) for b in range(B)]
    f = lambda k: torch.tensor(np.stack([p[k] for p in pats]), dtype=torch.float32)       # noqa: E731
    gt = {'outlines': f('ol'), 'num_edges': torch.tensor(np.stack([p['ne'] for p in pats])),
          'num_panels': torch.tensor([p['num_panels'] for p in pats]),
          'rotations': torch.tensor(rng.normal(0, 1, (B, P, 4)), dtype=torch.float32),
          'translations': torch.tensor(rng.normal(0, 1, (B, P, 3)), dtype=torch.float32),
          'stitches': torch.tensor(np.stack([p['st'] for p in pats])),
          'num_stitches': torch.tensor([p['nst'] for p in pats]),
          'free_edges_mask': torch.tensor(np.stack([p['free'] for p in pats]))}
    gt['empty_panels_mask'] = gt['num_edges'] < 3
    gt['stitch_tags'] = f('tags')
    preds = {'outlines': f('pred'),
             'rotations': gt['rotations'] + torch.tensor(rng.normal(0, 0.05, (B, P, 4)), dtype=torch.float32),
             'translations': gt['translations'] + torch.tensor(rng.normal(0, 0.05, (B, P, 3)), dtype=torch.float32),
             'stitch_tags': f('tags'), 'free_edges_mask': f('logit')}
    return preds, gt


def permute_panels(rng, preds, gt, shift_origin):
    """predictions in another panel order (and, with origin matching, every panel's loop starting elsewhere): the loss's
    matchings have something to undo"""
    B, P, L = preds['outlines'].shape[:3]
    for b in range(B):
        perm = torch.tensor(rng.permutation(P))
        for k in preds:
            preds[k][b] = preds[k][b][perm]
        if shift_origin:
            ne = gt['num_edges'][b][perm]
            for p in range(P):
                n = int(ne[p])
                if n >= 3:
                    s = int(rng.integers(0, n))
                    idx = torch.tensor([(i + s) % n for i in range(n)])
                    for k in ('outlines', 'stitch_tags', 'free_edges_mask'):
                        preds[k][b, p, :n] = preds[k][b, p, idx]

#!/usr/bin/env python3
"""Generates tests/golden/stitch_pairs_<tag>.pt: what the REFERENCE'S OWN prediction-time stitch recovery returns —
NNSewingPattern.all_edge_pairs, stitches_from_pair_classifier, _stitches_as_set and _stitch_entry
(nn/data/pattern_converter.py:411-508,554-567), called unbound and unmodified on a small stand-in object that supplies
panel_order(), _3D_edges_per_panel(), `pattern` and `name`, with the reference's own StitchOnEdge3DPairs carrying the shipped
trained weights (the state dict of tests/golden/stitch_pairs_known_answer.pt) and device_ids = ['cpu'].

Only runnable where the reference checkout exists (like scripts/make_quality_golden.py, whose sys.path set-up on the read-only
stubs it shares).  The fixtures hold data only: edges, edge counts, the statistics, the reference's pair order, its fp32 logits and
its recorded stitch list (None where the reference raises: exactly one positive makes `.squeeze().tolist()` an int).  The pair
rows themselves are kept for one small garment.  Seeded: a re-run writes the same files.

Garments are closed 3D edge loops in cm inside the box of the statistics; a planted stitch is an edge copied reversed onto another
panel with ~1 cm of noise (the loop is re-closed around it).  Decision margins are a CONDITION of a stored garment: with
tol = 1e-4 * max(1, max |logit|) (tests/stitch_pairs_restate.py tol_of) a draw is repeated while any fp64 logit lies within 4 tol
of 0 or the two best positives of an edge are closer than 4 tol, so that the device tests compare exactly, nothing excluded.

    python scripts/make_stitch_pairs_golden.py [REFERENCE_DIR]
"""
import os
import sys

import numpy as np
import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('GPE_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(REPO, 'oracle', 'refgen', 'stubs'), os.path.join(REF, 'nn'), REPO, os.path.join(REPO, 'tests')]

import nets as ref_nets  # noqa: E402  (the reference's module)
from data.pattern_converter import NNSewingPattern  # noqa: E402  (the reference's class)
import stitch_pairs_restate as R  # noqa: E402

torch.set_num_threads(1)
GOLDEN = os.path.join(REPO, 'tests', 'golden')


class StandIn:
    """the four things the reference's functions read from a pattern, and the functions themselves, unmodified"""
    all_edge_pairs = NNSewingPattern.all_edge_pairs
    stitches_from_pair_classifier = NNSewingPattern.stitches_from_pair_classifier
    _stitches_as_set = NNSewingPattern._stitches_as_set
    _stitch_entry = NNSewingPattern._stitch_entry

    def __init__(self, edges, num_edges):
        self.name = 'stand_in'
        self.pattern = {'stitches': []}
        self._order = ['p%02d' % p for p, n in enumerate(num_edges) if n > 0]
        self._edges = {'p%02d' % p: [edges[p, l].tolist() for l in range(int(n))] for p, n in enumerate(num_edges) if n > 0}

    def panel_order(self, force_update=False, pad_to_len=None):
        return self._order

    def _3D_edges_per_panel(self, randomize_direction=False):
        return self._edges


def slot(name):
    return int(name[1:])


def reference_model():
    fx = torch.load(os.path.join(GOLDEN, 'stitch_pairs_known_answer.pt'), weights_only=False)
    with open(os.path.join(REF, 'models/att/stitch_model.yaml')) as f:
        cfg = yaml.safe_load(f)
    model = ref_nets.StitchOnEdge3DPairs(dict(fx['data_config']), dict(fx['nn_config']), {})
    model.load_state_dict(fx['state_dict'])
    model.device_ids = ['cpu']
    model.eval()                    # (the reference's train() override returns None)
    st = cfg['dataset']['standardize']
    return model, fx, {'f_shift': [float(v) for v in st['f_shift']], 'f_scale': [float(v) for v in st['f_scale']]}


def draw_garment(rng, num_edges, stats, plants):
    """closed loops; plants: [((panel, edge) source, (panel, edge) target)]: the target becomes the reversed source + noise"""
    P, L = len(num_edges), max(int(max(num_edges)), 1)
    lo = np.asarray(stats['f_shift'][:3]) + 25.0
    hi = np.asarray(stats['f_shift'][:3]) + np.asarray(stats['f_scale'][:3]) - 25.0
    edges = np.zeros((P, L, 8), dtype=np.float32)
    for p, n in enumerate(num_edges):
        if n == 0:
            continue
        centre = rng.uniform(lo, hi)
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        v = np.cross(u, rng.normal(size=3))
        v /= np.linalg.norm(v)
        ang = np.sort(rng.uniform(0, 2 * np.pi, size=n))
        rad = rng.uniform(8.0, 22.0, size=n)
        verts = centre + rad[:, None] * (np.cos(ang)[:, None] * u + np.sin(ang)[:, None] * v)
        for l in range(n):
            curv = (0.0, 0.0) if rng.random() < 0.6 else (rng.uniform(0.2, 0.8), rng.uniform(-0.3, 0.3))
            edges[p, l] = np.concatenate([verts[l], verts[(l + 1) % n], curv])
    for (ps, es), (pt, et) in plants:
        n = int(num_edges[pt])
        src = edges[ps, es]
        start, end = src[3:6] + rng.normal(scale=0.6, size=3), src[0:3] + rng.normal(scale=0.6, size=3)
        edges[pt, et, 0:3], edges[pt, et, 3:6] = start, end
        edges[pt, et, 6:8] = (1.0 - src[6], -src[7]) if src[6] != 0 else (0.0, 0.0)
        edges[pt, (et - 1) % n, 3:6] = start            # keep the loop closed
        edges[pt, (et + 1) % n, 0:3] = end
    return edges


def record(tag, seed, num_edges, plants, model, state_dict, stats, want, keep_rows=False):
    """want(positives, per_edge_max_claims) -> bool: the property this case stands for"""
    rng = np.random.default_rng(seed)
    num_edges = np.asarray(num_edges, dtype=np.int32)
    for attempt in range(400):
        edges = draw_garment(rng, num_edges, stats, plants)
        pairs = R.enumerate_pairs(num_edges)
        lg64 = R.logits64(state_dict, R.pair_rows(edges, pairs), stats['f_shift'], stats['f_scale'])
        tol = R.tol_of(lg64)
        m0, gap = R.margins(pairs, lg64)
        claims = {}
        for k in np.nonzero(lg64 > 0)[0]:
            for e in R._edges_of(pairs[k]):
                claims[e] = claims.get(e, 0) + 1
        if m0 >= 4 * tol and gap >= 4 * tol and want(int((lg64 > 0).sum()), max(claims.values(), default=0)):
            break
    else:
        raise RuntimeError('%s: no draw with the wanted property and decision margins' % tag)
    # ---- the reference, unmodified ----
    obj = StandIn(edges, num_edges)
    with torch.no_grad():
        rows, mapping, _ = obj.all_edge_pairs(device='cpu')
        shift, scale = torch.tensor(stats['f_shift']), torch.tensor(stats['f_scale'])
        ref_logits = model((rows - shift) / scale).clone()
        try:
            obj.stitches_from_pair_classifier(model, stats)
            ref_st = [((slot(s[0]['panel']), slot(s[1]['panel']), s[0]['edge'], s[1]['edge']), float(s[0]['score']))
                      for s in obj.pattern['stitches']]
            ref_err = None
        except TypeError as e:
            ref_st, ref_err = None, 'TypeError: %s' % e
    order = np.asarray([(slot(a[0]), slot(b[0]), a[1], b[1]) for a, b in mapping], dtype=np.int8)
    assert (ref_logits.double().numpy() - lg64).__abs__().max() < tol, 'the restated logits disagree with the reference'
    fx = {'tag': tag, 'seed': seed, 'draws': attempt + 1, 'edges': torch.from_numpy(edges), 'num_edges': torch.from_numpy(num_edges),
          'f_shift': stats['f_shift'], 'f_scale': stats['f_scale'], 'ref_order': torch.from_numpy(order),
          'ref_logits': ref_logits.float(), 'ref_stitches': ref_st, 'ref_error': ref_err, 'plants': plants,
          'margin_zero': m0, 'margin_edge': gap, 'tol': tol, 'positives': int((lg64 > 0).sum())}
    if keep_rows:
        fx['ref_rows'] = rows.clone()
    out = os.path.join(GOLDEN, 'stitch_pairs_%s.pt' % tag)
    torch.save(fx, out)
    print('stitch_pairs_%-10s draws=%-3d edges=%-4d pairs=%-6d positives=%-3d ref stitches=%s  |logit|max=%.2f  margins %.3g / %.3g '
          '(4 tol = %.3g)  %.0f KB' % (tag, attempt + 1, int(num_edges.sum()), len(pairs), fx['positives'],
                                       'raises' if ref_st is None else len(ref_st), float(np.abs(lg64).max()), m0, gap, 4 * tol,
                                       os.path.getsize(out) / 1024))


def spread_plants(rng, num_edges, count):
    """`count` planted stitches between distinct edges of different present panels"""
    present = [p for p, n in enumerate(num_edges) if n > 0]
    used, out = set(), []
    while len(out) < count:
        a, b = rng.choice(present, size=2, replace=False)
        s, t = (int(a), int(rng.integers(num_edges[a]))), (int(b), int(rng.integers(num_edges[b])))
        # a target's neighbours are moved to re-close its loop: keep them out of other stitches
        nb = {(t[0], (t[1] + d) % int(num_edges[t[0]])) for d in (-1, 0, 1)}
        if s in used or nb & used or s in nb:
            continue
        used |= nb | {s}
        out.append((s, t))
    return out


if __name__ == '__main__':
    model, known, stats = reference_model()
    sd = known['state_dict']
    rng = np.random.default_rng(9100)
    small = [5, 0, 4, 6, 0, 0, 3, 5]
    record('small', 9101, small, spread_plants(rng, small, 4), model, sd, stats, lambda n, c: n >= 3, keep_rows=True)
    gaps = [0, 7, 0, 0, 8, 6, 0, 8, 5, 0, 7, 0]
    record('gaps', 9102, gaps, spread_plants(rng, gaps, 6), model, sd, stats, lambda n, c: n >= 4)
    record('none', 9103, [4, 5, 4, 3], [], model, sd, stats, lambda n, c: n == 0)
    record('one', 9104, [4, 5, 0, 4], [((0, 1), (3, 2))], model, sd, stats, lambda n, c: n == 1)
    # one source edge copied onto two other panels: an edge claimed by several positives
    record('claimed', 9105, [6, 6, 5, 6, 4], [((0, 2), (1, 3)), ((0, 2), (3, 1)), ((2, 0), (4, 2))], model, sd, stats,
           lambda n, c: n >= 3 and c >= 2)
    full = [14] * 23
    record('full', 9106, full, spread_plants(rng, full, 40), model, sd, stats, lambda n, c: n >= 20)

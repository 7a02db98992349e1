#!/usr/bin/env python3
"""Generates tests/golden/stitch_sample_small.pt: how the REFERENCE'S OWN training-pair draw distributes its decisions —
NNSewingPattern.stitches_as_3D_pairs and _3D_edges_per_panel (nn/data/pattern_converter.py:321-409, 517-552), called unbound and
unmodified on a small stand-in object that supplies panel_order(), `pattern` (panels with 3D vertices, edges with endpoints and
curvature, rotation, translation; stitches), `name` and a _point_in_3D that returns the vertex unchanged.

Only runnable where the reference checkout exists (like scripts/make_stitch_pairs_golden.py, whose sys.path set-up on the read-only
stubs it shares).  Two names are set at run time, in this script: `rotation_tools.euler_xyz_to_R` on the stub module (its result
only reaches the stand-in's _point_in_3D), and the module global `default_rng` of the reference's pattern_converter, replaced by a
recorder that hands every call on to a fresh UNSEEDED numpy generator and keeps the last permutation drawn: with it the output rows
are put back into their pre-shuffle order, so duplicates and non-stitched rows are told apart by position.

Garment: the `small` case of tests/golden/stitch_pairs_small.pt (edges, num_edges, plants as stitches).  Settings (6, 10), both
shuffles on, N = 2000 calls: the rarest category, a non-stitched ordered pair between two 6-edge panels, has probability
(1 / 36) / 23.5 = 1.2e-3 per row, so 10 N rows expect 23.6 hits.  Every row half is mapped back to (edge id, flipped) by exact value
match.  The fixture holds counts only.  The reference's generator cannot be seeded, so a run is kept only if every chi-square
statistic against the analytic model (tests/stitch_sample_restate.py model / chi2_statistics) lies under its 0.99 quantile;
otherwise all N calls are drawn again.  The tests hold the stored counts to the 0.9999 quantile.

    python scripts/make_stitch_sample_golden.py [REFERENCE_DIR]
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('GPE_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(REPO, 'oracle', 'refgen', 'stubs'), os.path.join(REF, 'nn'), REPO, os.path.join(REPO, 'tests')]

import data.pattern_converter as ref_converter  # noqa: E402  (the reference's module)
from data.pattern_converter import NNSewingPattern  # noqa: E402  (the reference's class)
from pattern import rotation as rotation_stub  # noqa: E402
import stitch_sample_restate as R  # noqa: E402

GOLDEN = os.path.join(REPO, 'tests', 'golden')
N_STITCHED, N_NON, CALLS = 6, 10, 2000
LAST = {}


class RecordingRng:
    """an unseeded numpy generator that remembers the last permutation it drew"""

    def __init__(self):
        self.rng = np.random.default_rng()

    def integers(self, *a, **kw):
        return self.rng.integers(*a, **kw)

    def permutation(self, n):
        LAST['perm'] = self.rng.permutation(n)
        return LAST['perm']


rotation_stub.euler_xyz_to_R = lambda angles: None
ref_converter.default_rng = RecordingRng


class StandIn:
    """what the reference's two functions read from a pattern, and the functions themselves, unmodified"""
    stitches_as_3D_pairs = NNSewingPattern.stitches_as_3D_pairs
    _3D_edges_per_panel = NNSewingPattern._3D_edges_per_panel

    def __init__(self, edges, num_edges, plants):
        self.name = 'stand_in'
        self._order = ['p%02d' % p for p, n in enumerate(num_edges) if n > 0]
        panels = {}
        for p, n in enumerate(num_edges):
            if n == 0:
                continue
            e = edges[p, :int(n)].astype(np.float64)
            panels['p%02d' % p] = {
                'vertices': [v.tolist() for l in range(int(n)) for v in (e[l, 0:3], e[l, 3:6])],        # already 3D
                'edges': [{'endpoints': [2 * l, 2 * l + 1], 'curvature': e[l, 6:8].tolist()} for l in range(int(n))],
                'rotation': [0.0, 0.0, 0.0], 'translation': [0.0, 0.0, 0.0]}
        self.pattern = {'panels': panels,
                        'stitches': [[{'panel': 'p%02d' % a[0], 'edge': a[1]}, {'panel': 'p%02d' % b[0], 'edge': b[1]}] for a, b in plants]}

    def panel_order(self, force_update=False, pad_to_len=None):
        return self._order

    def _point_in_3D(self, point, rotation, translation):
        return point


def main():
    fx = torch.load(os.path.join(GOLDEN, 'stitch_pairs_small.pt'), weights_only=False)
    edges, num_edges = fx['edges'].numpy(), fx['num_edges'].numpy()
    P, L, Fe = edges.shape
    E, Rn = P * L, N_STITCHED + N_NON
    stitches = [(a[0] * L + a[1], b[0] * L + b[1]) for a, b in fx['plants']]
    Sv = len(stitches)
    # every edge as a row half can carry it, in the reference's float64: as stored and reversed
    lookup = {}
    for p, n in enumerate(num_edges):
        for l in range(int(n)):
            e = edges[p, l].astype(np.float64)
            for flip, v in ((0, e), (1, R.flipped(e))):
                assert tuple(v) not in lookup
                lookup[tuple(v)] = (p * L + l, flip)
    obj = StandIn(edges, num_edges, [(tuple(a), tuple(b)) for a, b in fx['plants']])
    for run in range(1, 100):
        rec = {'N': CALLS, 'flip_seen': np.zeros(E, dtype=np.int64), 'flip_count': np.zeros(E, dtype=np.int64),
               'swap_count': np.zeros(Sv, dtype=np.int64), 'choice_hist': np.zeros(Sv, dtype=np.int64),
               'perm_counts': np.zeros((Rn, Rn), dtype=np.int64), 'flip_inconsistent': 0}
        pair_counts = {}
        for _ in range(CALLS):
            rows, mask = obj.stitches_as_3D_pairs(N_STITCHED, N_NON, True, True)        # ---- the reference, unmodified ----
            perm = LAST['perm']                                 # output row i is pre-shuffle row perm[i]
            assert rows.shape == (Rn, 2 * Fe) and mask.sum() == N_STITCHED
            pre, pre_mask = np.empty_like(rows), np.empty_like(mask)
            pre[perm], pre_mask[perm] = rows, mask
            assert pre_mask[:N_STITCHED].all() and not pre_mask[N_STITCHED:].any()
            rec['perm_counts'][perm, np.arange(Rn)] += 1
            halves = [(lookup[tuple(r[:Fe])], lookup[tuple(r[Fe:])]) for r in pre]
            state = {}
            for h in halves:
                for e, f in h:
                    state.setdefault(e, set()).add(f)
            rec['flip_inconsistent'] += sum(1 for v in state.values() if len(v) > 1)
            for e, v in state.items():
                rec['flip_seen'][e] += 1
                rec['flip_count'][e] += max(v)
            for k, (a, b) in enumerate(stitches):
                got = (halves[k][0][0], halves[k][1][0])
                assert got in ((a, b), (b, a))
                rec['swap_count'][k] += got == (b, a)
            for r in range(Sv, N_STITCHED):
                same = [k for k in range(Sv) if np.array_equal(pre[k], pre[r])]
                assert len(same) == 1
                rec['choice_hist'][same[0]] += 1
            for r in range(N_STITCHED, Rn):
                q = (halves[r][0][0], halves[r][1][0])
                pair_counts[q] = pair_counts.get(q, 0) + 1
        rec['pair_counts'] = np.asarray([(a, b, c) for (a, b), c in sorted(pair_counts.items())], dtype=np.int64)
        stats = R.chi2_statistics(rec, num_edges, L, stitches, N_STITCHED, N_NON)
        ok = rec['flip_inconsistent'] == 0
        for k, (x, df) in stats.items():
            q = R.chi2_quantile(df, 0.99)
            ok = ok and x < q
            print('run %d  %-8s chi-square %9.2f on %3d degrees of freedom (0.99 quantile %9.2f, 0.9999 quantile %9.2f)'
                  % (run, k, x, df, q, R.chi2_quantile(df, 0.9999)))
        if ok:
            break
    else:
        raise RuntimeError('no run under the 0.99 quantiles')
    out = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else int(v)) for k, v in rec.items()}
    out.update(garment='stitch_pairs_small.pt', n_stitched=N_STITCHED, n_non_stitched=N_NON, runs=run,
               stitches=torch.tensor(stitches, dtype=torch.int64))
    path = os.path.join(GOLDEN, 'stitch_sample_small.pt')
    torch.save(out, path)
    print('stitch_sample_small: N = %d calls, %d distinct non-stitched pairs of %d possible, flips inconsistent within a call: %d, '
          '%.0f KB' % (CALLS, len(pair_counts), len(R.model(num_edges, L, stitches)), rec['flip_inconsistent'], os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Generates tests/golden/fit_stats_small.pt: the REFERENCE'S OWN standardisation statistics on small inputs —
GarmentBaseDataset._get_distribution_stats, _get_norm_stats and _unpad (nn/data/datasets.py:524-568) and the two standardize methods
(Garment3DPatternFullDataset.standardize :596-654, GarmentStitchPairsDataset.standardize :1018-1048), called unbound and unmodified
on a stand-in object with `.config = {}` and `.transforms = []`.

Only runnable where the reference checkout exists (like scripts/make_stitch_sample_golden.py, whose sys.path set-up on the read-only
stubs it shares).  Garment3DPatternFullDataset.standardize fills config['standardize'] and then builds its transforms, which fails
on `np.int` with a current numpy: that AttributeError is caught and the config it has already filled is taken.

The cases are chosen so that the reference alone decides them, away from its own thresholds:
  padded    [3, 4, 6, 4] edge rows: whole empty panels, a zero row in the middle of a loop, a row of magnitude 5e-6 (dropped by
            _unpad) beside one of 2e-5 (kept); statistics with padded=True
  columns   [2, 50, 6]: a constant non-zero column (scale = tmin, std 0), an all-zero column (scale 1), a column whose extremes
            differ by 1e-6 relative (scale = tmin), a negative constant column (negative scale), two ordinary columns
  pattern   one full Garment3DPatternFullDataset.standardize over 5 garments (600 feature rows)
  stitch    one full GarmentStitchPairsDataset.standardize over 5 garments (60 pair rows)
The fixture holds the inputs, the reference's fp32 outputs, and for mean / std the distance from the float64 restatement
(tests/fit_stats_restate.py) the generator actually saw next to the bound n 2^-23 max|x| the tests hold it to.

    python scripts/make_fit_stats_golden.py [REFERENCE_DIR]
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('GPE_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(REPO, 'oracle', 'refgen', 'stubs'), os.path.join(REF, 'nn'), REPO, os.path.join(REPO, 'tests')]

from data.datasets import GarmentBaseDataset, Garment3DPatternFullDataset, GarmentStitchPairsDataset  # noqa: E402  (the reference)
import fit_stats_restate as R  # noqa: E402

GOLDEN = os.path.join(REPO, 'tests', 'golden')


class StandIn:
    """what the reference's functions read from a data set, and the functions themselves, unmodified"""
    _unpad = GarmentBaseDataset._unpad
    _get_distribution_stats = GarmentBaseDataset._get_distribution_stats
    _get_norm_stats = GarmentBaseDataset._get_norm_stats
    standardize_pattern = Garment3DPatternFullDataset.standardize
    standardize_stitch = GarmentStitchPairsDataset.standardize

    def __init__(self):
        self.config = {}
        self.transforms = []


def padded_outlines(rng, G, P, L):
    """edge rows [G, P, L, 4] with trailing padding rows, empty panels and (garment 0) the three special rows"""
    x = np.zeros((G, P, L, 4), dtype=np.float32)
    for g in range(G):
        for p in range(P):
            n = 0 if (g + p) % 4 == 3 else int(rng.integers(3, L + 1))
            x[g, p, :n] = rng.normal(0, 20, (n, 4)).astype(np.float32) * np.asarray([1, 1, 0.01, 0.01], dtype=np.float32)
    x[0, 0, :3] = rng.normal(0, 20, (3, 4)).astype(np.float32)
    x[0, 0, 1] = 0                                                  # a zero row in the middle of a loop: dropped
    x[0, 1, :3] = rng.normal(0, 20, (3, 4)).astype(np.float32)
    x[0, 1, 0] = np.asarray([5e-6, -5e-6, 5e-6, 0], dtype=np.float32)       # under the tolerance in every column: dropped
    x[0, 1, 1] = np.asarray([2e-5, 0, 0, 0], dtype=np.float32)              # one column over it: kept
    return x


def seen(ref, want, bound):
    """{'ref': fp32 tensor, 'seen': the distance from the float64 restatement, 'bound'}; the generator refuses a miss"""
    d = np.abs(ref.astype(np.float64) - want)
    assert (d <= bound).all(), (d, bound)
    return {'ref': torch.from_numpy(ref), 'seen': torch.from_numpy(d), 'bound': torch.from_numpy(np.asarray(bound))}


def case(obj, x, padded):
    t = torch.from_numpy(x)
    mean, std = obj._get_distribution_stats(t, padded=padded)          # ---- the reference, unmodified ----
    mn, scale = obj._get_norm_stats(t, padded=padded)
    w, bound = R.all_stats(x, padded), R.sum_bound(x, padded)
    assert np.array_equal(mn.numpy(), R.f32(w['min'])) and np.array_equal(scale.numpy(), R.f32(w['norm_scale']))
    return {'x': t, 'padded': padded, 'n': int(obj._unpad(t.view(-1, t.shape[-1])).shape[0]) if padded else int(t.numel() // t.shape[-1]),
            'mean': seen(mean.numpy(), w['mean'], bound), 'std': seen(std.numpy(), w['std'], bound),
            'min': mn, 'norm_scale': scale}


def main():
    rng = np.random.default_rng(20240607)
    obj = StandIn()
    out = {'cases': {}}
    out['cases']['padded'] = case(obj, padded_outlines(rng, 3, 4, 6), True)
    cols = rng.normal(0, 3, (2, 50, 6)).astype(np.float32)
    cols[..., 0] = 0.75
    cols[..., 1] = 0
    cols[..., 2] = np.where(rng.random((2, 50)) < 0.5, np.float32(1.0), np.float32(1.000001))
    cols[..., 3] = -2.5
    cols[..., 5] += 40
    out['cases']['columns'] = case(obj, cols, False)
    assert out['cases']['columns']['norm_scale'].tolist()[:4] == [0.75, 1.0, 1.0, -2.5]
    assert out['cases']['padded']['n'] < 3 * 4 * 6 - 2

    # one full standardize of each data set class
    G, N, P, L = 5, 120, 4, 6
    gt = {'outlines': padded_outlines(rng, G, P, L),
          'rotations': rng.uniform(-1, 1, (G, P, 4)).astype(np.float32),
          'translations': rng.normal(0, 30, (G, P, 3)).astype(np.float32),
          'stitch_tags': rng.normal(0, 25, (G, P, L, 3)).astype(np.float32)}
    gt['rotations'][:, 3] = 0                                        # an empty panel's placement is zero, a valid value here
    gt['translations'][:, 3] = 0
    feats = (rng.normal(0, 1, (G, N, 3)) * [25, 40, 12] + [0, 110, 3]).astype(np.float32)
    training = [{'features': torch.from_numpy(feats[g]), 'ground_truth': {k: torch.from_numpy(v[g]) for k, v in gt.items()}}
                for g in range(G)]
    obj = StandIn()
    try:
        obj.standardize_pattern(training)                              # ---- the reference, unmodified ----
    except AttributeError as e:
        print('Garment3DPatternFullDataset.standardize filled the config, then: %s' % e)
    ref, want = obj.config['standardize'], R.pattern_standardize(feats, gt)
    pat = {'features': torch.from_numpy(feats), 'gt': {k: torch.from_numpy(v) for k, v in gt.items()},
           'f_shift': seen(ref['f_shift'], want['f_shift'], R.sum_bound(feats)),
           'f_scale': seen(ref['f_scale'], want['f_scale'], R.sum_bound(feats)),
           'gt_shift': {'outlines': seen(ref['gt_shift']['outlines'], want['gt_shift']['outlines'], R.sum_bound(gt['outlines'], True))},
           'gt_scale': {'outlines': seen(ref['gt_scale']['outlines'], want['gt_scale']['outlines'], R.sum_bound(gt['outlines'], True))}}
    for k in ('rotations', 'translations', 'stitch_tags'):
        for side in ('gt_shift', 'gt_scale'):
            assert ref[side][k].dtype == np.float32 and np.array_equal(ref[side][k], R.f32(want[side][k])), (side, k)
            pat[side][k] = torch.from_numpy(ref[side][k])
    assert pat['gt_shift']['outlines']['ref'].tolist()[:2] == [0.0, 0.0]
    out['pattern'] = pat

    rows = rng.normal(0, 30, (G, 12, 16)).astype(np.float32)
    rows[..., 6:8] = rng.uniform(0, 1, (G, 12, 2)).astype(np.float32)
    obj = StandIn()
    try:
        obj.standardize_stitch([{'features': torch.from_numpy(rows[g]), 'ground_truth': torch.zeros(12, dtype=torch.bool)} for g in range(G)])
    except AttributeError as e:
        print('GarmentStitchPairsDataset.standardize filled the config, then: %s' % e)
    ref, want = obj.config['standardize'], R.stitch_standardize(rows)
    for k in ('f_shift', 'f_scale'):
        assert ref[k].dtype == np.float32 and np.array_equal(ref[k], R.f32(want[k])), k
    out['stitch'] = {'features': torch.from_numpy(rows), 'f_shift': torch.from_numpy(ref['f_shift']), 'f_scale': torch.from_numpy(ref['f_scale'])}

    path = os.path.join(GOLDEN, 'fit_stats_small.pt')
    torch.save(out, path)
    for name, c in out['cases'].items():
        print('%-8s n = %4d  max |mean - restatement| = %.3e, |std - restatement| = %.3e (least bound %.3e)'
              % (name, c['n'], float(c['mean']['seen'].max()), float(c['std']['seen'].max()), float(c['mean']['bound'].min())))
    print('fit_stats_small: %.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()

"""not-gpu: the fp64 restatement of the quality metrics (tests/quality_restate.py) against the reference's own numbers in
tests/golden/quality_*.pt, and the argument checks of the quality entry points (include/gpe_hip.h) without a GPU."""
import glob
import math
import os

import pytest
import torch

from gpe_amd import _lib, ops

import quality_restate

FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'quality_*.pt')))
QKEYS = set(ops.QUALITY_KEYS)


def test_fixtures_exist():
    names = {os.path.basename(f) for f in FIXTURES}
    for tag in ('lstm_e40', 'lstm_e0', 'att', 'matching', 'explicit_tags', 'no_correct', 'full'):
        assert 'quality_%s.pt' % tag in names


@pytest.mark.parametrize('path', FIXTURES, ids=[os.path.basename(f)[8:-3] for f in FIXTURES])
def test_restatement_reproduces_reference(path):
    fx = torch.load(path, weights_only=False)
    lc, dc = fx['loss_config'], fx['data_config']
    got, margin = quality_restate.restate(lc['quality_components'], fx['epoch'], lc['epoch_with_stitches'], dc['standardize'],
                                          dc['explicit_stitch_tags'], fx['preds'], fx['gt_matched'])
    assert margin >= quality_restate.MARGIN
    ref = {k: v for k, v in fx['loss_dict'].items() if k in QKEYS}
    assert set(got) == set(ref)
    for k, v in ref.items():
        if v is None:
            assert got[k] is None, k
        elif math.isnan(v):
            assert math.isnan(got[k]), k
        else:
            assert got[k] == pytest.approx(v, rel=1e-5, abs=1e-7), (k, got[k], v)


def test_fixtures_cover_the_corner_cases():
    seen_none = seen_nan = False
    for path in FIXTURES:
        fx = torch.load(path, weights_only=False)
        d = fx['loss_dict']
        seen_none |= any(d.get(k, 0) is None for k in QKEYS)
        seen_nan |= d.get('corr_num_edges_accuracy') is not None and math.isnan(d['corr_num_edges_accuracy'])
    assert seen_none and seen_nan
    full = torch.load(os.path.join(os.path.dirname(FIXTURES[0]), 'quality_full.pt'), weights_only=False)
    assert tuple(full['preds']['outlines'].shape[:3]) == (32, 23, 14) and int(full['gt']['num_stitches'].max()) == 24


def test_quality_entry_points_reject_bad_arguments_without_a_gpu():
    l = _lib.lib()
    stats = ops.quality_stats({'shift': [0, 0, 0.1, 0.1], 'scale': [25, 30, 0.3, 0.2]})
    # NULL workspace / outlines / stats, bad dimensions, unknown flags: -EINVAL before any launch
    assert l.gpe_quality_panels(None, 0, 0, 0, None, None, None, None, 0, None, 0, None, 0, None, 0, 1, 23, 14, 1, stats,
                                None, None) == -22
    assert l.gpe_quality_panels(None, 0, 0, 0, None, None, None, None, 0, None, 0, None, 0, None, 0, 0, 23, 14, 0, stats,
                                None, None) == -22
    assert l.gpe_quality_panels(None, 0, 0, 0, None, None, None, None, 0, None, 0, None, 0, None, 0, 2, 65, 14, 0, stats,
                                None, None) == -22
    assert l.gpe_quality_stitches(None, 0, 0, 0, 3, None, 0, 0, 0, None, None, 24, None, 2, 23, 14, 16, stats, None,
                                  None) == -22
    assert l.gpe_quality_stitches(None, 0, 0, 0, 3, None, 0, 0, 0, None, None, 24, None, 2, 64, 17, 32, stats, None,
                                  None) == -22
    assert l.gpe_quality_stitches(None, 0, 0, 0, 3, None, 0, 0, 0, None, None, 24, None, 2, 23, 14, 16, None, None,
                                  None) == -22
    assert l.gpe_quality_finalize(None, 2, 23, 14, 1, None, None, None) == -22
    assert l.gpe_quality_finalize(None, 0, 23, 14, 1, None, None, None) == -22


def test_quality_stats_layout():
    import numpy as np
    st = ops.quality_stats({'shift': [0, 0, 0.14890235662460327, 0.05642016604542732],
                            'scale': [25.267892837524418, 31.298505783081055, 0.2677369713783264, 0.2352069765329361]},
                           rot_stats={'shift': [1, 2, 3, 4], 'scale': [5, 6, 7, 8]},
                           tag_stats={'shift': [-1, -2, -3], 'scale': [2, 3, 4]})
    v = np.array(list(st), np.float32)
    pad = -torch.tensor([0, 0, 0.14890235662460327, 0.05642016604542732]) / \
        torch.tensor([25.267892837524418, 31.298505783081055, 0.2677369713783264, 0.2352069765329361])
    assert (v[8:12] == pad.numpy()).all()
    # the kernel's padding test |x - pad| <= tol decides like torch.isclose(x, pad, atol=0.07) on floats around the bound
    tol = torch.tensor(v[12:16])
    x = pad + tol
    xs = [x]
    for _ in range(64):
        xs.append(torch.nextafter(xs[-1], xs[-1] + 1))
        xs.insert(0, torch.nextafter(xs[0], xs[0] - 1))
    xs = torch.stack(xs)
    assert torch.equal((xs - pad).abs() <= tol, torch.isclose(xs, pad.expand_as(xs), atol=0.07))
    assert (v[24:28] == [1, 2, 3, 4]).all() and (v[32:36] == [5, 6, 7, 8]).all()
    assert (v[56:59] == [-1, -2, -3]).all() and (v[64:67] == [2, 3, 4]).all()

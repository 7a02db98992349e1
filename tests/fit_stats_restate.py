"""The reference's standardisation statistics restated in numpy float64 (nn/data/datasets.py:524-568, 596-645, 1018-1041), for the
tests of the device fit (csrc/gpe_fit_stats.hip, ops.FitAccumulator, staging.fit_*):

  unpad                 _unpad: a row is padding iff isclose(x, 0, atol=1e-5) in every column, i.e. |x| <= 1e-5 (the rtol term vanishes
                        against 0); decided on the fp32 values
  distribution_stats    _get_distribution_stats: two-pass mean and POPULATION std over the rows kept
  norm_stats            _get_norm_stats: min (max) with -0 < +0, and the scale rule of :562-566 (torch.isclose defaults rtol=1e-5, atol=1e-8) on the
                        fp32 extremes, evaluated in float64
  pattern_standardize   Garment3DPatternFullDataset.standardize's config['standardize']
  stitch_standardize    GarmentStitchPairsDataset.standardize's

Inputs are fp32 arrays; everything is computed in float64 and returned as float64 (round once with f32())."""
import numpy as np


def f32(v):
    """the one rounding to the reference's result precision"""
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(v, dtype=np.float64).astype(np.float32)


def rows(x):
    x = np.asarray(x)
    assert x.dtype == np.float32
    return x.reshape(-1, x.shape[-1])


def unpad(x, tolerance=1e-5):
    r = rows(x)
    keep = ~np.all(np.abs(r) <= np.float32(tolerance), axis=1)
    return r[keep]


def distribution_stats(x, padded=False):
    """-> (n, mean, std): float64 two-pass over the rows kept"""
    r = (unpad(x) if padded else rows(x)).astype(np.float64)
    n = r.shape[0]
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = r.sum(axis=0) / n
        std = np.sqrt(((r - mean) ** 2).sum(axis=0) / n)
    return n, mean, std


def scale_rule(tmin, tmax):
    """:562-566 on one column's fp32 extremes"""
    tmin, tmax = float(np.float32(tmin)), float(np.float32(tmax))
    if abs(tmin - tmax) <= 1e-8 + 1e-5 * abs(tmax):
        return 1.0 if abs(tmin) <= 1e-8 else tmin
    return tmax - tmin


def norm_stats(x, padded=False):
    """-> (n, min, max, scale); a NaN in a column makes its extremes NaN, as torch.min / torch.max"""
    r = (unpad(x) if padded else rows(x)).astype(np.float64)
    with np.errstate(invalid='ignore'):
        mn, mx = r.min(axis=0), r.max(axis=0)
    # IEEE 754-2019 minimum / maximum: -0 < +0 (numpy leaves the sign of a zero extreme to the order of the rows)
    neg = np.signbit(r)
    mn = np.where((mn == 0) & neg.any(axis=0), -0.0, np.where(mn == 0, 0.0, mn))
    mx = np.where((mx == 0) & (~neg).any(axis=0), 0.0, np.where(mx == 0, -0.0, mx))
    with np.errstate(invalid='ignore'):
        scale = np.asarray([scale_rule(a, b) for a, b in zip(mn, mx)], dtype=np.float64)
    return r.shape[0], mn, mx, scale


def all_stats(x, padded=False):
    """everything the device's result block holds, in float64: {'n', 'mean', 'std', 'min', 'max', 'norm_scale'}"""
    n, mean, std = distribution_stats(x, padded)
    _, mn, mx, scale = norm_stats(x, padded)
    return {'n': n, 'mean': mean, 'std': std, 'min': mn, 'max': mx, 'norm_scale': scale}


def pattern_standardize(features, gt):
    """config['standardize'] of Garment3DPatternFullDataset.standardize (:612-645) in float64"""
    _, f_shift, f_scale = distribution_stats(features)
    _, p_shift, p_scale = distribution_stats(gt['outlines'], padded=True)
    p_shift = p_shift.copy()
    p_shift[0] = p_shift[1] = 0
    out = {'f_shift': f_shift, 'f_scale': f_scale, 'gt_shift': {'outlines': p_shift}, 'gt_scale': {'outlines': p_scale}}
    for k in ('rotations', 'translations', 'stitch_tags'):
        _, mn, _, scale = norm_stats(gt[k])
        out['gt_shift'][k], out['gt_scale'][k] = mn, scale
    return out


def stitch_standardize(features):
    """config['standardize'] of GarmentStitchPairsDataset.standardize (:1034-1040) in float64"""
    _, mn, _, scale = norm_stats(features)
    return {'f_shift': mn, 'f_scale': scale}


def sum_bound(x, padded=False):
    """n 2^-23 max|x| per column: the worst case of an fp32 sum of n terms (n 2^-24 max|x|), doubled for the reference's two passes"""
    r = (unpad(x) if padded else rows(x)).astype(np.float64)
    return r.shape[0] * 2.0 ** -23 * np.abs(r).max(axis=0)


def ulp32(v):
    """the spacing of fp32 at |v| (per element)"""
    v = np.abs(np.asarray(v, dtype=np.float32))
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)

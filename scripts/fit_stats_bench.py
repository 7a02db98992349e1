#!/usr/bin/env python3
"""What fitting the standardisation statistics on the device costs and what it replaces.  The resident set is `--garments` synthetic
garments (a bent `--side` x `--side` grid each) and their ground-truth tensors at the data set's shapes ([G, 23, 14, 4] outlines with
trailing padding, [G, 23, 4] rotations, [G, 23, 3] translations, [G, 23, 14, 3] stitch tags).  One process, wall clock around work
that ends in a device synchronise, `--warmup` runs first, best of `--rounds`:

  device_fit      staging.MeshPointSampler.fit_feature_stats(index, chunk=`--chunk`): draw one cloud of `--points` points per garment
                  and accumulate, with its two host reads
  device_gt       staging.fit_pattern_standardization on the resident ground truth
  host_stats      the reference's formulas (_get_distribution_stats / _get_norm_stats / _unpad, nn/data/datasets.py:524-568) in torch on
                  the host over the SAME clouds and ground truth, already collated: a lower bound on what the fit replaces — the
                  reference also samples every cloud on the host first (igl) and collates them

and, from device events around `--reps` back-to-back launches, the kernels alone on `--bw-garments` clouds (a tensor larger than
the 256 MiB memory-side cache, so the reads come from HBM):

  fit_part_us     gpe_fit_part over [bw_garments, points, 3]; fit_part_gbs = the tensor's bytes over that time, hbm_share = its share
                  of the 8 TB/s the HBM is specified at
  fit_finish_us   gpe_fit_finish over its records

One JSON line.

    python scripts/fit_stats_bench.py [--garments 4096] [--points 2000] [--chunk 256] [--side 40] [--bw-garments 16384] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

HBM_PEAK = 8.0e12           # bytes / s, the specified rate


def synthetic_set(G, side, seed=0):
    """-> [(verts fp32 [side^2, 3], faces int32, labels int32)]: a grid bent and scaled differently per garment, in centimetres"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(0, 1, side), np.linspace(0, 1, side), indexing='ij')
    idx = np.arange(side * side).reshape(side, side)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]).astype(np.int32)
    labels = ((np.arange(side)[:, None] * 3 // side) * 3 + np.arange(side)[None, :] * 3 // side).ravel().astype(np.int32)
    out = []
    for g in range(G):
        bend, sx, sz = rng.uniform(1.0, 5.0), rng.uniform(20, 40), rng.uniform(30, 60)
        r = 0.4 + 0.6 * u
        verts = np.stack([sx * np.cos(bend * u) * r, 100 + sx * np.sin(bend * u) * r, sz * (2 * v - 1) + 0.1 * u], axis=-1).reshape(-1, 3)
        out.append((verts.astype(np.float32), faces, labels))
    return out


def synthetic_gt(G, seed=1, P=23, L=14):
    rng = np.random.default_rng(seed)
    n = rng.integers(0, L + 1, (G, P))
    n[rng.random((G, P)) < 0.6] = 0                                # most panel slots of a garment are empty
    live = (np.arange(L)[None, None, :] < n[:, :, None])
    ol = (rng.normal(0, 20, (G, P, L, 4)) * [1, 1, 0.01, 0.01]).astype(np.float32) * live[..., None]
    tags = rng.normal(0, 25, (G, P, L, 3)).astype(np.float32) * live[..., None]
    rot = rng.uniform(-1, 1, (G, P, 4)).astype(np.float32) * (n > 0)[..., None]
    tr = rng.normal(0, 30, (G, P, 3)).astype(np.float32) * (n > 0)[..., None]
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in
            (('outlines', ol), ('rotations', rot), ('translations', tr), ('stitch_tags', tags))}


def host_distribution(x, padded=False):
    """_get_distribution_stats (with _unpad) as the reference writes it"""
    x = x.view(-1, x.shape[-1])
    if padded:
        x = x[~torch.all(torch.isclose(x, torch.zeros_like(x), atol=1e-5), axis=1)]
    mean = x.mean(axis=0)
    return mean, torch.sqrt(((x - mean) ** 2).sum(0) / x.shape[0])


def host_norm(x):
    """_get_norm_stats as the reference writes it"""
    x = x.view(-1, x.shape[-1])
    mn, mx = torch.min(x, dim=0)[0], torch.max(x, dim=0)[0]
    scale = torch.empty_like(mn)
    for i, (a, b) in enumerate(zip(mn, mx)):
        scale[i] = (a if not torch.isclose(a, torch.zeros(1)) else 1.) if torch.isclose(a, b) else b - a
    return mn, scale


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def events(fn, reps):
    """microseconds per call from device events around `reps` back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--garments', type=int, default=4096)
    ap.add_argument('--points', type=int, default=2000)
    ap.add_argument('--chunk', type=int, default=256)
    ap.add_argument('--side', type=int, default=40)
    ap.add_argument('--bw-garments', type=int, default=16384)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('fit_stats_bench needs the MI355X: a timing taken elsewhere says nothing about it')
    from gpe_amd import ops, staging
    t0 = time.perf_counter()
    G, N = a.garments, a.points
    sampler = staging.MeshPointSampler(synthetic_set(G, a.side), None, mesh_samples=N)
    index = torch.arange(G, device='cuda')
    gt_host = synthetic_gt(G)
    gt = {k: v.cuda() for k, v in gt_host.items()}
    res = {'garments': G, 'points': N, 'chunk': a.chunk, 'setup_s': round(time.perf_counter() - t0, 1), 'ms': {}}

    # the clouds the host side computes on: the ones the fit draws (same seed and chunks), brought over once, outside the timing
    sampler.reseed(0, 0)
    clouds = torch.cat([sampler.sample(index[g0:g0 + a.chunk])[0].cpu() for g0 in range(0, G, a.chunk)])
    variants = {
        'device_fit': lambda: sampler.fit_feature_stats(index, seed=0, chunk=a.chunk, install=False),
        'device_gt': lambda: staging.fit_pattern_standardization(gt, {'f_shift': [0, 0, 0], 'f_scale': [1, 1, 1]}),
        'host_stats': lambda: (host_distribution(clouds), host_distribution(gt_host['outlines'], True), host_norm(gt_host['rotations']),
                               host_norm(gt_host['translations']), host_norm(gt_host['stitch_tags']))}
    out = {}
    for name, fn in variants.items():
        for _ in range(a.warmup):
            fn()
    for _ in range(a.rounds):                                    # alternating: drift of the clocks hits every variant alike
        for name, fn in variants.items():
            ms, out[name] = wall(fn)
            res['ms'].setdefault(name, []).append(round(ms, 3))
    res['best_ms'] = {k: min(v) for k, v in res['ms'].items()}
    res['spread_pct'] = {k: round(100.0 * (max(v) - min(v)) / min(v), 1) for k, v in res['ms'].items()}
    res['host_over_device'] = round(res['best_ms']['host_stats'] / (res['best_ms']['device_fit'] + res['best_ms']['device_gt']), 1)
    # the two sides computed the same thing
    res['max_abs_diff_vs_host'] = {
        'f_shift': float(np.abs(out['device_fit']['f_shift'] - out['host_stats'][0][0].numpy()).max()),
        'f_scale': float(np.abs(out['device_fit']['f_scale'] - out['host_stats'][0][1].numpy()).max()),
        'outlines_scale': float(np.abs(out['device_gt']['gt_scale']['outlines'] - out['host_stats'][1][1].numpy()).max()),
        'translations_scale': float(np.abs(out['device_gt']['gt_scale']['translations'] - out['host_stats'][3][1].numpy()).max())}

    # the kernels alone, on a tensor the memory-side cache cannot hold
    del clouds
    big = torch.randn(a.bw_garments, N, 3, device='cuda')
    part = torch.empty(ops.fit_leaves(a.bw_garments, N), 13, device='cuda', dtype=torch.float64)
    block = torch.empty(17, device='cuda', dtype=torch.float64)
    for _ in range(3):
        ops.fit_part(big, part)
        ops.fit_finish(part, out=block)
    nbytes = big.numel() * 4
    res['kernels'] = {'bw_garments': a.bw_garments, 'input_mb': round(nbytes / 2 ** 20, 1), 'leaves': part.shape[0], 'reps': a.reps}
    us = [events(lambda: ops.fit_part(big, part), a.reps) for _ in range(a.rounds)]
    res['kernels']['fit_part_us'] = [round(v, 1) for v in us]
    res['kernels']['fit_part_gbs'] = round(nbytes / (min(us) * 1e-6) / 1e9, 1)
    res['kernels']['hbm_share'] = round(nbytes / (min(us) * 1e-6) / HBM_PEAK, 3)
    us = [events(lambda: ops.fit_finish(part, out=block), a.reps) for _ in range(a.rounds)]
    res['kernels']['fit_finish_us'] = [round(v, 1) for v in us]
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""What drawing the model's clouds from resident raw scans costs and what it replaces.  The resident set is `--scans` synthetic scans
of `--points` points each (uniform in a box); a batch is `--batch` slots of `--samples` points.  One process, the variants
alternating, `--warmup` calls each first, then `--rounds` windows per variant:

  device     staging.ScanSampler.sample(index), eager: a memset and three launches (csrc/gpe_scan_sample.hip).  HIP events around a
             window of `--steps` calls, the device drained before the first; ms per call
  host_loop  the lines of the reference's nn/evaluation_scripts/predict_per_example.py that the call replaces, at the same shape:
             per scan np.random.permutation(n)[:samples], (p - f_shift) / f_scale, then torch.stack and the copy to the device.
             Wall clock around a window of `--host-steps` batches that ends in a device synchronise
  labels     ScanSampler.labels(att_weights) on the last sample with `--panels` weights per point: one launch, HIP events

Every call gets its own index tensor (a row of a resident table).  One JSON line: the windows of every variant in ms per call, the
median and the spread of each, and host_loop / device (medians).  No ratio is fixed in advance.

    python scripts/scan_sample_bench.py [--batch 32] [--points 200000] [--samples 2000] [--scans 32] [--steps 50] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]

STATS = {'f_shift': [0.05, 1.1, -0.02], 'f_scale': [0.6, 0.7, 0.3]}
VARIANTS = ('device', 'host_loop', 'labels')


class Bench:
    def __init__(self, a, seed=0):
        from gpe_amd import staging
        rng = np.random.default_rng(seed)
        self.a = a
        self.host = [rng.uniform(-1, 1, (a.points, 3)) for _ in range(a.scans)]      # float64, as load_points leaves them
        self.sampler = staging.ScanSampler(self.host, STATS, mesh_samples=a.samples, seed=seed + 1)
        self.index_host = rng.integers(0, a.scans, size=(64, a.batch)).astype(np.int32)
        self.index = torch.from_numpy(self.index_host).cuda()
        self.turn = 0
        self.att = torch.rand(a.batch, a.samples, a.panels, device='cuda')
        self.shift, self.scale = np.asarray(STATS['f_shift']), np.asarray(STATS['f_scale'])
        self.rs = np.random.RandomState(seed + 2)

    def call(self, name):
        self.turn = (self.turn + 1) % self.index.shape[0]
        if name == 'device':
            self.out = self.sampler.sample(self.index[self.turn])
        elif name == 'labels':
            self.lab = self.sampler.labels(self.att)
        else:
            clouds = []
            for g in self.index_host[self.turn]:
                points = self.host[g]
                if abs(points.shape[0] - self.a.samples) > 10:                        # predict_per_example.py:137-141
                    points = points[self.rs.permutation(points.shape[0])[:self.a.samples]]
                points = (points - self.shift) / self.scale                           # :143-144
                clouds.append(torch.tensor(points).float())                           # :145
            self.host_out = torch.stack(clouds).to('cuda')

    def window(self, name, calls):
        torch.cuda.synchronize()
        if name == 'host_loop':
            t0 = time.perf_counter()
            for _ in range(calls):
                self.call(name)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / calls
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            self.call(name)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--points', type=int, default=200000)
    ap.add_argument('--samples', type=int, default=2000)
    ap.add_argument('--scans', type=int, default=32)
    ap.add_argument('--panels', type=int, default=23)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--host-steps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('scan_sample_bench.py measures on the MI355X: no device found')
    t0 = time.perf_counter()
    bench = Bench(a)
    calls = {'device': a.steps, 'host_loop': a.host_steps, 'labels': max(a.steps // 10, 2)}
    res = {'shape': [a.batch, a.samples, 3], 'points_per_scan': a.points, 'resident_scans': a.scans, 'panels': a.panels,
           'calls_per_window': calls, 'setup_s': round(time.perf_counter() - t0, 1), 'ms_per_call': {}}
    for v in VARIANTS:
        bench.window(v, 1 if v == 'host_loop' else a.warmup)
    for _ in range(a.rounds):                                 # alternating: drift of the clocks hits every variant alike
        for v in VARIANTS:
            res['ms_per_call'].setdefault(v, []).append(round(bench.window(v, calls[v]), 4))
    status = bench.sampler.status
    res['status_of_last_call'] = {'repeated_rows': int(status.clamp(min=0).sum()), 'refused_slots': int((status < 0).sum())}
    med = {k: statistics.median(v) for k, v in res['ms_per_call'].items()}
    res['median_ms'] = {k: round(v, 4) for k, v in med.items()}
    res['spread_pct'] = {k: round(100.0 * (max(v) - min(v)) / min(v), 2) for k, v in res['ms_per_call'].items()}
    res['host_loop_over_device'] = round(med['host_loop'] / med['device'], 1)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""What feeding a captured training step from the device costs against handing it its inputs from the host.  The step is
GarmentFullPattern3D at `--batch` x `--points`, k = `--k` (defaults: BASELINE cfg 1, N = 1024, batch 8, k = 5), math f16x3 as
bench.py runs it, clouds drawn by a MeshPointSampler from `--garments` synthetic resident meshes (scripts/mesh_sample_bench.py),
ground truth of every garment from bench.synthetic.  One process, the two variants alternating, `--warmup` steps each first, then
`--rounds` windows of `--steps` steps (wall clock around a window, device drained at both ends):

  device_fed   staging.EpochFeeder inside the captured step: sg.step() without an argument; begin_epoch() at every epoch's start
               (counted in the window)
  host_fed     the same step the earlier way: sg.step(index, gt), the index a row of a host table, the ground truth of its garments
               gathered from host tensors (one indexing per tensor: cheaper than a DataLoader's collate) and staged by StepGraph

and, on its own, the schedule draw of one epoch at `--schedule-garments` garments in ten types and batches of `--schedule-batch`
(defaults 9678 and 30): windows of `--draws` draws.  One JSON line: milliseconds per step (all windows, median, spread), the
difference, and microseconds per draw.

    python scripts/epoch_feed_bench.py [--batch 8] [--points 1024] [--k 5] [--garments 256] [--steps 100] [--rounds 5] [--warmup 10]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests'), os.path.join(REPO, 'scripts')]

STATS = {'f_shift': [0.0, 0.0, 0.0], 'f_scale': [0.6, 0.6, 0.6]}
VARIANTS = ('device_fed', 'host_fed')


def ids_by_type(G, types, seed):
    """G garment ids dealt to `types` types of uneven sizes"""
    rng = np.random.default_rng(seed)
    cut = np.sort(rng.choice(np.arange(1, G), size=types - 1, replace=False))
    perm = rng.permutation(G)
    return {'type%d' % c: perm[a:b] for c, (a, b) in enumerate(zip(np.concatenate([[0], cut]), np.concatenate([cut, [G]])))}


class Bench:
    def __init__(self, a, total_steps, seed=0):
        import bench as flagship
        import gpe_amd
        import mesh_sample_bench
        from gpe_amd import configs, graph, nets, ops, optim, staging
        gpe_amd.set_math('f16x3')
        self.B, N, G = a.batch, a.points, a.garments
        resident = ops.mesh_resident(mesh_sample_bench.synthetic_set(G, seed))
        data_config = configs.data_config()
        nn_cfg = configs.lstm_model_config(k_neighbors=a.k)
        torch.manual_seed(seed)
        base = nets.GarmentFullPattern3D(data_config, dict(nn_cfg), dict(nn_cfg['loss'])).cuda().train()
        base.loss.with_quality_eval = False
        _, self.gt_host = flagship.synthetic(G, 1, data_config, seed=1000, device='cpu')
        self.gt_bytes_per_garment = sum(v[0].numel() * v.element_size() for v in self.gt_host.values())
        ids = ids_by_type(G, 4, seed + 3)
        self.sg, self.sched, self.turn = {}, {}, {v: 0 for v in VARIANTS}
        for name in VARIANTS:
            model = copy.deepcopy(base)
            opt = optim.FusedAdam(optim.FlatArena(model), lr=2e-3, schedule=optim.OneCycle(2e-3, total_steps))
            sampler = staging.MeshPointSampler(resident, STATS, mesh_samples=N, seed=seed + 1)
            self.sched[name] = staging.BalancedBatchSchedule(ids, self.B, seed=seed + 2)
            if name == 'device_fed':
                self.feeder = staging.EpochFeeder(self.sched[name], sampler, self.gt_host)
                fl = lambda model=model, f=self.feeder: model.loss(model(f.next()[0]), f.last_gt, epoch=0)[0]      # noqa: E731
            else:
                fl = lambda i, g, model=model, s=sampler: model.loss(model(s.sample(i)[0]), g, epoch=0)[0]         # noqa: E731
            self.sg[name] = graph.StepGraph(fl, opt, warmup=2)
        self.steps_per_epoch = len(self.feeder)

    def step(self, name):
        t = self.turn[name]
        self.turn[name] = t + 1
        if name == 'device_fed':
            if t % self.steps_per_epoch == 0:
                self.feeder.begin_epoch()
            return self.sg[name].step()
        if t % self.steps_per_epoch == 0:                       # the host's schedule: the device's table read back once per epoch
            self.sched[name].draw()
            self.rows = self.sched[name].host_table()
        row = self.rows[t % self.steps_per_epoch]
        pick = row.long()
        return self.sg[name].step(row, {k: v[pick] for k, v in self.gt_host.items()})

    def window(self, name, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step(name)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps


def schedule_windows(a):
    from gpe_amd import staging
    s = staging.BalancedBatchSchedule(ids_by_type(a.schedule_garments, 10, 7), a.schedule_batch, seed=1)
    out = []
    for r in range(a.rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.draws):
            s.draw()
        torch.cuda.synchronize()
        if r:                                                   # (the first window warms up)
            out.append(round((time.perf_counter() - t0) * 1e6 / a.draws, 2))
    return {'garments': a.schedule_garments, 'batch': a.schedule_batch, 'rows': len(s), 'quotas': s.quotas, 'draws_per_window': a.draws,
            'us_per_draw': out, 'median_us': statistics.median(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--garments', type=int, default=256)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--points', type=int, default=1024)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--schedule-garments', type=int, default=9678)
    ap.add_argument('--schedule-batch', type=int, default=30)
    ap.add_argument('--draws', type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('epoch_feed_bench needs the MI355X: nothing here is measured on a CPU')
    import gpe_amd
    t0 = time.perf_counter()
    bench = Bench(a, 2 * (a.warmup + a.rounds * a.steps) + 2)
    res = {'shape': [a.batch, a.points, 3], 'k': a.k, 'resident_garments': a.garments, 'steps_per_epoch': bench.steps_per_epoch,
           'gt_bytes_per_garment': bench.gt_bytes_per_garment, 'math': gpe_amd.get_math(), 'steps_per_window': a.steps,
           'setup_s': round(time.perf_counter() - t0, 1), 'ms_per_step': {}}
    for v in VARIANTS:
        bench.window(v, a.warmup)
    for _ in range(a.rounds):                                   # alternating: drift of the clocks hits both alike
        for v in VARIANTS:
            res['ms_per_step'].setdefault(v, []).append(round(bench.window(v, a.steps), 4))
    med = {k: statistics.median(v) for k, v in res['ms_per_step'].items()}
    res['median_ms'] = med
    res['spread_pct'] = {k: round(100.0 * (max(v) - min(v)) / min(v), 2) for k, v in res['ms_per_step'].items()}
    res['device_minus_host_ms'] = round(med['device_fed'] - med['host_fed'], 4)
    res['device_over_host_pct'] = round(100.0 * (med['device_fed'] - med['host_fed']) / med['host_fed'], 2)
    res['feeder_status'] = int(bench.feeder.status)
    res['schedule_draw'] = schedule_windows(a)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""What drawing the pattern model's input clouds on the device costs and what it replaces.  The resident set is `--garments`
synthetic garments of 10 000 vertices and 19 602 faces each (a bent 100 x 100 grid, nine panels, about 5 % stitch vertices, so the
re-label launch runs); the step is GarmentFullPattern3D at `--batch` x `--points`, k = `--k` (defaults: BASELINE cfg 1; cfg 2 is
--batch 32 --points 2048 --k 16), math f16x3 as bench.py runs it.  One process, the variants alternating, `--warmup` steps each
first, best of `--rounds` windows of `--steps` steps (wall clock around a window, device drained at both ends):

  sampler         staging.MeshPointSampler.sample(index) alone, eager: its launches and their host side
  step_fixed      graph.StepGraph over the training step on one fixed tensor of features (what bench.py --graph runs)
  step_sampled    the same captured step with the sampler inside: index in, fresh clouds every replay
  host_draw       tests/mesh_sample_restate.py drawing the same batch in numpy, plus the copy to the device: the stand-in for a host
                  loader (windows of `--host-steps` batches; the reference's own loader adds a Python loop per point)

Every step gets its own index tensor (a row of a resident table), as a training loop would hand one over.  One JSON line:
milliseconds per step, spread, step_sampled - step_fixed (the feature's cost inside the step) and host_draw / sampler.

    python scripts/mesh_sample_bench.py [--batch 8] [--points 1024] [--k 5] [--steps 100] [--rounds 3] [--warmup 10] [--host-steps 2]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

SIDE = 100
VARIANTS = ('sampler', 'step_fixed', 'step_sampled', 'host_draw')
STATS = {'f_shift': [0.0, 0.0, 0.0], 'f_scale': [0.6, 0.6, 0.6]}


def synthetic_set(G, seed=0):
    """-> [(verts fp32 [10000, 3], faces int32 [19602, 3], labels int32 [10000])]: a grid bent and scaled differently per garment"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(0, 1, SIDE), np.linspace(0, 1, SIDE), indexing='ij')
    idx = np.arange(SIDE * SIDE).reshape(SIDE, SIDE)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]).astype(np.int32)
    panel = ((np.arange(SIDE)[:, None] * 3 // SIDE) * 3 + np.arange(SIDE)[None, :] * 3 // SIDE).ravel()
    out = []
    for g in range(G):
        bend, sx, sz = rng.uniform(1.0, 5.0), rng.uniform(0.5, 1.0), rng.uniform(0.5, 1.0)
        r = 0.4 + 0.6 * u
        verts = np.stack([sx * np.cos(bend * u) * r, sx * np.sin(bend * u) * r, sz * (2 * v - 1) + 0.1 * u], axis=-1).reshape(-1, 3)
        labels = panel.copy()
        labels[rng.random(SIDE * SIDE) < 0.05] = -1
        out.append((verts.astype(np.float32), faces, labels.astype(np.int32)))
    return out


class Bench:
    def __init__(self, a, total_steps, seed=0):
        import bench as flagship
        import gpe_amd
        from gpe_amd import configs, graph, nets, ops, optim, staging
        gpe_amd.set_math('f16x3')
        self.B, self.N = a.batch, a.points
        self.host = synthetic_set(a.garments, seed)
        resident = ops.mesh_resident(self.host)
        self.resident_mb = sum(t.numel() * t.element_size() for t in (resident.verts4, resident.faces, resident.face_cdf)) / 2 ** 20
        self.sampler = {k: staging.MeshPointSampler(resident, STATS, mesh_samples=self.N, seed=seed + 1) for k in ('sampler', 'step_sampled')}
        self.index_host = np.random.default_rng(seed + 2).integers(0, a.garments, size=(64, self.B)).astype(np.int32)
        self.index = torch.from_numpy(self.index_host).cuda()
        self.turn = 0
        data_config = configs.data_config()
        nn_cfg = configs.lstm_model_config(k_neighbors=a.k)
        torch.manual_seed(seed)
        base = nets.GarmentFullPattern3D(data_config, dict(nn_cfg), dict(nn_cfg['loss'])).cuda().train()
        base.loss.with_quality_eval = False
        _, self.gt = flagship.synthetic(self.B, self.N, data_config, seed=1000, device=torch.device('cuda', 0))
        self.feats = self.sampler['sampler'].sample(self.index[0])[0].clone()
        self.sg = {}
        for name in ('step_fixed', 'step_sampled'):
            model = copy.deepcopy(base)
            opt = optim.FusedAdam(optim.FlatArena(model), lr=2e-3, schedule=optim.OneCycle(2e-3, total_steps))
            if name == 'step_fixed':
                fl = lambda f, g, model=model: model.loss(model(f), g, epoch=0)[0]
            else:
                fl = lambda i, g, model=model, s=self.sampler[name]: model.loss(model(s.sample(i)[0]), g, epoch=0)[0]
            self.sg[name] = graph.StepGraph(fl, opt, warmup=2)

    def next_index(self):
        self.turn = (self.turn + 1) % self.index.shape[0]
        return self.index[self.turn]

    def step(self, name):
        if name == 'sampler':
            self.sampler[name].sample(self.next_index())
        elif name == 'step_fixed':
            self.sg[name].step(self.feats, self.gt)
        elif name == 'step_sampled':
            self.sg[name].step(self.next_index(), self.gt)
        else:
            import mesh_sample_restate as R
            self.turn = (self.turn + 1) % self.index.shape[0]
            feats, seg, _, _ = R.sample_batch(self.host, self.index_host[self.turn].tolist(), self.N, 1, self.turn,
                                              shift=STATS['f_shift'], scale=STATS['f_scale'])
            self.host_out = (torch.from_numpy(feats).cuda(), torch.from_numpy(seg).cuda())

    def window(self, name, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step(name)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--garments', type=int, default=256)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--points', type=int, default=1024)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--host-steps', type=int, default=2)
    a = ap.parse_args()
    import gpe_amd
    t0 = time.perf_counter()
    bench = Bench(a, a.warmup + a.rounds * a.steps + 1)
    res = {'shape': [a.batch, a.points, 3], 'k': a.k, 'resident_garments': a.garments, 'resident_mb': round(bench.resident_mb, 1),
           'math': gpe_amd.get_math(), 'steps_per_window': a.steps, 'host_steps_per_window': a.host_steps,
           'setup_s': round(time.perf_counter() - t0, 1), 'ms_per_step': {}}
    for v in VARIANTS:
        bench.window(v, 1 if v == 'host_draw' else a.warmup)
    for _ in range(a.rounds):                                 # alternating: drift of the clocks hits every variant alike
        for v in VARIANTS:
            res['ms_per_step'].setdefault(v, []).append(round(bench.window(v, a.host_steps if v == 'host_draw' else a.steps), 4))
    status = bench.sampler['step_sampled'].status
    res['status_of_last_step'] = {'fell_back_points': int(status.clamp(min=0).sum()), 'refused_slots': int((status < 0).sum())}
    best = {k: min(v) for k, v in res['ms_per_step'].items()}
    res['best_ms'] = best
    res['spread_pct'] = {k: round(100.0 * (max(v) - min(v)) / min(v), 2) for k, v in res['ms_per_step'].items()}
    res['sampled_minus_fixed_ms'] = round(best['step_sampled'] - best['step_fixed'], 4)
    res['sampled_over_fixed_pct'] = round(100.0 * (best['step_sampled'] - best['step_fixed']) / best['step_fixed'], 2)
    res['garments_per_s'] = {k: round(a.batch * 1e3 / best[k], 1) for k in ('step_fixed', 'step_sampled')}
    res['host_over_sampler'] = round(best['host_draw'] / best['sampler'], 1)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""What drawing the stitch classifier's training pairs on the device costs and what it replaces, at the shipped training shape:
30 garments x (200 + 200) pair rows x 16 features per step, both shuffles on, drawn from 2000 resident synthetic garments
(23 panel slots x 14 edge slots, about 60 % of the panels present, 20 - 60 stitches each).  One process, the variants alternating,
`--warmup` steps each first, best of `--rounds` windows of `--steps` steps (wall clock around a window, device drained at both ends):

  sampler         staging.StitchPairSampler.sample(index) alone, eager: one launch and its host side
  sampler_graph   the same call captured once and replayed: the launch without the host side
  step_fixed      graph.StepGraph over a training step on one fixed tensor of rows (scripts/stitch_train_bench.py `captured`)
  step_sampled    the same captured step with the sampler inside: index in, fresh pairs every replay
  host_draw       tests/stitch_sample_restate.py drawing the same batch in numpy, plus the copy to the device: the stand-in for a host
                  loader (windows of `--host-steps` batches; the reference's own draw is a Python loop per row)

Every step gets its own index tensor (a row of a resident [*, 30] table), as a training loop would hand one over.  One JSON line:
milliseconds per step, spread, step_sampled - step_fixed (the feature's cost inside the step) and host_draw / sampler.

    python scripts/stitch_sample_bench.py [--steps 300] [--rounds 3] [--warmup 20] [--host-steps 5]
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

G, P, L, S = 2000, 23, 14, 60
B, N_ST, N_NON = 30, 200, 200
VARIANTS = ('sampler', 'sampler_graph', 'step_fixed', 'step_sampled', 'host_draw')


def synthetic_set(seed=0):
    """-> numpy edges fp32 [G, P, L, 8], num_edges [G, P], gt [G, 2, S], gt_num [G]: random edges in a 200 cm box, stitches between
    present edges of different panels"""
    rng = np.random.default_rng(seed)
    edges = rng.uniform(-100, 100, size=(G, P, L, 8)).astype(np.float32)
    edges[..., 6:] = np.where(rng.random((G, P, L, 1)) < 0.6, 0.0, rng.uniform(-0.5, 0.8, size=(G, P, L, 2))).astype(np.float32)
    ne = np.where(rng.random((G, P)) < 0.6, rng.integers(3, L + 1, size=(G, P)), 0).astype(np.int32)
    ne[:, 0], ne[:, 1] = np.maximum(ne[:, 0], 3), np.maximum(ne[:, 1], 3)          # at least two panels
    gt, num = np.zeros((G, 2, S), dtype=np.int32), rng.integers(20, S + 1, size=G).astype(np.int32)
    for g in range(G):
        present = np.nonzero(ne[g])[0]
        for s in range(num[g]):
            a, b = rng.choice(present, size=2, replace=False)
            gt[g, 0, s], gt[g, 1, s] = a * L + rng.integers(ne[g, a]), b * L + rng.integers(ne[g, b])
    return edges, ne, gt, num


class Bench:
    def __init__(self, total_steps, seed=0):
        import copy
        import gpe_amd
        from gpe_amd import graph, optim, staging
        self.host = synthetic_set(seed)
        self.stats = {'f_shift': [-100.0] * 6 + [0.0, -0.5] + [-100.0] * 6 + [0.0, -0.5], 'f_scale': [200.0] * 6 + [1.0, 1.3] + [200.0] * 6 + [1.0, 1.3]}
        dev = [torch.from_numpy(a).cuda() for a in self.host]
        self.sampler = {k: staging.StitchPairSampler(*dev, self.stats, N_ST, N_NON, True, True, seed=seed + 1)
                        for k in ('sampler', 'sampler_graph', 'step_sampled')}
        self.index_host = np.random.default_rng(seed + 2).integers(0, G, size=(64, B)).astype(np.int32)
        self.index = torch.from_numpy(self.index_host).cuda()
        self.turn = 0
        torch.manual_seed(seed)
        base = gpe_amd.nets.StitchOnEdge3DPairs({'element_size': 16}, {}, {}).cuda().train()
        self.rows, self.labels = self.sampler['sampler'].sample(self.index[0])
        self.rows, self.labels = self.rows.clone(), self.labels.clone()
        self.sg = {}
        for name in ('step_fixed', 'step_sampled'):
            model = copy.deepcopy(base)
            opt = optim.FusedAdam(optim.FlatArena(model), lr=2e-3, schedule=optim.OneCycle(2e-3, total_steps))
            if name == 'step_fixed':
                fl = lambda f, g, model=model: model.loss(model(f), g)[:2]
            else:
                fl = lambda i, model=model, s=self.sampler[name]: (lambda r, y: model.loss(model(r), y)[:2])(*s.sample(i))
            self.sg[name] = graph.StepGraph(fl, opt, warmup=2)
        self.cg = None

    def next_index(self):
        self.turn = (self.turn + 1) % self.index.shape[0]
        return self.index[self.turn]

    def step(self, name):
        if name == 'sampler':
            self.sampler[name].sample(self.next_index())
        elif name == 'sampler_graph':
            if self.cg is None:
                s = self.sampler[name]
                self.static_index = self.index[0].clone()
                s.sample(self.static_index)
                self.side = torch.cuda.Stream()
                self.side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(self.side):
                    self.cg = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.cg, stream=self.side):
                        self.static_out = s.sample(self.static_index)
                self.side.synchronize()
            with torch.cuda.stream(self.side):
                self.static_index.copy_(self.next_index(), non_blocking=True)
                self.cg.replay()
        elif name == 'step_fixed':
            self.sg[name].step(self.rows, self.labels)
        elif name == 'step_sampled':
            self.sg[name].step(self.next_index())
        else:
            import stitch_sample_restate as R
            self.turn = (self.turn + 1) % self.index.shape[0]
            rows, labels, _, _ = R.sample_batch(*self.host, self.index_host[self.turn].tolist(), N_ST, N_NON, 3, self.stats['f_shift'],
                                                self.stats['f_scale'], 1, self.turn)
            self.host_out = (torch.from_numpy(rows).cuda(), torch.from_numpy(labels).cuda())

    def window(self, name, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step(name)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--host-steps', type=int, default=5)
    a = ap.parse_args()
    import gpe_amd
    t0 = time.perf_counter()
    bench = Bench(a.warmup + a.rounds * a.steps + 1)
    res = {'shape': [B, N_ST + N_NON, 16], 'resident_garments': G, 'resident_mb': round(sum(x.nbytes for x in bench.host) / 2 ** 20, 1),
           'math': gpe_amd.get_math(), 'steps_per_window': a.steps, 'host_steps_per_window': a.host_steps,
           'setup_s': round(time.perf_counter() - t0, 1), 'ms_per_step': {}}
    for v in VARIANTS:
        bench.window(v, 1 if v == 'host_draw' else a.warmup)
    for _ in range(a.rounds):                                 # alternating: drift of the clocks hits every variant alike
        for v in VARIANTS:
            res['ms_per_step'].setdefault(v, []).append(round(bench.window(v, a.host_steps if v == 'host_draw' else a.steps), 4))
    status = bench.sampler['step_sampled'].status
    res['status_of_last_step'] = {'gave_up_rows': int(status.clamp(min=0).sum()), 'refused_slots': int((status < 0).sum())}
    best = {k: min(v) for k, v in res['ms_per_step'].items()}
    res['best_ms'] = best
    res['spread_pct'] = {k: round(100.0 * (max(v) - min(v)) / min(v), 2) for k, v in res['ms_per_step'].items()}
    res['sampled_minus_fixed_ms'] = round(best['step_sampled'] - best['step_fixed'], 4)
    res['host_over_sampler'] = round(best['host_draw'] / best['sampler'], 1)
    res['host_over_sampler_graph'] = round(best['host_draw'] / best['sampler_graph'], 1)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()

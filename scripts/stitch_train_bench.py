#!/usr/bin/env python3
"""A training step of the edge-pair classifier (nets.StitchOnEdge3DPairs) at the shipped training shape: 30 garments x 400 sampled
pair rows x 16 features = 12 000 rows per step, MLP([16, 200, 200, 200, 1]), metrics on (the default), FusedAdam under OneCycle.
Three variants from the same weights in one process, alternating, `--warmup` steps each first, best of `--rounds` windows of
`--steps` steps (wall clock around a window, device drained at both ends):

  torch_loss    eager; the loss written as the torch expressions ComposedLoss ran on device tensors before the loss kernel
                (BCEWithLogitsLoss, round(sigmoid), the sums, and the two host reads of `hit / n if n else 0`)
  device_loss   eager; model.loss = ops.PairClassLossFn, one forward and one backward launch, no host read
  captured      graph.StepGraph over the same step with the loss dict as extras

Before timing, seven steps of each from the same weights: device_loss and captured must agree bit for bit (losses and metrics);
torch_loss must meet the first loss within 1e-5 (same weights: the bar of tests/test_gpu_stitch_train.py) and the later ones within
2e-3 max(1, loss) (the trajectory bar: Adam turns rounding-level gradient differences into +- lr).  One JSON line.

    python scripts/stitch_train_bench.py [--steps 300] [--rounds 3] [--warmup 20]

Launches per step and kernel times come from separate kernel-trace runs of ONE variant (warm-up steps included in the trace: the
script prints how many steps ran in all):

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/stitch_train_bench.py --only captured --steps 200
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPE = (30, 400, 16)
VARIANTS = ('torch_loss', 'device_loss', 'captured')


def torch_loss(preds, ground_truth):
    """ComposedLoss.__call__ as it ran on device tensors before ops.pair_class_loss, default configuration"""
    loss_dict = {}
    pair_loss = torch.nn.functional.binary_cross_entropy_with_logits(preds.view(-1), ground_truth.view(-1).float())
    loss_dict.update(edge_pair_class_loss=pair_loss)
    full_loss = 0. + pair_loss
    with torch.no_grad():
        cls = torch.round(torch.sigmoid(preds))
        loss_dict.update(edge_pair_class_acc=(cls == ground_truth).sum().float() / ground_truth.numel())
        hit = ((cls == 1) & (ground_truth == 1)).sum().float()
        n_pred, n_gt = (cls == 1).sum().float(), (ground_truth == 1).sum().float()
        loss_dict.update(stitch_precision=hit / n_pred if n_pred else 0, stitch_recall=hit / n_gt if n_gt else 0)
    return full_loss, loss_dict


class Variant:
    def __init__(self, name, model, rows, labels, total_steps):
        from gpe_amd import graph, optim
        self.name, self.model, self.rows, self.labels = name, model, rows, labels
        self.opt = optim.FusedAdam(optim.FlatArena(model), lr=2e-3, schedule=optim.OneCycle(2e-3, total_steps))
        self.sg = graph.StepGraph(lambda f, g: model.loss(model(f), g)[:2], self.opt, warmup=2) if name == 'captured' else None
        self.count = 0

    def step(self):
        """-> (loss, loss dict) of the step"""
        self.count += 1
        if self.sg is not None:
            return self.sg.step(self.rows, self.labels), self.sg.extras[0]
        out = self.model(self.rows)
        loss, d = torch_loss(out, self.labels) if self.name == 'torch_loss' else self.model.loss(out, self.labels)[:2]
        loss.backward()
        self.opt.step()
        return loss, d

    def window(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps


def setup(names, total_steps, seed=0):
    import gpe_amd
    torch.manual_seed(seed)
    base = gpe_amd.nets.StitchOnEdge3DPairs({'element_size': SHAPE[2]}, {}, {}).cuda().train()
    rows = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(seed + 1))
    labels = rows[..., 0] + 0.5 * rows[..., 1] * rows[..., 2] > 0.75
    rows, labels = rows.cuda(), labels.cuda()
    return [Variant(n, copy.deepcopy(base), rows, labels, total_steps) for n in names]


def agreement():
    """seven steps of every variant from the same weights"""
    runs = {}
    for v in setup(VARIANTS, 1000):
        runs[v.name] = []
        for _ in range(7):
            loss, d = v.step()
            runs[v.name].append([float(loss)] + [float(d[k]) for k in ('edge_pair_class_acc', 'stitch_precision', 'stitch_recall')])
        torch.cuda.synchronize()
    assert runs['device_loss'] == runs['captured'], (runs['device_loss'], runs['captured'])
    dist = [abs(a[0] - b[0]) for a, b in zip(runs['torch_loss'], runs['device_loss'])]
    assert dist[0] < 1e-5 and all(d < 2e-3 * max(1.0, b[0]) for d, b in zip(dist, runs['device_loss'])), dist
    return {'device_loss_equals_captured': True, 'torch_loss_distance_per_step': ['%.3g' % d for d in dist],
            'losses': ['%.6f' % r[0] for r in runs['device_loss']], 'last_metrics': runs['device_loss'][-1][1:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--only', choices=VARIANTS, help='run one variant for --warmup + --steps steps and time nothing (for a kernel trace)')
    a = ap.parse_args()
    import gpe_amd
    if a.only:
        v, = setup([a.only], a.warmup + a.steps + 1)
        v.window(a.warmup)
        ms = v.window(a.steps)
        print(json.dumps({'only': a.only, 'steps_run': v.count, 'ms_per_step_under_trace': round(ms, 4)}), flush=True)
        return
    res = {'shape': list(SHAPE), 'rows_per_step': SHAPE[0] * SHAPE[1], 'math': gpe_amd.get_math(), 'steps_per_window': a.steps,
           'agreement': agreement(), 'ms_per_step': {}}
    variants = setup(VARIANTS, a.warmup + a.rounds * a.steps + 1)
    for v in variants:
        v.window(a.warmup)
    for _ in range(a.rounds):                                 # alternating: drift of the clocks hits every variant alike
        for v in variants:
            res['ms_per_step'].setdefault(v.name, []).append(round(v.window(a.steps), 4))
    best = {k: min(v) for k, v in res['ms_per_step'].items()}
    res['best_ms'] = best
    res['spread_pct'] = {k: round(100.0 * (max(v) - min(v)) / min(v), 2) for k, v in res['ms_per_step'].items()}
    res['pair_rows_per_s'] = {k: round(res['rows_per_step'] / (b * 1e-3)) for k, b in best.items()}
    res['torch_over_device'] = round(best['torch_loss'] / best['device_loss'], 3)
    res['torch_over_captured'] = round(best['torch_loss'] / best['captured'], 3)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()

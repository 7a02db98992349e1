"""Cost of DynamicASAPool at the cfg-2 shape (B 32, N 2048, F 112 — the output of the first EdgeConv layer at EConv_feature 112 would be
56 wide with graph_pooling; both widths are timed): the pool's kNN search, its kernels forward + backward, and a whole training step
of GarmentFullPattern3D with graph_pooling: True (k 16, pool_ratio 0.1) next to the unpooled step.  Prints one JSON object;
--out writes it to a file as well (profiles/).

    python scripts/asap_bench.py --out profiles/asap_bench.json
"""
import argparse
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import gpe_amd  # noqa: E402
from gpe_amd import _lib as L, configs, nets, net_blocks as nb, ops, optim  # noqa: E402


def _per_call(fn, reps):
    """-> {entry point: mean ms per call of fn} from HIP events around every C-ABI call (the library's TIMING hook)."""
    fn()
    torch.cuda.synchronize()
    L.TIMING = []
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out = {}
        for name, _args, e0, e1 in L.TIMING:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1) / reps
        return out
    finally:
        L.TIMING = None


def _pool_cost(B, N, F, ratio, reps):
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    pool = nb.DynamicASAPool(F, pool_ratio=ratio).to(dev)
    x = torch.randn(B * N, F, device=dev, requires_grad=True)
    g = torch.randn(B * ops.asap_count(N, ratio), F, device=dev)

    def step():
        out, _ = pool(x, (B, N))
        out.backward(g)
    t = _per_call(step, reps)
    return {'F': F, 'knn_ms': round(t.get('gpe_knn', 0.0), 4), 'knn_reverse_ms': round(t.get('gpe_knn_reverse', 0.0), 4),
            'pool_fwd_ms': round(t.get('gpe_asap_fwd', 0.0), 4), 'pool_bwd_ms': round(t.get('gpe_asap_bwd', 0.0), 4)}


def _step_ms(graph_pooling, B, N, k, steps, warmup):
    dev = torch.device('cuda', 0)
    data_config = configs.data_config()
    cfg = configs.lstm_model_config(k_neighbors=k, graph_pooling=graph_pooling, pool_ratio=0.1)
    torch.manual_seed(0)
    model = nets.GarmentFullPattern3D(data_config, copy.deepcopy(cfg), copy.deepcopy(cfg['loss'])).to(dev).train()
    model.loss.with_quality_eval = False
    opt = optim.FusedAdam(optim.FlatArena(model), lr=2e-3)
    feats, gt = bench.synthetic(B, N, data_config, seed=1000, device=dev)

    def one():
        loss = model.loss(model(feats), gt, epoch=0)[0]
        loss.backward()
        opt.step()
    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        one()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--points', type=int, default=2048)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--math', default='f16x3')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    gpe_amd.set_math(a.math)
    res = {'shape': {'B': a.batch, 'N': a.points, 'k': a.k, 'pool_ratio': 0.1}, 'math_mode': a.math,
           'pool_layer1': _pool_cost(a.batch, a.points, 56, 0.1, a.steps),
           'pool_F112': _pool_cost(a.batch, a.points, 112, 0.1, a.steps),
           'step_ms_pooled': round(_step_ms(True, a.batch, a.points, a.k, a.steps, a.warmup), 4),
           'step_ms_unpooled': round(_step_ms(False, a.batch, a.points, a.k, a.steps, a.warmup), 4)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

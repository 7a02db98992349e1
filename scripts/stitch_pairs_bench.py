#!/usr/bin/env python3
"""Stitch recovery from the edge-pair classifier (ops.stitch_pairs, csrc/gpe_stitch_pairs.hip) at the size of a prediction batch:
B = 32 full garments of 23 panels x 14 edges (49 588 pairs each, 1.59 M per call), the shipped classifier widths
MLP([16, 200, 200, 200, 1]).  Times route='fused' (store-free kernel) against route='rows' (materialised pair rows through the
dense-MLP kernels: what a caller had to do before the fused path existed) in one process, alternating, with device events after a
warm-up and enough repetitions for windows >= 1 s, in the f32 and f16x3 arithmetic modes; records the peak device memory of both
routes and compares their outputs (stitches exactly, logits within 2 tol, tol = 1e-4 * max(1, max |logit|)).  One JSON line.
Kernel times come from a separate kernel-trace run:

    python scripts/stitch_pairs_bench.py [--batch 32] [--window 1.0] [--rounds 3]

--eval times the evaluating call (ops.stitch_pairs_eval: the same pass plus ComposedLoss' numbers over all pairs against ground-truth
stitches) against two baselines in the same process, alternating, per route and mode: the prediction-only call, and the host detour a
caller had to take before (dense logits [B, E, E], a torch gather of the valid entries, labels from a Python set, torch BCE and
counts, one host read of the numbers).
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/stitch_pairs_bench.py --window 0.2 --rounds 1
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, 'tests', 'golden')


def inputs(B, seed=0):
    """B variations of the full 23 x 14 garment of tests/golden/stitch_pairs_full.pt (vertices moved by ~2 mm each)"""
    fx = torch.load(os.path.join(GOLDEN, 'stitch_pairs_full.pt'), weights_only=False)
    g = torch.Generator().manual_seed(seed)
    edges = fx['edges'][None].repeat(B, 1, 1, 1)
    edges[..., :6] += 0.2 * torch.randn(edges[..., :6].shape, generator=g)
    edges[0] = fx['edges']
    return edges.cuda(), fx['num_edges'][None].repeat(B, 1).cuda(), {'f_shift': fx['f_shift'], 'f_scale': fx['f_scale']}


def timed(fn, window):
    """median-free: total device time of n back-to-back calls, n grown until the window is >= `window` seconds -> ms per call"""
    n = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= window * 1e3:
            return ms / n, n
        n = max(n + 1, int(n * window * 1.2e3 / max(ms, 1e-3)))


def ground_truth(fx, B):
    """the planted stitches of the full garment in the product's layout, for every garment of the batch"""
    L = fx['edges'].shape[1]
    gt = torch.tensor([[a[0] * L + a[1] for a, _ in fx['plants']], [b[0] * L + b[1] for _, b in fx['plants']]], dtype=torch.int32)
    return gt[None].repeat(B, 1, 1).cuda(), torch.full((B,), gt.shape[1], dtype=torch.int32).cuda()


def host_detour(model, edges, ne, stats, route, plants, L):
    """what scoring all pairs took without the evaluating kernels"""
    out = model.predict_stitches(edges, ne, stats, route=route, return_logits=True)
    dense = out['logits']
    valid = ~torch.isnan(dense)
    b, i, j = valid.nonzero(as_tuple=True)
    st = {(a[0] * L + a[1], c[0] * L + c[1]) for a, c in plants}
    st |= {(c, a) for a, c in st}
    lab = torch.zeros(dense.shape[1:], dtype=torch.bool)
    for a, c in st:
        lab[a, c] = True
    y = lab.to(dense.device)[i, j]
    x = dense[b, i, j]
    loss = torch.nn.functional.binary_cross_entropy_with_logits(x, y.float())
    cls = torch.sigmoid(x) > 0.5
    nums = torch.stack([(cls == y).sum(), (cls & y).sum(), cls.sum(), y.sum()])
    return float(loss), nums.tolist()


def eval_main(a):
    import gpe_amd
    known = torch.load(os.path.join(GOLDEN, 'stitch_pairs_known_answer.pt'), weights_only=False)
    fx = torch.load(os.path.join(GOLDEN, 'stitch_pairs_full.pt'), weights_only=False)
    model = gpe_amd.nets.StitchOnEdge3DPairs(known['data_config'], dict(known['nn_config']), {})
    model.load_state_dict(known['state_dict'])
    model = model.cuda().eval()
    edges, ne, stats = inputs(a.batch)
    gt, n = ground_truth(fx, a.batch)
    P, L = edges.shape[1:3]
    res = {'eval': True, 'B': a.batch, 'P': P, 'L': L, 'window_s': a.window, 'modes': {}}
    for mode in ('f32', 'f16x3'):
        prev = gpe_amd.set_math(mode)
        res['modes'][mode] = {}
        for route in ('fused', 'rows'):
            r = {}
            calls = {'predict': lambda: model.predict_stitches(edges, ne, stats, route=route),
                     'eval': lambda: model.evaluate_stitches(edges, ne, gt, n, stats, route=route),
                     'detour': lambda: host_detour(model, edges, ne, stats, route, fx['plants'], L)}
            out, loss_dict = calls['eval']()
            loss, nums = calls['detour']()
            c = out['counts'].sum(0).tolist()
            r['counts_equal_detour'] = c[1:5] == nums
            r['loss'] = float(loss_dict['edge_pair_class_loss'])
            r['loss_minus_detour'] = r['loss'] - loss
            for f in calls.values():
                for _ in range(3):
                    f()
            for rnd in range(a.rounds):
                for k, f in calls.items():
                    ms, cnt = timed(f, a.window)
                    r.setdefault(k + '_ms', []).append(round(ms, 4))
            best = {k: min(r[k + '_ms']) for k in calls}
            r['eval_over_predict'] = round(best['eval'] / best['predict'], 4)
            r['eval_minus_predict_ms'] = round(best['eval'] - best['predict'], 4)
            r['detour_over_eval'] = round(best['detour'] / best['eval'], 3)
            r['spread_pct'] = {k: round(100.0 * (max(r[k + '_ms']) - best[k]) / best[k], 2) for k in calls}
            res['modes'][mode][route] = r
        gpe_amd.set_math(prev)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--eval', action='store_true', help='time the evaluating call against prediction-only and the host detour')
    a = ap.parse_args()
    if a.eval:
        return eval_main(a)
    import gpe_amd
    known = torch.load(os.path.join(GOLDEN, 'stitch_pairs_known_answer.pt'), weights_only=False)
    model = gpe_amd.nets.StitchOnEdge3DPairs(known['data_config'], dict(known['nn_config']), {})
    model.load_state_dict(known['state_dict'])
    model = model.cuda().eval()
    edges, ne, stats = inputs(a.batch)
    P, L = edges.shape[1:3]
    pairs = sum(int(ne[0, i]) * int(ne[0, j]) for i in range(P) for j in range(i + 1, P))
    res = {'B': a.batch, 'P': P, 'L': L, 'pairs_per_call': pairs * a.batch, 'window_s': a.window, 'modes': {}}
    for mode in ('f32', 'f16x3'):
        prev = gpe_amd.set_math(mode)
        r = {}
        # outputs at this size: the two routes against each other
        f = model.predict_stitches(edges, ne, stats, route='fused', return_logits=True)
        w = model.predict_stitches(edges, ne, stats, route='rows', return_logits=True)
        valid = ~torch.isnan(w['logits'])
        tol = 1e-4 * max(1.0, w['logits'][valid].abs().max().item())
        r['tol'] = tol
        r['valid_pairs'] = int(valid.sum())
        r['nan_masks_equal'] = bool(torch.equal(valid, ~torch.isnan(f['logits'])))
        r['max_logit_diff'] = (f['logits'][valid] - w['logits'][valid]).abs().max().item()
        r['logits_within_2tol'] = r['max_logit_diff'] < 2 * tol
        r['stitches_equal'] = bool(torch.equal(f['stitches'], w['stitches']) and torch.equal(f['num_stitches'], w['num_stitches']))
        r['stitches_per_garment'] = f['num_stitches'].float().mean().item()
        del f, w, valid
        for route in ('fused', 'rows'):
            call = lambda route=route: model.predict_stitches(edges, ne, stats, route=route)
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            call()
            torch.cuda.synchronize()
            r[route + '_peak_MB'] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        for rnd in range(a.rounds):                       # alternating: drift of the clock hits both routes alike
            for route in ('fused', 'rows'):
                ms, n = timed(lambda route=route: model.predict_stitches(edges, ne, stats, route=route), a.window)
                r.setdefault(route + '_ms', []).append(round(ms, 4))
                r[route + '_calls_per_window'] = n
        fb, rb = min(r['fused_ms']), min(r['rows_ms'])
        r['spread_pct'] = {k: round(100.0 * (max(r[k + '_ms']) - min(r[k + '_ms'])) / min(r[k + '_ms']), 2) for k in ('fused', 'rows')}
        r['rows_over_fused'] = round(rb / fb, 3)
        r['fused_pairs_per_s'] = round(res['pairs_per_call'] / (fb * 1e-3))
        gpe_amd.set_math(prev)
        res['modes'][mode] = r
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()

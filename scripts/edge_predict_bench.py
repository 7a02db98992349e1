#!/usr/bin/env python3
"""The encoder's prediction path (DynamicEdgeConv.predict / model.predict, csrc/gpe_edge_predict.hip) at the shapes of BASELINE cfg 1
(GarmentFullPattern3D, N = 1024, batch 8, k = 5), cfg 2 (2048, 32, 16) and cfg 4 (GarmentSegmentPattern3D, 4096, 32, 20).

Per shape and arithmetic mode (f32, f16x3) it times, in one process, alternating, with device events after a warm-up and enough
repetitions per window:
  per conv layer   conv.forward in eval mode under no_grad (what a caller ran before predict existed: the comparand)
                   conv.predict(route='fused') and conv.predict(route='layers')
  end to end       model(x) in eval mode under no_grad (the comparand), model.predict(x, route='fused' / 'layers' / 'auto')
and records the peak device memory above the resting level of one call of each, and the largest output difference between the fused
route and the eval forward.  One JSON line per shape.

    python scripts/edge_predict_bench.py [--cfg 1 2 4] [--window 0.3] [--rounds 3] [--modes f32 f16x3]
Kernel times come from a separate kernel-trace run:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/edge_predict_bench.py --cfg 2 --window 0.05 --rounds 1
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CFGS = {1: ('lstm', 1024, 8, 5), 2: ('lstm', 2048, 32, 16), 4: ('att', 4096, 32, 20)}


def timed(fn, window):
    """total device time of n back-to-back calls, n grown until the window is >= `window` seconds -> ms per call"""
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
            return ms / n
        n = max(n + 1, int(n * window * 1.2e3 / max(ms, 1e-3)))


def peak_mb(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def race(calls, window, rounds):
    """calls: {name: fn} -> {name: {'ms': best, 'spread_pct', 'peak_MB'}}; the calls alternate inside every round"""
    out = {k: {'peak_MB': peak_mb(f), 'all_ms': []} for k, f in calls.items()}
    for _ in range(rounds):
        for k, f in calls.items():
            out[k]['all_ms'].append(round(timed(f, window), 4))
    for r in out.values():
        r['ms'] = min(r['all_ms'])
        r['spread_pct'] = round(100.0 * (max(r['all_ms']) - r['ms']) / r['ms'], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', type=int, nargs='+', default=[1, 2, 4], choices=sorted(CFGS))
    ap.add_argument('--modes', nargs='+', default=['f32', 'f16x3'])
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    import gpe_amd
    from gpe_amd import configs, nets
    data_config = configs.data_config()
    for c in a.cfg:
        kind, N, B, k = CFGS[c]
        nn_cfg = (configs.att_model_config if kind == 'att' else configs.lstm_model_config)(k_neighbors=k)
        torch.manual_seed(0)
        cls = nets.GarmentSegmentPattern3D if kind == 'att' else nets.GarmentFullPattern3D
        model = cls(data_config, dict(nn_cfg), dict(nn_cfg['loss'])).cuda().train()
        x = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(1000)).cuda()
        with torch.no_grad():
            model(x, log_step=0, epoch=0)                 # one training-mode forward: running statistics away from (0, 1)
        model.eval()
        convs = model.feature_extractor.conv_layers
        res = {'cfg': c, 'model': kind, 'N': N, 'B': B, 'k': k, 'edges': B * N * k, 'window_s': a.window, 'modes': {}}
        for mode in a.modes:
            prev = gpe_amd.set_math(mode)
            r = {}
            with torch.no_grad():
                h = x.view(B * N, 3)
                for li, conv in enumerate(convs):
                    want = conv(h, B, N)
                    got = conv.predict(h, B, N, route='fused')
                    r['conv%d' % li] = race({'forward': lambda conv=conv, h=h: conv(h, B, N),
                                             'fused': lambda conv=conv, h=h: conv.predict(h, B, N, route='fused'),
                                             'layers': lambda conv=conv, h=h: conv.predict(h, B, N, route='layers')}, a.window, a.rounds)
                    r['conv%d' % li]['max_abs_diff'] = (got - want).abs().max().item()
                    r['conv%d' % li]['max_abs'] = want.abs().max().item()
                    h = want.contiguous()
                del want, got, h

                def fwd():
                    with torch.no_grad():
                        return model(x)
                torch.manual_seed(5)
                want = fwd()
                torch.manual_seed(5)
                got = model.predict(x, route='fused')
                r['model_max_abs_diff'] = {key: (got[key] - want[key]).abs().max().item() for key in want}
                del want, got
                r['model'] = race({'forward': fwd,
                                   'fused': lambda: model.predict(x, route='fused'),
                                   'layers': lambda: model.predict(x, route='layers'),
                                   'auto': lambda: model.predict(x)}, a.window, a.rounds)
            for part in r.values():
                if isinstance(part, dict) and 'forward' in part:
                    part['fused_over_forward'] = round(part['fused']['ms'] / part['forward']['ms'], 3)
            gpe_amd.set_math(prev)
            res['modes'][mode] = r
        print(json.dumps(res), flush=True)
        del model, x
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

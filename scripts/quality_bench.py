#!/usr/bin/env python3
"""Validation-pass cost of the quality metrics (ComposedPatternLoss quality_components, csrc/gpe_quality.hip): model.eval() +
no_grad forward + loss per batch, quality on vs off, synchronised wall time over warmed batches, at the shipped
lstm_stitch_tags training shape (GarmentFullPattern3D, N = 2000, batch 30, k = 5, epoch 40) and at cfg 2 (N = 2048, batch 32,
k = 16).  Prints one JSON line per shape.  The quality kernels' own time comes from a separate kernel-trace run:

    python scripts/quality_bench.py [--batches 60] [--warmup 10]
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/quality_bench.py --batches 20 --warmup 2
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {'shipped': dict(N=2000, B=30, k=5), 'cfg2': dict(N=2048, B=32, k=16)}


def run(name, shape, batches, warmup, epoch):
    import bench
    from gpe_amd import configs, nets
    data_config = configs.data_config()
    nn_cfg = configs.lstm_model_config(k_neighbors=shape['k'])
    torch.manual_seed(0)
    model = nets.GarmentFullPattern3D(data_config, dict(nn_cfg), dict(nn_cfg['loss'])).cuda().eval()
    feats, gt = bench.synthetic(shape['B'], shape['N'], data_config, seed=1, device='cuda')
    gt['num_panels'] = (gt['num_edges'] >= 3).sum(1)
    res = {'shape': name, 'B': shape['B'], 'N': shape['N'], 'k': shape['k'], 'epoch': epoch,
           'quality_components': nn_cfg['loss']['quality_components']}
    for quality in (False, True, False, True):        # interleaved: drift of the clock hits both settings alike
        model.loss.with_quality_eval = quality
        times = []
        with torch.no_grad():
            for i in range(warmup + batches):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                preds = model(feats)
                _, d, _ = model.loss(preds, dict(gt), epoch=epoch)
                torch.cuda.synchronize()
                if i >= warmup:
                    times.append(time.perf_counter() - t0)
        times.sort()
        key = 'quality_on' if quality else 'quality_off'
        med = times[len(times) // 2] * 1e3
        res.setdefault(key + '_median_ms', []).append(round(med, 4))
        if quality:
            res['keys'] = sorted(k for k in d if k in __import__('gpe_amd').ops.QUALITY_KEYS)
    on, off = min(res['quality_on_median_ms']), min(res['quality_off_median_ms'])
    res['overhead_ms'] = round(on - off, 4)
    res['overhead_pct'] = round(100.0 * (on - off) / off, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--epoch', type=int, default=40)
    ap.add_argument('--shapes', default='shipped,cfg2')
    a = ap.parse_args()
    for name in a.shapes.split(','):
        print(json.dumps(run(name, SHAPES[name], a.batches, a.warmup, a.epoch)), flush=True)


if __name__ == '__main__':
    main()

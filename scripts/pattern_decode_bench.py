#!/usr/bin/env python3
"""Times ops.pattern_decode (csrc/gpe_pattern_decode.hip) against the per-garment host loop it replaces, on the same inputs.

Shapes: the shipped pattern size P = 23, L = 14 at B = 1200 (the size of the reference's test split) and B = 32.  Inputs are
garment-shaped (tests/quality_restate.make_batch): 3 - 11 real panels and up to 24 stitches per garment.
Device: `--reps` calls between two device events after `--warmup` calls, repeated `--rounds` times; the median round is reported with
the spread (a launch returns before the kernel finishes: only the events, or a synchronise, see its end).  The tensors stay on the
device: no host read is inside the timed window.
Host: tests/pattern_decode_restate.host_loop — the reference's steps in fp64 numpy, one garment and one panel at a time — on CPU
copies of the same tensors, host clock, best of `--host-rounds` (B = 1200 once).  The reference's own loop cannot be timed where
its `pattern` package is absent; the restatement walks the same per-panel and per-stitch Python loops.
Prints one JSON line per shape.  Needs the MI355X: there is no fallback.

    python scripts/pattern_decode_bench.py [--reps 200] [--rounds 5]
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
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

import gpe_amd  # noqa: E402
import pattern_decode_restate as R  # noqa: E402
import quality_restate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-rounds', type=int, default=3)
    ap.add_argument('--batches', type=int, nargs='*', default=[1200, 32])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pattern_decode_bench needs the MI355X')
    fx = torch.load(os.path.join(REPO, 'tests', 'golden', 'quality_lstm_e40.pt'), weights_only=False)
    dc = fx['data_config']
    P, L, S, stats = dc['max_pattern_len'], dc['max_panel_len'], dc['max_num_stitches'], dc['standardize']
    kinds = ['ok', 'pad_real', 'ok', 'open', 'extra', 'ok', 'odd', 'ok']
    for B in args.batches:
        preds, _ = quality_restate.make_batch(np.random.default_rng(B), B, P, L, S, dc, kinds)
        dev = {k: v.cuda() for k, v in preds.items()}
        for _ in range(args.warmup):
            out = gpe_amd.ops.pattern_decode(dev, stats)
        torch.cuda.synchronize()
        rounds = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                out = gpe_amd.ops.pattern_decode(dev, stats)
            e1.record()
            e1.synchronize()
            rounds.append(e0.elapsed_time(e1) / args.reps)
        host = []
        for _ in range(1 if B > 100 else args.host_rounds):
            t0 = time.perf_counter()
            want = R.host_loop(preds, stats)
            host.append((time.perf_counter() - t0) * 1e3)
        same = all(np.array_equal(out[k].cpu().numpy(), want[k], equal_nan=True) for k in R.KEYS)
        d_ms, h_ms = statistics.median(rounds), min(host)
        print(json.dumps({'bench': 'pattern_decode', 'B': B, 'P': P, 'L': L, 'device_ms_per_call': round(d_ms, 5),
                          'device_ms_min_max': [round(min(rounds), 5), round(max(rounds), 5)],
                          'device_us_per_garment': round(1e3 * d_ms / B, 4), 'host_loop_ms': round(h_ms, 2),
                          'host_us_per_garment': round(1e3 * h_ms / B, 1), 'ratio_host_over_device': round(h_ms / d_ms, 1),
                          'same_result': bool(same), 'reps': args.reps, 'rounds': args.rounds}), flush=True)


if __name__ == '__main__':
    main()

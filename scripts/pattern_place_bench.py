#!/usr/bin/env python3
"""Times the step between the two prediction stages (ops.pattern_place, csrc/gpe_pattern_place.hip) and the tail of
model.predict_garment (place + the edge-pair classifier, ops.stitch_pairs with the shipped weights) against the per-garment host loop a
caller had to write before, on the same decoded patterns.

Shape: the shipped pattern size P = 23, L = 14 at B = 1200 (the size of the reference's test split).  Inputs are garment-shaped
(tests/quality_restate.make_batch: 3 - 11 real panels per garment), decoded on the device once, outside every timed window.
Device: `--place-reps` / `--reps` calls between two device events (windows of about half a second) after `--warmup` calls, repeated
`--rounds` times, the two variants alternating; the median round is reported with its spread.  At this size a call of place alone is
as long as its enqueue: the figure is the rate of back-to-back calls, host side included.  The tensors stay on the device: no host
read is inside a timed window.
Host loop: per garment, the decoded tensors read back, tests/pattern_place_restate.host_loop (the reference's per-panel steps in fp64
numpy), the garment's edges copied to the device and one stitch_pairs call of batch 1; host clock around the loop, ending in a device
synchronise.  The restatement's part of that time is reported on its own.  The reference's own loop cannot be timed where its `pattern`
package is absent; the restatement walks the same per-panel Python loops.
Prints one JSON line.  Needs the MI355X: there is no fallback.

    python scripts/pattern_place_bench.py [--batch 1200] [--reps 60] [--place-reps 20000] [--rounds 5]
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
GOLDEN = os.path.join(REPO, 'tests', 'golden')

import gpe_amd  # noqa: E402
import pattern_place_restate as R  # noqa: E402
import quality_restate  # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1200)
    ap.add_argument('--reps', type=int, default=60, help='calls of the tail per timed window')
    ap.add_argument('--place-reps', type=int, default=20000, help='calls of place alone per timed window')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-garments', type=int, default=0, help='garments the host loop walks (0: all)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('pattern_place_bench needs the MI355X')
    ops = gpe_amd.ops
    fx = torch.load(os.path.join(GOLDEN, 'quality_lstm_e40.pt'), weights_only=False)
    dc = fx['data_config']
    B, P, L, S, stats = args.batch, dc['max_pattern_len'], dc['max_panel_len'], dc['max_num_stitches'], dc['standardize']
    known = torch.load(os.path.join(GOLDEN, 'stitch_pairs_known_answer.pt'), weights_only=False)
    model = gpe_amd.nets.StitchOnEdge3DPairs(known['data_config'], dict(known['nn_config']), {})
    model.load_state_dict(known['state_dict'])
    model = model.cuda().eval()
    full = torch.load(os.path.join(GOLDEN, 'stitch_pairs_full.pt'), weights_only=False)
    pair_stats = {'f_shift': full['f_shift'], 'f_scale': full['f_scale']}
    preds, _ = quality_restate.make_batch(np.random.default_rng(B), B, P, L, S, dc, ['ok', 'pad_real', 'ok', 'open', 'extra', 'ok'])
    decoded = ops.pattern_decode({k: v.cuda() for k, v in preds.items()}, stats)

    def place():
        return ops.pattern_place(decoded)

    def tail():
        o = ops.pattern_place(decoded)
        return o, model.predict_stitches(o['edges3d'], decoded['num_edges'], pair_stats)

    for _ in range(args.warmup):
        placed, (_, sewn) = place(), tail()
    torch.cuda.synchronize()
    rounds = {'place': [], 'tail': []}
    for _ in range(args.rounds):                            # alternating: a drift of the clock hits both alike
        rounds['place'].append(timed(place, args.place_reps))
        rounds['tail'].append(timed(tail, args.reps))
    # the per-garment host loop
    n = B if args.host_garments <= 0 else min(B, args.host_garments)
    keys = ops.PATTERN_PLACE_INPUTS
    restate_s = 0.0
    host_edges = np.zeros((n, P, L, 8), np.float32)
    host_stitches, host_counts = [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(n):
        one = {k: decoded[k][b:b + 1].cpu().numpy() for k in keys}
        t1 = time.perf_counter()
        o = R.host_loop(one)
        restate_s += time.perf_counter() - t1
        host_edges[b] = o['edges3d'][0]
        out = model.predict_stitches(torch.from_numpy(o['edges3d']).cuda(), decoded['num_edges'][b:b + 1], pair_stats)
        host_stitches.append(out['stitches'])
        host_counts.append(out['num_stitches'])
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3
    # the same answers: edge rows within 1 ulp (tests/test_pattern_place_host.py), stitches equal where the rows are bit-equal
    got = placed['edges3d'][:n].cpu().numpy()
    ordered = lambda a: np.where(a.view(np.int32) < 0, -(a.view(np.int32).astype(np.int64) & 0x7fffffff), a.view(np.int32))  # noqa: E731
    ulps = int(np.abs(ordered(got) - ordered(host_edges)).max())
    rows_equal = (got.view(np.int32) == host_edges.view(np.int32)).reshape(n, -1).all(1)
    st_equal = np.array([bool(torch.equal(host_stitches[b][0], sewn['stitches'][b]) and
                              int(host_counts[b][0]) == int(sewn['num_stitches'][b])) for b in range(n)])
    med = {k: statistics.median(v) for k, v in rounds.items()}
    print(json.dumps({
        'bench': 'pattern_place', 'B': B, 'P': P, 'L': L, 'panels': int((decoded['num_edges'] > 0).sum()),
        'edges': int(decoded['num_edges'].sum()), 'stitches_found': int(sewn['num_stitches'].sum()),
        'place_ms_per_call': round(med['place'], 5), 'place_ms_min_max': [round(min(rounds['place']), 5), round(max(rounds['place']), 5)],
        'place_us_per_garment': round(1e3 * med['place'] / B, 4),
        'tail_ms_per_call': round(med['tail'], 4), 'tail_ms_min_max': [round(min(rounds['tail']), 4), round(max(rounds['tail']), 4)],
        'host_garments': n, 'host_loop_ms': round(host_ms, 1), 'host_restatement_ms': round(restate_s * 1e3, 1),
        'host_ms_per_garment': round(host_ms / n, 3), 'tail_ms_per_garment': round(med['tail'] / B, 5),
        'max_ulps_edges3d': ulps, 'garments_rows_bit_equal': int(rows_equal.sum()),
        'stitches_equal_where_rows_equal': bool(st_equal[rows_equal].all()), 'garments_stitches_equal': int(st_equal.sum()),
        'reps': args.reps, 'place_reps': args.place_reps, 'rounds': args.rounds}), flush=True)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Times the second stage of the two-stage evaluation pass over 1200 garments drawn from a seed
(tests/quality_restate.make_batch), batch 30, P = 23, L = 14, the shipped classifier weights, two ways in one command:

  device   evaluation.FrameworkEvaluator: begin, add_predictions per batch (decode -> place -> classifier -> ONE accumulate launch),
           finish (one pooling launch, ONE host read for the whole set);
  host     the same pass from the public calls the package had before: ops.pattern_decode, DecodedPatterns.place,
           StitchOnEdge3DPairs.evaluate_stitches, then ONE .cpu() per batch of the per-garment counts / loss sums (and of the
           decode's few integers the rules read, packed into the same tensor: the kindest form) and the rules and the fold on the host,
           vectorised (`host_fold` below: numpy masks for the rules, np.add.accumulate on float32 for the sequential adds — bit for
           bit the fold of tests/framework_eval_restate.fold, which is checked).  The host clock around that numpy part alone is
           reported as `host_fold_ms`: what is left of the host pass is the launches and the wait at every batch's read.

Both must agree before anything is timed: records, counters and integer totals exactly, the folded floats bit for bit (the same fp32
adds in the same order on both sides).  Protocol: warm-up passes of both, then `--rounds` rounds in which the two ALTERNATE; a
round's window is `reps` whole passes between two device events, `reps` chosen so that a window lasts at least `--window` seconds;
the median round and the spread are reported.  The predictions stay on the device; no first-stage model runs.

    python scripts/framework_eval_bench.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/framework_eval_bench.py --profile-passes 3
        (a run of its own for the kernel times of the two new launches: no timing, `n` device passes only)
Prints one JSON line; needs the MI355X."""
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
import framework_eval_restate as FW  # noqa: E402
import quality_restate  # noqa: E402


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def host_fold(h, P):
    """the rules and the fold of include/gpe_hip_framework.h on the packed per-garment numbers of a whole set (float64 [G, 12 + 2 P]:
    loss_sum, the six counts, num_selected, num_stitches, first_invalid, num_panels, gt_num_panels, num_edges [P], place_flags [P])
    -> (result dict of the one folder, records [G, 10]).  np.add.accumulate adds one element at a time in order, in float32."""
    f32 = np.float32
    ls, counts = h[:, 0], h[:, 1:7].astype(np.int64)
    n_sel, nums, first, n_pan, gt_pan = (h[:, i].astype(np.int64) for i in range(7, 12))
    bad = ((h[:, 12:12 + P] > 0) & (h[:, 12 + P:12 + 2 * P] != 0)).any(1)
    pairs, correct, tp, pred, gtp, sel_tp = counts.T
    state = np.where(bad, 1, np.where(np.where(first >= 0, first, nums) == 0, 2, np.where(pairs == 0, 3, 0)))
    corr = n_pan == gt_pan

    def ratio(num, den):
        return np.where(den != 0, num.astype(f32) / np.where(den != 0, den, 1).astype(f32), f32(0)).astype(f32)
    loss = (ls / np.where(pairs != 0, pairs, 1)).astype(f32)
    vals = np.stack([loss, loss, ratio(correct, pairs), ratio(tp, pred), ratio(tp, gtp), ratio(sel_tp, n_sel), ratio(sel_tp, gtp)], 1)
    res = {}
    for name, members in zip(FW.SETS, (state == 0, (state == 0) & corr)):
        n = int(members.sum())
        sums = np.add.accumulate(vals[members], axis=0, dtype=f32)[-1] if n else None
        res[name] = {k: (sums[j] / f32(n) if n else None) for j, k in enumerate(FW.KEYS)}
    res['skipped'] = dict(zip(FW.SKIP_REASONS, [int((state == 1).sum()), int((state == 2).sum()), int((state == 3).sum()),
                                                int(((state == 0) & ~corr).sum())]))
    records = np.concatenate([state[:, None].astype(np.float64), corr[:, None].astype(np.float64), h[:, 0:8]], 1)
    return res, records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--garments', type=int, default=1200)
    ap.add_argument('--batch', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--window', type=float, default=0.5, help='least seconds between the two device events of a window')
    ap.add_argument('--profile-passes', type=int, default=0, help='run this many device passes and nothing else (for a profiler)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('framework_eval_bench needs the MI355X')
    ops, evaluation = gpe_amd.ops, gpe_amd.evaluation
    from gpe_amd.patterns import DecodedPatterns
    q = torch.load(os.path.join(GOLDEN, 'quality_lstm_e40.pt'), weights_only=False)
    small = torch.load(os.path.join(GOLDEN, 'full3d_small.pt'), weights_only=False)
    dc = q['data_config']
    G, B, P, L, S, stats = args.garments, args.batch, dc['max_pattern_len'], dc['max_panel_len'], dc['max_num_stitches'], dc['standardize']
    known = torch.load(os.path.join(GOLDEN, 'stitch_pairs_known_answer.pt'), weights_only=False)
    stitch = gpe_amd.nets.StitchOnEdge3DPairs(known['data_config'], dict(known['nn_config']), {})
    stitch.load_state_dict(known['state_dict'])
    stitch = stitch.cuda().eval()
    full = torch.load(os.path.join(GOLDEN, 'stitch_pairs_full.pt'), weights_only=False)
    pair_stats = {'f_shift': full['f_shift'], 'f_scale': full['f_scale']}
    torch.manual_seed(0)          # the pattern model is never run here: the evaluator only wants one in eval mode on the device
    model = gpe_amd.nets.GarmentFullPattern3D(small['data_config'], dict(small['nn_config']), dict(q['loss_config'])).cuda().eval()
    preds, gt = quality_restate.make_batch(np.random.default_rng(G), G, P, L, S, dc, ['ok', 'pad_real', 'ok', 'open', 'extra', 'ok'])
    gt = {'stitches': gt['stitches'], 'num_panels': gt['num_panels']}
    cuts = [slice(a, min(a + B, G)) for a in range(0, G, B)]
    batches = [({k: v[c].cuda() for k, v in preds.items()}, {k: v[c].cuda() for k, v in gt.items()}) for c in cuts]
    ev = evaluation.FrameworkEvaluator(model, stitch, dc, pair_stats, shape_metrics=False)

    def device():
        ev.begin(total=G)
        for p, g in batches:
            ev.add_predictions(p, g)
        return ev.finish()[0]

    fold_s, last_h = [], [None]

    def host():
        rows = []
        with torch.no_grad():
            for p, g in batches:
                d = DecodedPatterns(ops.pattern_decode(p, stats, stitches=g['stitches'])).place()
                first, nums = d.first_invalid, d.num_stitches
                out, _ = stitch.evaluate_stitches(d.edges3d, d.num_edges, d.stitches, torch.where(first >= 0, first, nums), pair_stats)
                n = first.shape[0]
                packed = torch.cat([out['loss_sum'].view(n, 1), out['counts'].double(), out['num_stitches'].view(n, 1).double(),
                                    nums.view(n, 1).double(), first.view(n, 1).double(), d.num_panels.view(n, 1).double(),
                                    g['num_panels'].view(n, 1).double(), d.num_edges.double(), d.place_flags.double()], 1)
                rows.append(packed.cpu().numpy())           # THE host read of the batch
        t = time.perf_counter()
        last_h[0] = np.concatenate(rows)
        out = host_fold(last_h[0], P)
        fold_s.append(time.perf_counter() - t)
        return out

    if args.profile_passes:
        for _ in range(args.profile_passes):
            device()
        torch.cuda.synchronize()
        return
    for _ in range(args.warmup):
        got, (want, want_records) = device(), host()
    torch.cuda.synchronize()
    # agreement: integers exactly, floats bit for bit
    records = ev.records.cpu().numpy()
    if not np.array_equal(records.view(np.int64), want_records.view(np.int64)):
        raise SystemExit('the device records differ from the host loop\'s in rows %s' % np.argwhere((records != want_records).any(1))[:5].ravel())
    if got['skipped'] != want['skipped']:
        raise SystemExit('skipped: device %s, host %s' % (got['skipped'], want['skipped']))
    for name in FW.SETS:
        for k in FW.KEYS:
            a, b = got[name][k], want[name][k]
            if (a is None) != (b is None) or (a is not None and np.float32(a).view(np.int32) != np.float32(b).view(np.int32)):
                raise SystemExit('%s %s: device %r, host %r' % (name, k, a, b))
    # the vectorised host fold is the restatement's, bit for bit (so the host side is timed on a correct fold, not a convenient one)
    garments = [FW.garment(r[1:7], r[0], r[7], r[8], r[9], r[10], r[11], r[12:12 + P], r[12 + P:12 + 2 * P]) for r in last_h[0]]
    slow = FW.result(*FW.fold(garments)[:3])[0]
    for name in FW.SETS:
        for k in FW.KEYS:
            a, b = want[name][k], slow[name][k]
            if (a is None) != (b is None) or (a is not None and np.float32(a).view(np.int32) != np.float32(b).view(np.int32)):
                raise SystemExit('host_fold differs from tests/framework_eval_restate.fold in %s %s: %r, %r' % (name, k, a, b))
    totals = FW.pool(records)[0]
    if [ev.pooled['all']['counts']['stitch'][k] for k in FW.TOTALS] != totals[0, 0].tolist():
        raise SystemExit('the pooled totals differ from the fold of the records')
    # windows of at least args.window seconds
    once = {'device': window(device, 1), 'host': window(host, 1)}
    reps = {k: max(1, int(np.ceil(args.window * 1e3 / v))) for k, v in once.items()}
    rounds = {'device': [], 'host': []}
    del fold_s[:]
    for _ in range(args.rounds):                             # alternating: a drift of the clock hits both alike
        for k, fn in (('device', device), ('host', host)):
            rounds[k].append(window(fn, reps[k]))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    spread = {k: [round(min(v), 3), round(max(v), 3)] for k, v in rounds.items()}
    print(json.dumps({
        'bench': 'framework_eval', 'garments': G, 'batch': B, 'batches': len(batches), 'P': P, 'L': L,
        'counted': int(totals[0, 0, 7]), 'corr': int(totals[0, 1, 7]), 'skipped': got['skipped'], 'pairs': int(totals[0, 0, 0]),
        'unit': 'ms per pass over the set (device events around whole passes, the host work of a pass inside)',
        'device_ms': round(med['device'], 3), 'device_min_max': spread['device'], 'host_ms': round(med['host'], 3),
        'host_min_max': spread['host'],
        'host_fold_ms': round(1e3 * statistics.median(fold_s), 3), 'host_fold_min_max': [round(1e3 * min(fold_s), 3), round(1e3 * max(fold_s), 3)],
        'device_ms_per_batch': round(med['device'] / len(batches), 4),
        'host_ms_per_batch': round(med['host'] / len(batches), 4), 'passes_per_window': reps, 'rounds': args.rounds,
        'agree': 'records, counters and totals exactly; folded floats bit for bit', 'math': gpe_amd.get_math()}), flush=True)


if __name__ == '__main__':
    main()

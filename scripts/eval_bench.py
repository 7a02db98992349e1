"""An evaluation pass over a data set, measured three ways in one session:
  (a) host      model.predict + loss.__call__ per batch (one host read per batch inside the loss: the contributor counts), then the
                dicts averaged on the host by the reference's rule, one device-to-host copy per batch — what the package offered
                before evaluation.Evaluator;
  (b) eager     evaluation.Evaluator(capture=False): the same launches + one accumulate launch per batch, one host read per pass;
  (c) captured  evaluation.Evaluator(capture=True): the per-batch body replayed from a hipGraph;
and ops.quality_pool alone on a table of G = 20 000 garments in 12 groups.

Shapes: BASELINE cfg 1 (N = 1024, batch 8, k = 5) and cfg 2 (N = 2048, batch 32, k = 16), 64 batches, synthetic inputs from a seed.
Every variant is warmed up with one whole pass, then timed over `--reps` passes, the variants ALTERNATING inside a repetition; a
pass is timed with a host clock around work that ends in a device synchronise.  The three variants must agree bit for bit on every
key (checked before anything is timed).  `--noise 0 0.5 1 2` instead evaluates a MeshPointSampler-fed pass per noise level
(evaluation_scripts/noise_levels.py in shape: synthetic meshes, so the values mean nothing — the loop does).

    python scripts/eval_bench.py --out profiles/eval_bench.json
Prints one JSON line per configuration; needs the MI355X (there is no CPU path to time)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CONFIGS = {'cfg1': dict(points=1024, batch=8, k=5), 'cfg2': dict(points=2048, batch=32, k=16)}


def host_rule(per_batch):
    """the reference's aggregation (eval_utils.py:35-76) over [(full_loss, loss dict)], with ONE device-to-host copy per batch (the
    values that are not None, stacked) where the reference makes one per value: the kindest form of the host rule"""
    lists = {'full_loss': []}
    for full, d in per_batch:
        present = [k for k, v in d.items() if v is not None]
        vals = torch.stack([full] + [d[k] for k in present]).cpu().numpy()
        lists['full_loss'].append(vals[0])
        for k in d:
            lists.setdefault(k, [])
        for k, v in zip(present, vals[1:]):
            lists[k].append(v)
    with np.errstate(all='ignore'):
        return {k: (sum(v) / len(v) if v else None) for k, v in lists.items()}


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.float32(a), np.float32(b)
    return bool(a.view(np.int32) == b.view(np.int32) or (np.isnan(a) and np.isnan(b)))


def batches_for(cfg, n_batches, data_config, dev):
    from bench import synthetic
    out = []
    for i in range(n_batches):
        feats, gt = synthetic(cfg['batch'], cfg['points'], data_config, seed=500 + i, device=dev)
        # (an untrained model rarely predicts the right number of panels: most corr_ values are None here, the case the per-batch
        # host read of the contributor counts exists for)
        gt['num_panels'] = torch.full((cfg['batch'],), data_config['max_pattern_len'], dtype=torch.long, device=dev)
        out.append((feats, gt))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def measure(name, cfg, args, dev):
    import gpe_amd
    from gpe_amd import configs, evaluation, nets
    data_config = configs.data_config()
    nn_cfg = configs.lstm_model_config(k_neighbors=cfg['k'])
    torch.manual_seed(0)
    model = nets.GarmentFullPattern3D(data_config, dict(nn_cfg), dict(nn_cfg['loss'])).to(dev).eval()
    model.loss.with_quality_eval = True
    batches = batches_for(cfg, args.batches, data_config, dev)
    epoch = args.epoch

    def host():
        torch.manual_seed(1)
        per_batch = []
        with torch.no_grad():
            for x, gt in batches:
                full, d, _ = model.loss(model.predict(x), dict(gt), epoch=epoch)
                per_batch.append((full, d))
        return host_rule(per_batch)

    evs = {'eager': evaluation.Evaluator(model, epoch=epoch, capture=False),
           'captured': evaluation.Evaluator(model, epoch=epoch, capture=True)}

    def run(which):
        def f():
            torch.manual_seed(1)
            with torch.no_grad():
                return evs[which].run(batches)
        return f

    variants = {'host': host, 'eager': run('eager'), 'captured': run('captured')}
    results = {k: f() for k, f in variants.items()}                       # the warm-up pass of every variant, and the parity check
    for k in ('eager', 'captured'):
        bad = [key for key in results['host'] if not same(results[k][key], results['host'][key])]
        if list(results[k]) != list(results['host']) or bad:
            raise SystemExit('%s: the %s pass differs from the host pass in %s' % (name, k, bad or 'its keys'))
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, f in variants.items():                                     # alternating: drift of the shared host hits all three alike
            times[k].append(timed(f))
    ms = lambda v: 1e3 * v / args.batches            # noqa: E731
    rec = {'config': name, **cfg, 'batches': args.batches, 'reps': args.reps, 'epoch': epoch, 'math': gpe_amd.get_math(),
           'unit': 'ms per batch (host clock around a whole pass, ending in a device synchronise)',
           'none_keys': sorted(k for k, v in results['host'].items() if v is None),
           'replays_per_pass': evs['captured'].replays, 'captures_per_pass': evs['captured'].captures}
    for k, v in times.items():
        rec[k] = {'median': round(ms(statistics.median(v)), 4), 'min': round(ms(min(v)), 4), 'max': round(ms(max(v)), 4)}
    return rec


def measure_pool(args, dev):
    from gpe_amd import ops
    G, n_groups, P, L = args.pool_garments, 12, 23, 14
    g = torch.Generator().manual_seed(3)
    table = torch.zeros(G, 16, dtype=torch.float64)
    table[:, 0] = (torch.rand(G, generator=g) < 0.8).double()
    table[:, 1] = torch.rand(G, generator=g).float().double()
    table[:, 2], table[:, 3] = torch.rand(G, generator=g) * 5, torch.randint(3, 12, (G,), generator=g).double()
    table[:, 4], table[:, 5] = torch.rand(G, generator=g) * 3, torch.rand(G, generator=g) * 90
    table[:, 8] = (torch.rand(G, generator=g) < 0.9).double()
    table[:, 9], table[:, 10] = torch.rand(G, generator=g), torch.rand(G, generator=g).float().double()
    table[:, 11] = torch.randint(0, P * L + 1, (G,), generator=g).double()
    table = table.to(dev)
    group = torch.randint(0, n_groups, (G,), generator=g).int().to(dev)
    for _ in range(3):
        out = ops.quality_pool(table, group, n_groups, P, L, 63)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(args.pool_reps):
        e0.record()
        again = ops.quality_pool(table, group, n_groups, P, L, 63)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    assert torch.equal(out[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(out[1], again[1])
    return {'config': 'quality_pool', 'garments': G, 'groups': n_groups, 'reps': args.pool_reps,
            'unit': 'ms per call (device events around one launch)',
            'median': round(statistics.median(ts), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4),
            'table_MB': round(G * 16 * 8 / 1e6, 2)}


def _grid(nx, ny, bend):
    """nx x ny vertices on a bent sheet inside [-1, 1]^3, two triangles per cell"""
    u, v = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny), indexing='ij')
    verts = np.stack([0.9 * np.cos(bend * u) * (0.4 + 0.6 * u), 0.9 * np.sin(bend * u) * (0.4 + 0.6 * u), 1.6 * v - 0.8 + 0.1 * u], axis=-1)
    idx = np.arange(nx * ny).reshape(nx, ny)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)])
    return verts.reshape(-1, 3).astype(np.float32), faces.astype(np.int64)


def noise_levels(args, dev):
    """one sampler-fed pass per noise level (nn/evaluation_scripts/noise_levels.py): the sampler's point_noise_w is an attribute"""
    from gpe_amd import configs, evaluation, nets, staging
    cfg = CONFIGS['cfg1']
    data_config = configs.data_config()
    nn_cfg = configs.lstm_model_config(k_neighbors=cfg['k'])
    torch.manual_seed(0)
    model = nets.GarmentFullPattern3D(data_config, dict(nn_cfg), dict(nn_cfg['loss'])).to(dev).eval()
    meshes = []
    for m in range(32):
        v, f = _grid(20 + m, 12, 1.0 + 0.1 * m)
        meshes.append((v, f, np.arange(len(v)) % 5))
    sampler = staging.MeshPointSampler(meshes, None, mesh_samples=cfg['points'])
    gts = [b[1] for b in batches_for(cfg, 4, data_config, dev)]
    batches = [(torch.arange(8 * i, 8 * i + 8, device=dev), gts[i]) for i in range(4)]
    out = {}
    for w in args.noise:
        sampler.point_noise_w = float(w)
        torch.manual_seed(1)
        r = evaluation.eval_metrics(model, batches, sampler, epoch=args.epoch, seed=0)
        out[str(w)] = {k: (None if v is None else float(v)) for k, v in r.items()}
    return {'config': 'noise_levels', 'levels': out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', nargs='+', default=['cfg1', 'cfg2'], choices=sorted(CONFIGS))
    ap.add_argument('--batches', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--epoch', type=int, default=1000)
    ap.add_argument('--math', default='f16x3')
    ap.add_argument('--pool-garments', type=int, default=20000)
    ap.add_argument('--pool-reps', type=int, default=50)
    ap.add_argument('--noise', nargs='*', type=float, default=None, help='evaluate a sampler-fed pass per noise level instead')
    ap.add_argument('--out', default=None, help='also write the records to this JSON file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_bench.py times the MI355X: no GPU, no number')
    import gpe_amd
    dev = torch.device('cuda', 0)
    gpe_amd.set_math(args.math)
    if args.noise is not None:
        recs = [noise_levels(args, dev)]
    else:
        recs = [measure(c, CONFIGS[c], args, dev) for c in args.configs] + [measure_pool(args, dev)]
    for r in recs:
        print(json.dumps(r))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(recs, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

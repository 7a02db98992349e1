"""Times the guarded against the unguarded FusedAdam.step() on the arena of the BASELINE cfg-2 model (GarmentFullPattern3D,
k = 16): guarded = clipping + skip + per-parameter norms (one norm pass, one finish, the guarded Adam launch), unguarded = today's
single launch.  Both variants run in ONE process in alternating windows; the best of three windows each is reported with the
spread, as device time between events around the step and as host wall-clock per step.

    python scripts/adam_guard_bench.py [--iters 300] [--out profiles/adam_guard.md]

The gradient is copied in from a fixed random buffer in front of every step (outside the events): the step clears it."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('adam_guard_bench needs the MI355X: a CPU run cannot time anything')
    from gpe_amd import configs, nets, optim
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    nn_cfg = configs.lstm_model_config(k_neighbors=16)
    model = nets.GarmentFullPattern3D(configs.data_config(), dict(nn_cfg), dict(nn_cfg['loss'])).to(dev).train()
    arena = optim.FlatArena(model)
    opts = {'unguarded': optim.FusedAdam(arena, lr=2e-3),
            'guarded': optim.FusedAdam(arena, lr=2e-3, max_grad_norm=1.0, skip_nonfinite=True, param_grad_norms=True)}
    gsrc = torch.randn(arena.numel, device=dev) * 1e-3
    for o, p in zip(arena.offsets, arena.params):                      # padding floats are zero
        gsrc[o + p.numel():o + (p.numel() + 3) // 4 * 4] = 0

    def window(opt, iters):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for e0, e1 in ev:
            arena.grad.copy_(gsrc)
            e0.record()
            opt.step()
            e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / iters
        return sum(e0.elapsed_time(e1) for e0, e1 in ev) / iters * 1e3, wall * 1e6

    for opt in opts.values():                                          # warm-up: code objects, the lane, the allocator
        window(opt, 20)
    res = {k: [] for k in opts}
    for _ in range(args.windows):
        for name, opt in opts.items():                                 # alternating windows
            res[name].append(window(opt, args.iters))
    g = opts['guarded']
    lines = ['# Guarded against unguarded FusedAdam.step(), cfg-2 arena', '',
             'Arena: %d parameters, %d floats (%.1f MB of gradient read once by the norm pass, %d slots of 2048 floats).'
             % (len(arena.params), arena.numel, arena.numel * 4 / 1e6, g._nslots),
             'One process, alternating windows of %d steps, %d windows each; device = time between events around step(), host = '
             'wall-clock per step including the gradient copy that precedes it.  Last guarded step: norm %.6g, factor %.6g, skipped %d.'
             % (args.iters, args.windows, g.grad_norm.item(), g.clip_coef.item(), g.skipped.item()), '',
             '| variant | launches | device us/step: best | windows | host us/step: best | windows |', '|---|---|---|---|---|---|']
    best = {}
    for name, launches in (('unguarded', 1), ('guarded', 3)):
        d, w = [r[0] for r in res[name]], [r[1] for r in res[name]]
        best[name] = (min(d), max(d) - min(d), min(w))
        lines.append('| %s | %d | %.2f | %s | %.2f | %s |' % (name, launches, min(d), ' / '.join('%.2f' % v for v in d), min(w),
                                                            ' / '.join('%.2f' % v for v in w)))
    diff = best['guarded'][0] - best['unguarded'][0]
    spread = max(best['guarded'][1], best['unguarded'][1])
    lines += ['', 'Guard cost on the device: %.2f us per step (best against best); spread of the windows %.2f us: the difference is %s '
              'the spread.  Host: %.2f us per step.' % (diff, spread, 'INSIDE' if abs(diff) <= spread else 'outside',
                                                       best['guarded'][2] - best['unguarded'][2])]
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()

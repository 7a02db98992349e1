"""The guarded Adam step on the device (include/gpe_hip_ext.h; optim.FusedAdam's max_grad_norm / skip_nonfinite / guard_overflow /
param_grad_norms):
  (1) the norm pass against float64 torch: accuracy, zero and huge gradients, non-finite values, watched words, reproducibility;
  (1b) the guarded Adam kernel with the factor at 1 against gpe_adam_step, bit for bit, float4 body and every tail length;
  (2) no trigger = the unguarded step, bit for bit;  (3) clipping against float64 clip_grad_norm_ + Adam + OneCycleLR;
  (4) a poisoned gradient is skipped and the step numbers go on;  (5) the same inside a captured step;
  (6) the fp16-activation window: the step that ran on clamped values is not applied.
Tolerances: a norm is fp64 accumulation plus one rounding to fp32, held to 2^-22 relative against float64 torch on the same
gradient."""
import copy
import ctypes
import os
import warnings

import pytest
import torch

import adam_guard_restate as AG

pytestmark = pytest.mark.gpu

SLOT = 2048
EPS22 = 2.0 ** -22


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def f32(x):
    """the nearest fp32 value (what a float argument of the C ABI becomes)"""
    return torch.tensor(float(x), dtype=torch.float64).float().item()


def _bits(x):
    return torch.tensor([x], dtype=torch.float32).view(torch.int32).cuda()


class NormPass:
    """The two launches of the norm pass over segments of `sizes` floats (padded to fours), driven through the C ABI."""

    def __init__(self, gpe, sizes):
        self.L = gpe._lib
        self.sizes = list(sizes)
        self.padded = [(s + 3) // 4 * 4 for s in sizes]
        self.nseg = len(sizes)
        ends, off = [], 0
        for p in self.padded:
            off += p
            ends.append(off)
        self.starts, self.ends, self.n = [e - p for e, p in zip(ends, self.padded)], ends, off
        c_slots = (ctypes.c_long * (self.nseg + 1))()
        self.total = self.L.query('gpe_grad_norm_slots', (ctypes.c_long * self.nseg)(*ends), self.nseg, c_slots)
        assert self.total == sum((p + SLOT - 1) // SLOT for p in self.padded)
        self.seg_end = torch.tensor(ends, dtype=torch.int64).cuda()
        self.seg_slot = torch.tensor(list(c_slots), dtype=torch.int64).cuda()
        self.part = torch.full((self.total,), float('nan'), dtype=torch.float64).cuda()
        self.blk = torch.zeros(8, dtype=torch.int32).cuda()
        self.seg_norm = torch.full((self.nseg,), -1.0).cuda()

    def fill(self, gen, scale=1.0):
        """a gradient with zero padding floats"""
        g = torch.zeros(self.n)
        for s, n in zip(self.starts, self.sizes):
            g[s:s + n] = torch.randn(n, generator=gen) * scale
        return g.cuda()

    def run(self, g, gscale=1.0, max_norm=0.0, nonfinite=1, words=(), limit=65504.0, runs=None, reversed_=0):
        runs = runs or [(0, self.nseg)]
        for lo, hi in runs:
            self.L.call('gpe_grad_norm_part', g, self.n, self.seg_end, self.seg_slot, self.nseg, lo, hi, self.total, self.part)
        c_runs = (ctypes.c_int * (2 * len(runs)))(*[j for r in runs for j in r])
        c_words = (ctypes.c_void_p * max(len(words), 1))(*[w.data_ptr() for w in words])
        self.L.call('gpe_grad_norm_finish', self.part, self.seg_slot, self.nseg, self.total, c_runs, len(runs), float(gscale),
                    float(max_norm), int(nonfinite), c_words, len(words), float(limit), self.seg_norm, reversed_, self.blk)
        torch.cuda.synchronize()
        b = self.blk.cpu()
        return {'norm': b[0:1].view(torch.float32)[0].item(), 'coef': b[1:2].view(torch.float32)[0].item(), 'skip': int(b[2]),
                'steps': int(b[4:6].view(torch.int64)[0]), 'skipped': int(b[6:8].view(torch.int64)[0]), 'bits': b[:3].clone(),
                'seg': self.seg_norm.cpu().clone()}

    def reference(self, g, gscale=1.0, live=None):
        g64 = g.double().cpu()
        segs = [g64[s:s + p] for s, p in zip(self.starts, self.padded)]
        total, seg = AG.norms([x for j, x in enumerate(segs) if live is None or j in live], gscale)
        return float(total), [float(v) for v in seg]


# the issue's segment sizes; n = 4; exactly one slot, and one float4 past the slot boundary; a last workgroup that is partly empty
SIZE_SETS = [[1, 3, 4, 5, 150, 3200, 1], [1], [SLOT], [SLOT + 4], [3 * SLOT + 4], [5 * SLOT + 1001, 7, 2 * SLOT, 2]]


@pytest.mark.parametrize('sizes', SIZE_SETS, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('gscale', [1.0, -0.5])
def test_norm_pass_matches_float64_torch(gpe, sizes, gscale):
    npass = NormPass(gpe, sizes)
    g = npass.fill(torch.Generator().manual_seed(len(sizes)), scale=3.0)
    total, seg = npass.reference(g, gscale)
    half = f32(total / 2)
    out = npass.run(g, gscale=gscale, max_norm=half)
    print('norm %.9g vs %.9g; worst segment %.3g of 2^-22' % (out['norm'], total, max(abs(a - b) / b for a, b in zip(out['seg'].tolist(), seg)) / EPS22))
    assert abs(out['norm'] - total) <= EPS22 * total
    for j, (a, b) in enumerate(zip(out['seg'].tolist(), seg)):
        assert abs(a - b) <= EPS22 * b, j
    assert out['coef'] == f32(AG.factor(out['norm'], half)) and 0.49 < out['coef'] < 0.51 and out['skip'] == 0 and (out['steps'], out['skipped']) == (1, 0)
    # clipping off: the factor is exactly 1; a threshold above the norm as well; model.parameters() order on request
    off = npass.run(g, gscale=gscale, max_norm=0.0, reversed_=1)
    assert off['coef'] == 1.0 and off['norm'] == out['norm'] and torch.equal(off['seg'], out['seg'].flip(0))
    assert npass.run(g, gscale=gscale, max_norm=total * 1.01)['coef'] == 1.0


def test_norm_pass_zero_huge_and_dead_segments(gpe):
    npass = NormPass(gpe, SIZE_SETS[0])
    z = torch.zeros(npass.n).cuda()
    out = npass.run(z, max_norm=1.0)
    assert out['norm'] == 0.0 and out['coef'] == 1.0 and out['skip'] == 0 and not out['seg'].any()
    # 1e25: the squares overflow fp32, the norm does not
    big = torch.zeros(npass.n)
    for s, n in zip(npass.starts, npass.sizes):
        big[s:s + n] = 1e25
    big = big.cuda()
    total, seg = npass.reference(big)
    out = npass.run(big, max_norm=1.0)
    assert abs(out['norm'] - total) <= EPS22 * total and out['skip'] == 0 and 0 < out['coef'] < 1e-25
    # ... and a norm that does not fit fp32 is not finite
    assert npass.run(big, gscale=1e13)['skip'] == 1 and npass.run(big, gscale=1e13, nonfinite=0)['skip'] == 0
    # several runs, ONE norm; segments outside every run are dead: norm 0, no contribution (their stale slots are not read)
    g = npass.fill(torch.Generator().manual_seed(2))
    npass.run(g)
    g2 = g.clone()
    g2[npass.starts[2]:npass.ends[3]] = float('nan')                 # dead segments may hold anything
    live = [0, 1, 4, 5, 6]
    total, seg = npass.reference(g2, live=live)
    out = npass.run(g2, runs=[(0, 2), (4, 7)])
    assert abs(out['norm'] - total) <= EPS22 * total and out['skip'] == 0
    assert out['seg'][2] == 0 and out['seg'][3] == 0
    for j, b in zip(live, seg):
        assert abs(out['seg'][j].item() - b) <= EPS22 * b


@pytest.mark.parametrize('value', [float('inf'), float('nan')])
def test_norm_pass_flags_non_finite_values(gpe, value):
    npass = NormPass(gpe, SIZE_SETS[0])
    g = npass.fill(torch.Generator().manual_seed(3))
    # the first element, the last element (size-1 segment: beside three padding floats), the float beside a padding float
    spots = [0, npass.starts[-1], npass.starts[1] + 2]
    assert npass.padded[1] == 4 and npass.sizes[1] == 3
    skipped = 0
    for spot in spots:
        bad = g.clone()
        bad[spot] = value
        out = npass.run(bad)
        assert out['skip'] == 1 and not torch.isfinite(torch.tensor(out['norm'])), spot
        skipped += 1
        assert out['skipped'] == skipped
        quiet = npass.run(bad, nonfinite=0)
        assert quiet['skip'] == 0 and quiet['skipped'] == skipped
    assert npass.run(g)['skip'] == 0


def test_norm_pass_watched_words(gpe):
    npass = NormPass(gpe, SIZE_SETS[0])
    g = npass.fill(torch.Generator().manual_seed(4))
    ok, at, nan = _bits(65503.9), _bits(65504.0), _bits(float('nan'))
    assert npass.run(g, words=[ok])['skip'] == 0
    assert npass.run(g, words=[ok, at])['skip'] == 1 and npass.run(g, words=[at], nonfinite=0)['skip'] == 1
    assert npass.run(g, words=[nan, ok])['skip'] == 1
    assert npass.run(g, words=[ok] * 8)['skip'] == 0 and npass.run(g, words=[ok] * 7 + [at])['skip'] == 1
    out = npass.run(g, words=[_bits(3.0)], limit=2.0)
    assert out['skip'] == 1 and out['skipped'] == 5 and out['steps'] == 7


def test_norm_pass_is_reproducible(gpe):
    """bit-identical on a second call and under another CU reservation: 1200 slots, more than the grid at either reservation"""
    npass = NormPass(gpe, [1100 * SLOT - 40, 36, 100 * SLOT, 3])
    assert npass.total > 4 * 256
    g = npass.fill(torch.Generator().manual_seed(5))
    total, seg = npass.reference(g)
    first = npass.run(g, max_norm=1.0)
    assert abs(first['norm'] - total) <= EPS22 * total
    again = npass.run(g, max_norm=1.0)
    prev = gpe.set_reserved_cus(16)
    try:
        reserved = npass.run(g, max_norm=1.0)
    finally:
        gpe.set_reserved_cus(prev)
    for other in (again, reserved):
        assert torch.equal(other['bits'], first['bits']) and torch.equal(other['seg'], first['seg'])


@pytest.mark.parametrize('weight_decay', [0.0, 1e-4])
@pytest.mark.parametrize('n', [1024, 1021, 1022, 1023])
def test_guarded_kernel_repeats_the_unguarded_roundings(gpe, n, weight_decay):
    """factor 1, flag clear: p, m, v bit-equal to gpe_adam_step — the float4 body and tails of one, two and three elements"""
    L = gpe._lib
    gen = torch.Generator().manual_seed(n)
    p0, m0 = torch.randn(n, generator=gen).cuda(), (torch.randn(n, generator=gen) * 0.1).cuda()
    v0, g0 = (torch.rand(n, generator=gen) * 0.01).cuda(), torch.randn(n, generator=gen).cuda()
    blk = torch.zeros(8, dtype=torch.int32).cuda()
    blk[1:2] = _bits(1.0)
    for gscale, step in ((1.0, 1), (0.37, 7)):
        a = [t.clone() for t in (p0, g0, m0, v0)]
        b = [t.clone() for t in (p0, g0, m0, v0)]
        L.call('gpe_adam_step', *a, n, 2e-3, 0.9, 0.999, 1e-8, weight_decay, step, gscale, 1)
        L.call('gpe_adam_step_guarded', *b, n, 2e-3, 0.9, 0.999, 1e-8, weight_decay, step, gscale, 1, blk)
        torch.cuda.synchronize()
        for name, x, y in zip('pgmv', a, b):
            assert torch.equal(x, y), (name, gscale, (x != y).nonzero().flatten()[:8].tolist())
        assert not b[1].any() and not torch.equal(a[0], p0)
    # the flag set: nothing moves, the gradient is cleared (or kept when zero_grad == 0)
    blk[2] = 1
    for zero in (1, 0):
        b = [t.clone() for t in (p0, g0, m0, v0)]
        L.call('gpe_adam_step_guarded', *b, n, 2e-3, 0.9, 0.999, 1e-8, weight_decay, 3, 1.0, zero, blk)
        torch.cuda.synchronize()
        assert torch.equal(b[0], p0) and torch.equal(b[2], m0) and torch.equal(b[3], v0)
        assert (not b[1].any()) if zero else torch.equal(b[1], g0)


def _two_linears(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(37, 50), torch.nn.Linear(50, 3)).cuda()


@pytest.mark.parametrize('weight_decay', [0.0, 1e-4])
@pytest.mark.parametrize('grad_scale', [1.0, 0.5])
def test_no_trigger_is_the_unguarded_step(gpe, weight_decay, grad_scale):
    L = gpe._lib
    net_a = _two_linears()
    net_b = copy.deepcopy(net_a)
    opt_a = gpe.optim.FusedAdam(net_a, lr=2e-3, weight_decay=weight_decay)
    opt_b = gpe.optim.FusedAdam(net_b, lr=2e-3, weight_decay=weight_decay, max_grad_norm=1e9)
    assert not opt_a.guarded and opt_a.grad_norm is None and opt_b.guarded and opt_b.param_norms is None
    gen = torch.Generator().manual_seed(1)
    for step in range(3):
        x = torch.randn(16, 37, generator=gen).cuda()
        for net, opt in ((net_a, opt_a), (net_b, opt_b)):
            net(x).square().mean().backward()
            L.TIMING = []
            try:
                opt.step(grad_scale=grad_scale)
                names = [t[0] for t in L.TIMING]
            finally:
                L.TIMING = None
            # the launch budget: defaults = today's one launch; guarded = one pass per run + one finish in front of it
            assert names == (['gpe_grad_norm_part', 'gpe_grad_norm_finish', 'gpe_adam_step_guarded'] if opt.guarded else ['gpe_adam_step'])
        torch.cuda.synchronize()
        assert torch.equal(opt_a.arena.flat, opt_b.arena.flat) and torch.equal(opt_a.m, opt_b.m) and torch.equal(opt_a.v, opt_b.v)
        assert not opt_b.arena.grad.any() and not opt_a.arena.grad.any()
        assert opt_b.clip_coef.item() == 1.0 and opt_b.last_skipped.item() == 0 and opt_b.grad_norm.item() > 0
    assert opt_b.skipped.item() == 0 and opt_a.arena.flat.abs().sum().item() > 0


def test_clipping_vs_torch_float64(gpe):
    """the net and schedule of test_fused_adam_onecycle_vs_torch under a threshold of half the first step's norm: steps 1 - 11 clip
    (factor 0.50 .. 0.74); the norm has fallen to 0.92 of the threshold by step 12, which runs with the factor at exactly 1"""
    net = _two_linears()
    ref = copy.deepcopy(net).double()
    gen = torch.Generator().manual_seed(1)
    xs = [torch.randn(16, 37, generator=gen) for _ in range(12)]
    ref(xs[0].cuda().double()).square().mean().backward()
    max_norm = f32(0.5 * AG.norms([p.grad for p in ref.parameters()])[0].item())
    for p in ref.parameters():
        p.grad = None
    opt = gpe.optim.FusedAdam(net, lr=2e-3, weight_decay=1e-4, schedule=gpe.optim.OneCycle(2e-3, 40), max_grad_norm=max_norm,
                              param_grad_norms=True)
    ropt = torch.optim.Adam(ref.parameters(), lr=2e-3, weight_decay=1e-4)
    rs = torch.optim.lr_scheduler.OneCycleLR(ropt, max_lr=2e-3, epochs=4, steps_per_epoch=10, cycle_momentum=False)
    worst = worst_own = 0.0
    clipped = 0
    for step, x in enumerate(xs):
        net(x.cuda()).square().mean().backward()
        ref(x.cuda().double()).square().mean().backward()
        own, own_seg = AG.norms([p.grad for p in net.parameters()])          # float64 torch on the gradient the pass reads
        opt.step()
        rnorm = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm).item()
        ropt.step()
        rs.step()
        ropt.zero_grad()
        got = opt.grad_norm.item()
        worst, worst_own = max(worst, abs(got - rnorm) / rnorm), max(worst_own, abs(got - own.item()) / own.item())
        print('step %2d: grad_norm %.9g, float64 net %.9g (%.3g of 2^-22), float64 of the same gradient %.9g (%.3g of 2^-22)'
              % (step, got, rnorm, abs(got - rnorm) / rnorm / EPS22, own.item(), abs(got - own.item()) / own.item() / EPS22))
        assert (opt.clip_coef.item() < 1.0) == (rnorm + 1e-6 > max_norm)
        clipped += opt.clip_coef.item() < 1.0
        assert abs(got - own.item()) <= EPS22 * own.item()
        assert abs(got - rnorm) <= EPS22 * rnorm
        assert opt.clip_coef.item() == f32(AG.factor(got, max_norm))
        for a, b in zip(opt.param_norms.tolist(), own_seg):                    # model.parameters() order
            assert abs(a - b.item()) <= EPS22 * b.item()
        assert not opt.arena.grad.any() and opt.last_skipped.item() == 0
    assert clipped >= 10 and opt.arena.flat.isfinite().all()
    for p, q in zip(net.parameters(), ref.parameters()):
        assert relerr(p, q) < 1e-5
    print('worst |grad_norm - reference| / reference: float64 net %.3g, same gradient %.3g (2^-22 = %.3g)' % (worst, worst_own, EPS22))


def test_poisoned_gradient_is_skipped_and_step_numbers_go_on(gpe):
    """NaN written into arena.grad between backward() and step() at step 3 of 5: that step changes nothing but the gradient, and
    steps 4 and 5 run with the scalars of steps 4 and 5 (the restatement on the same gradients; one that rewinds does not fit)"""
    net = _two_linears(seed=2)
    sched = gpe.optim.OneCycle(2e-2, 40)
    kw = dict(lr=2e-2, weight_decay=1e-4, max_grad_norm=0.0625, skip_nonfinite=True)
    opt = gpe.optim.FusedAdam(net, schedule=sched, **kw)
    a = opt.arena
    params = [p for p in net.parameters()]
    rest = AG.GuardedAdam64(params, lr_of_step=sched.lr, **kw)
    rewound = AG.GuardedAdam64(params, lr_of_step=sched.lr, **kw)        # the rule this code does NOT follow: a skip rewinds
    gen = torch.Generator().manual_seed(3)
    for step in range(1, 6):
        net(torch.randn(16, 37, generator=gen).cuda()).square().mean().backward()
        if step == 3:
            a.grad[a.offsets[1] + 1] = float('nan')
        grads = [p.grad.clone() for p in params]
        before = (a.flat.clone(), opt.m.clone(), opt.v.clone())
        opt.step()
        rest.step(grads)
        if step != 3:
            rewound.step(grads)
        torch.cuda.synchronize()
        assert not a.grad.any()                                            # cleared, the poisoned one too
        if step == 3:
            assert all(torch.equal(x, y) for x, y in zip(before, (a.flat, opt.m, opt.v)))
            assert opt.last_skipped.item() == 1 and rest.last_skipped
        else:
            assert opt.last_skipped.item() == 0 and not torch.equal(before[0], a.flat)
            assert abs(opt.grad_norm.item() - float(rest.norm)) <= EPS22 * float(rest.norm)
        assert opt.skipped.item() == (step >= 3)
    assert opt.t == 5 and opt.steps == [5] * len(a.params) and rest.t == 5 and rewound.t == 4
    # fp32 against fp64 on the same gradients over four applied steps: per step one rounding of p (2^-24 |p|) and ~10 roundings of
    # an update of at most ~3 lr (lr <= 2e-3 here) — below 1e-6 of max |p|; a rewound step number changes the bias corrections of
    # steps 4 and 5 by ~10 % of an update each, ~1e-3 of max |p|
    for p, q, r in zip(params, rest.p, rewound.p):
        print('fp32 vs the restatement %.3g; vs a restatement that rewinds %.3g' % (relerr(p, q), relerr(p, r)))
        assert relerr(p, q) < 1e-6
        assert relerr(p, r) > 1e-5
    sd = opt.state_dict()                                                  # torch's layout, unchanged: the skipped step counts
    assert all(float(s['step']) == 5 for s in sd['state'].values()) and set(sd) == {'state', 'param_groups'}


def test_captured_guarded_step_replays_the_eager_steps(gpe, golden_dir):
    """StitchOnEdge3DPairs at the shape of tests/golden/stitch_train_small.pt; the loss is multiplied by an input scalar that is inf
    at step 5: non-finite gradients from a finite forward.  Seven steps through StepGraph = seven eager guarded steps, bit for bit."""
    from gpe_amd import optim, graph
    fx = torch.load(os.path.join(golden_dir, 'stitch_train_small.pt'), weights_only=False)
    pairs, labels = fx['pairs'].cuda(), fx['labels'].cuda()
    assert tuple(pairs.shape[1:]) == (271, 12) and fx['nn_config'] == {'stitch_hidden_size': 72, 'stitch_mlp_n_layers': 2}
    torch.manual_seed(11)
    model_a = gpe.nets.StitchOnEdge3DPairs(fx['data_config'], dict(fx['nn_config']), {}).cuda().train()
    model_b = copy.deepcopy(model_a)
    kw = dict(lr=2e-3, max_grad_norm=0.02, skip_nonfinite=True, param_grad_norms=True)
    opt_a = optim.FusedAdam(optim.FlatArena(model_a), schedule=optim.OneCycle(2e-3, 40), **kw)
    opt_b = optim.FusedAdam(optim.FlatArena(model_b), schedule=optim.OneCycle(2e-3, 40), **kw)

    def forward_loss(model):
        return lambda f, g, s: model.loss(model(f), g)[0] * s

    def snap(opt, loss):
        return [loss.detach().clone(), opt.arena.flat.clone(), opt.m.clone(), opt.v.clone(), opt.grad_norm.clone(),
                opt.param_norms.clone(), opt.skipped.clone(), opt.last_skipped.clone(), opt.clip_coef.clone()]

    scales = [torch.tensor([float('inf') if i == 5 else 1.0]).cuda() for i in range(1, 8)]
    eager, replayed = [], []
    fa = forward_loss(model_a)
    for s in scales:
        loss = fa(pairs, labels, s)
        loss.backward()
        opt_a.step()
        eager.append(snap(opt_a, loss))
    sg = graph.StepGraph(forward_loss(model_b), opt_b, warmup=2)
    for s in scales:
        loss = sg.step(pairs, labels, s)
        replayed.append(snap(opt_b, loss))
    sg.synchronize()
    torch.cuda.synchronize()
    assert sg.captures == 1 and sg.replays == 5
    names = ('loss', 'parameters', 'exp_avg', 'exp_avg_sq', 'grad_norm', 'param_norms', 'skipped', 'last_skipped', 'clip_coef')
    for i, (ea, rp) in enumerate(zip(eager, replayed)):
        for name, x, y in zip(names, ea, rp):
            assert torch.equal(x, y) or (name in ('loss', 'grad_norm', 'param_norms') and i == 4 and
                                           torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(x.nan_to_num(), y.nan_to_num())), (i, name)
    assert [int(e[6]) for e in eager] == [0, 0, 0, 0, 1, 1, 1] and [int(e[7]) for e in eager] == [0, 0, 0, 0, 1, 0, 0]
    for k in (1, 2, 3):                                                # the parameters and moments after step 5 are those after step 4
        assert torch.equal(eager[4][k], eager[3][k]) and torch.equal(replayed[4][k], replayed[3][k])
    assert not torch.equal(eager[5][1], eager[4][1]) and not torch.equal(eager[3][1], eager[2][1])
    assert all(e[8].item() < 1.0 for i, e in enumerate(eager) if i != 4)          # every applied step clipped
    assert torch.isfinite(eager[6][1]).all() and torch.isfinite(eager[6][4])
    for (n, p), q in zip(model_a.named_buffers(), model_b.buffers()):
        assert torch.equal(p, q) and torch.isfinite(p.float()).all(), n
    assert opt_a.t == opt_b.t == 7 and opt_a.steps == opt_b.steps and opt_a.last_lr == opt_b.last_lr


# ---- the fp16-activation window -----------------------------------------------------------------------------------------------
def _conv(gpe, scale_last=1.0, seed=5):
    """the conv of test_half_activation_guard: 3 -> 200 -> 150, k = 16, non-trivial BatchNorm affines with negative scales"""
    from oracle import ref_path as O
    C, H, Fo, k = 3, 200, 150, 16
    torch.manual_seed(seed)
    oconv = O.DynamicEdgeConv(O.MLP([2 * C, H, H, Fo]), k=k)
    with torch.no_grad():
        for blk in oconv.nn:
            blk[2].weight.uniform_(0.5, 1.5)
            blk[2].bias.uniform_(-0.3, 0.3)
        oconv.nn[2][2].weight[::5] *= -1
        oconv.nn[2][0].weight *= scale_last
    pconv = gpe.net_blocks.DynamicEdgeConv(gpe.net_blocks.MLP([2 * C, H, H, Fo]), k=k)
    pconv.load_state_dict(oconv.state_dict())
    return pconv.cuda().train()


@pytest.fixture
def f16x3_fallback(gpe):
    prev = gpe.set_math('f16x3')
    mode0 = gpe.ops.set_half_act_guard('fallback')
    yield
    gpe.ops.set_half_act_guard(mode0)
    gpe.set_math(prev)


B_, N_, K_ = 8, 512, 16


def _conv_data():
    g = torch.Generator().manual_seed(6)
    return torch.randn(B_ * N_, 3, generator=g).cuda(), torch.randn(B_ * N_, 150, generator=g).cuda()


def test_half_activation_window_eager(gpe, f16x3_fallback):
    ops, optim, L = gpe.ops, gpe.optim, gpe._lib
    assert L.query('gpe_edge_lazy_dz3_ok', B_, N_, K_, 150, 200) == 1
    x, wgt = _conv_data()
    conv = _conv(gpe)
    opt = optim.FusedAdam(optim.FlatArena(conv), lr=1e-3, guard_overflow=True)
    a = opt.arena

    def step():
        (conv(x, B_, N_) * wgt).sum().backward()
        nwords = len(ops.watched_words(x.device))
        before = (a.flat.clone(), opt.m.clone(), opt.v.clone())
        opt.step()
        torch.cuda.synchronize()
        assert ops.watched_words(x.device) == []
        return nwords, all(torch.equal(p, q) for p, q in zip(before, (a.flat, opt.m, opt.v)))

    # a layer in range is never skipped (its word is watched all the same)
    for _ in range(2):
        assert step() == (1, False)
    assert opt.skipped.item() == 0 and not conv.half_act_guard.disabled and opt.m.any()
    # the last Linear x 1e5 in place: the step that runs on clamped values changes nothing
    with torch.no_grad():
        conv.nn[2][0].weight *= 1e5
    ops.bump_weights_epoch()
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter('always')
        assert step() == (1, True)
    assert opt.skipped.item() == 1 and opt.last_skipped.item() == 1 and not a.grad.any()
    assert not any('fp16 storage' in str(w.message) for w in wl)
    # one step late the guard itself notices: it warns, stores fp32 rows — and that step IS applied
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter('always')
        assert step() == (0, False)
    assert conv.half_act_guard.disabled and any('fp16 storage' in str(w.message) for w in wl)
    assert opt.skipped.item() == 1 and opt.last_skipped.item() == 0 and opt.t == 4


def test_half_activation_window_captured(gpe, f16x3_fallback):
    ops, optim, graph = gpe.ops, gpe.optim, gpe.graph
    x, wgt = _conv_data()
    conv = _conv(gpe)
    opt = optim.FusedAdam(optim.FlatArena(conv), lr=1e-3, guard_overflow=True)
    a = opt.arena
    sg = graph.StepGraph(lambda f, w: (conv(f, B_, N_) * w).sum(), opt, warmup=2)

    def step():
        before = a.flat.clone()
        sg.step(x, wgt)
        sg.synchronize()
        torch.cuda.synchronize()
        return torch.equal(before, a.flat)

    for _ in range(4):                                                  # two eager steps, the capture, one more replay: all applied
        assert not step()
    assert (sg.captures, sg.replays) == (1, 2) and opt.skipped.item() == 0 and len(sg.guards) == 1
    with torch.no_grad():
        conv.nn[2][0].weight *= 1e5
    ops.bump_weights_epoch()
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter('always')
        assert step()                                                   # the tripping replay: the weights are bit-identical
        assert opt.skipped.item() == 1 and opt.last_skipped.item() == 1 and sg.captures == 1
        # the guard's own poll goes on as before: it sees the word of that replay one poll later (a replay that is skipped as
        # well), and the graph is then captured again on fp32 rows — a step that is applied
        more = 0
        while sg.graph is not None:
            assert step() and more < 2
            more += 1
        assert opt.skipped.item() == 1 + more and conv.half_act_guard.disabled
        assert not step()
    assert any('fp16 storage' in str(w.message) for w in wl)
    assert sg.captures == 2 and sg.guards == [] and opt.skipped.item() == 1 + more and opt.last_skipped.item() == 0
    assert opt.t == 6 + more


def test_guard_overflow_refuses_more_than_one_rank(gpe, monkeypatch):
    net = _two_linears()
    opt = gpe.optim.FusedAdam(net, guard_overflow=True)
    net(torch.randn(4, 37).cuda()).sum().backward()
    monkeypatch.setattr(torch.distributed, 'is_initialized', lambda: True)
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda *a: 2)
    with pytest.raises(RuntimeError, match='local to a rank'):
        opt.step()

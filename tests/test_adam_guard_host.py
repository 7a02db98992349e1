"""not-gpu: the guarded Adam step (include/gpe_hip_ext.h, optim.FusedAdam's max_grad_norm / skip_nonfinite / guard_overflow /
param_grad_norms) as far as it goes without a device:
  (1) the fp64 restatement (tests/adam_guard_restate.py) agrees with torch's clip_grad_norm_ + torch.optim.Adam + OneCycleLR in
      float64 over 8 steps, one of them skipped (a skipped step keeps its number);
  (2) both headers are bound, every symbol of gpe_hip_ext.h is exported, and the default parse_header() is still the main header;
  (3) the new entry points refuse bad arguments before any launch;
  (4) FusedAdam's new options default to the unguarded path and are validated."""
import ctypes
import inspect
import math

import pytest
import torch

import gpe_amd
from gpe_amd import _lib, optim
import adam_guard_restate as AG

EXT = ('gpe_grad_norm_slots', 'gpe_grad_norm_part', 'gpe_grad_norm_finish', 'gpe_adam_step_guarded', 'gpe_adam_step_guarded_dev')


@pytest.mark.parametrize('weight_decay', [0.0, 1e-4])
def test_restatement_agrees_with_torch_float64(weight_decay):
    torch.manual_seed(3)
    shapes = [(5, 3), (3,), (7, 2), (1,)]
    params = [torch.randn(s, dtype=torch.float64) for s in shapes]
    tparams = [torch.nn.Parameter(p.clone()) for p in params]
    topt = torch.optim.Adam(tparams, lr=2e-3, weight_decay=weight_decay)
    tsched = torch.optim.lr_scheduler.OneCycleLR(topt, max_lr=2e-3, epochs=4, steps_per_epoch=10, cycle_momentum=False)
    sched = optim.OneCycle(2e-3, 40)
    max_norm = 2.0
    ours = AG.GuardedAdam64(params, lr=2e-3, weight_decay=weight_decay, max_grad_norm=max_norm, skip_nonfinite=True,
                            lr_of_step=sched.lr)
    g = torch.Generator().manual_seed(4)
    clipped = 0
    for step in range(8):
        # magnitudes either side of the threshold: some steps clip, some do not
        grads = [torch.randn(s, generator=g, dtype=torch.float64) * (0.05 if step % 2 else 3.0) for s in shapes]
        if step == 4:
            grads[2][3, 1] = float('nan')
        ours.step(grads)
        if step == 4:
            # torch's side of a skipped step: no optimizer step, every parameter's step count advances, the scheduler steps
            assert ours.last_skipped and not math.isfinite(float(ours.norm))
            for p in tparams:
                topt.state[p]['step'] += 1
        else:
            for p, gr in zip(tparams, grads):
                p.grad = gr.clone()
            tnorm = torch.nn.utils.clip_grad_norm_(tparams, max_norm)
            assert abs(float(ours.norm) - float(tnorm)) <= 1e-12 * float(tnorm)
            assert not ours.last_skipped
            clipped += ours.coef < 1.0
            for p, gr in zip(tparams, grads):                # torch scaled the gradients in place by our factor
                assert torch.allclose(p.grad, gr * ours.coef, rtol=1e-13, atol=0)
            topt.step()
        tsched.step()
    assert 0 < clipped < 7 and ours.skipped == 1 and ours.t == 8
    for p, q in zip(ours.p, tparams):
        assert (p - q.detach()).abs().max().item() <= 1e-12
    for i, q in enumerate(tparams):
        st = topt.state[q]
        assert float(st['step']) == 8
        assert (ours.m[i] - st['exp_avg']).abs().max().item() <= 1e-12
        assert (ours.v[i] - st['exp_avg_sq']).abs().max().item() <= 1e-12


def test_restatement_rules():
    g = [torch.tensor([3.0, 0.0]), torch.tensor([4.0])]
    total, seg = AG.norms(g, gscale=-0.5)
    assert float(total) == 2.5 and [float(s) for s in seg] == [1.5, 2.0]
    assert AG.factor(2.5, None) == 1.0 and AG.factor(2.5, 0.0) == 1.0 and AG.factor(2.5, 10.0) == 1.0
    assert AG.factor(2.5, 1.0) == 1.0 / (2.5 + 1e-6)
    assert not AG.skip_rule(float('inf'), False) and AG.skip_rule(float('inf'), True) and AG.skip_rule(float('nan'), True)
    assert AG.skip_rule(1.0, False, [1.0, 65504.0]) and AG.skip_rule(1.0, False, [float('nan')])
    assert not AG.skip_rule(1.0, True, [65503.9])


def test_both_headers_are_bound_and_exported():
    main, ext = _lib.parse_header(), _lib.parse_header(_lib.EXT_HEADER_PATH)
    assert len(main) == 123 and not set(main) & set(ext)          # the default path is still the main header
    assert set(ext) == set(EXT)
    assert _lib.HEADERS == (_lib.HEADER_PATH, _lib.EXT_HEADER_PATH)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ext:
        assert hasattr(raw, name), 'libgpe_hip.so does not export %s' % name
    l = _lib.lib()
    assert l.gpe_abi_version() == 7
    for name, (res, args) in ext.items():
        fn = getattr(l, name)
        assert fn.restype is _lib._CT[res] and list(fn.argtypes) == [_lib._CT[a] for a in args], name
        if name != 'gpe_grad_norm_slots':
            assert res == 'i' and args[-1] == 'p', name


def test_a_declared_symbol_that_is_not_exported_fails_loudly(tmp_path, monkeypatch):
    h = tmp_path / 'ext.h'
    h.write_text('int gpe_not_in_the_library(const float* x, void* stream);\n')
    monkeypatch.setattr(_lib, 'HEADERS', (_lib.HEADER_PATH, str(h)))
    monkeypatch.setattr(_lib, '_lib', None)
    with pytest.raises(AttributeError, match='gpe_not_in_the_library'):
        _lib.lib()


def test_slot_table_is_host_only():
    l = _lib.lib()
    ends = (ctypes.c_long * 4)(4, 2052, 2052 + 2048, 2052 + 2048 + 2052)
    slots = (ctypes.c_long * 5)()
    assert l.gpe_grad_norm_slots(ends, 4, slots) == 5 and list(slots) == [0, 1, 2, 3, 5]
    assert l.gpe_grad_norm_slots(None, 4, slots) == -22 and l.gpe_grad_norm_slots(ends, 4, None) == -22
    assert l.gpe_grad_norm_slots(ends, 0, slots) == -22 and l.gpe_grad_norm_slots(ends, 4097, slots) == -22
    assert l.gpe_grad_norm_slots((ctypes.c_long * 2)(8, 8), 2, slots) == -22        # not increasing
    assert l.gpe_grad_norm_slots((ctypes.c_long * 2)(8, 14), 2, slots) == -22       # not a multiple of four
    assert l.gpe_grad_norm_slots((ctypes.c_long * 1)(0), 1, slots) == -22


def test_bad_arguments_are_rejected_without_a_gpu():
    """NULL or misaligned pointers, n <= 0 and more than 8 words come back as -22 before any launch.  The non-NULL 'device'
    pointers are made-up addresses: an entry point that refuses its arguments never touches them."""
    l = _lib.lib()
    A = 0x7f0000001000                           # 16-byte aligned
    part = lambda **k: l.gpe_grad_norm_part(*[k.get(n, d) for n, d in (('g', A), ('n', 64), ('seg_end', A), ('seg_slot', A), ('nseg', 3),
                                                                        ('lo', 0), ('hi', 3), ('slots', 3), ('part', A), ('stream', None))])
    for bad in (dict(g=None), dict(seg_end=None), dict(seg_slot=None), dict(part=None), dict(g=A + 4), dict(g=A + 8), dict(part=A + 4),
                dict(seg_end=A + 4), dict(n=0), dict(n=-5), dict(nseg=0), dict(nseg=4097), dict(lo=2, hi=2), dict(hi=4), dict(lo=-1),
                dict(slots=0)):
        assert part(**bad) == -22, bad
    runs = (ctypes.c_int * 2)(0, 3)
    words = (ctypes.c_void_p * 9)(*[A] * 9)
    fin = lambda **k: l.gpe_grad_norm_finish(*[k.get(n, d) for n, d in (
        ('part', A), ('seg_slot', A), ('nseg', 3), ('slots', 3), ('runs', runs), ('nruns', 1), ('gscale', 1.0), ('max_norm', 0.0),
        ('nonfinite', 1), ('words', words), ('nwords', 0), ('limit', 65504.0), ('seg_norm', None), ('reversed', 0), ('guard', A),
        ('stream', None))])
    for bad in (dict(part=None), dict(seg_slot=None), dict(guard=None), dict(runs=None), dict(guard=A + 8), dict(guard=A + 4),
                dict(part=A + 4), dict(seg_norm=A + 2), dict(nwords=9), dict(nwords=-1), dict(nwords=2, words=None), dict(nruns=0),
                dict(nruns=17), dict(nseg=0), dict(slots=0),
                dict(runs=(ctypes.c_int * 2)(0, 4)), dict(runs=(ctypes.c_int * 2)(2, 2)),
                dict(runs=(ctypes.c_int * 4)(1, 3, 0, 1), nruns=2),                    # runs must ascend
                dict(nwords=2, words=(ctypes.c_void_p * 2)(A, None)), dict(nwords=1, words=(ctypes.c_void_p * 1)(A + 2))):
        assert fin(**bad) == -22, bad
    step = lambda **k: l.gpe_adam_step_guarded(*[k.get(n, d) for n, d in (
        ('p', A), ('g', A), ('m', A), ('v', A), ('n', 64), ('lr', 1e-3), ('b1', 0.9), ('b2', 0.999), ('eps', 1e-8), ('wd', 0.0),
        ('step', 1), ('gscale', 1.0), ('zero', 1), ('guard', A), ('stream', None))])
    dev = lambda **k: l.gpe_adam_step_guarded_dev(*[k.get(n, d) for n, d in (
        ('p', A), ('g', A), ('m', A), ('v', A), ('n', 64), ('hyper', A), ('b1', 0.9), ('b2', 0.999), ('eps', 1e-8), ('wd', 0.0),
        ('gscale', 1.0), ('zero', 1), ('guard', A), ('stream', None))])
    for fn in (step, dev):
        for bad in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(guard=None), dict(p=A + 4), dict(v=A + 8),
                    dict(guard=A + 8), dict(n=0), dict(n=-1)):
            assert fn(**bad) == -22, bad
    assert step(step=0) == -22 and dev(hyper=None) == -22 and dev(hyper=A + 2) == -22


def test_constructor_defaults_and_checks():
    sig = inspect.signature(optim.FusedAdam.__init__).parameters
    assert [sig[k].default for k in ('max_grad_norm', 'skip_nonfinite', 'guard_overflow', 'param_grad_norms')] == [None, False, False, False]
    net = torch.nn.Linear(3, 2)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='max_grad_norm'):
            optim.FusedAdam(net, max_grad_norm=bad)
    # the options are accepted, and do not open a CPU path
    with pytest.raises(RuntimeError, match='no CPU path'):
        optim.FusedAdam(net, max_grad_norm=1.0, skip_nonfinite=True, guard_overflow=True, param_grad_norms=True)
    # the record of watched fp16-activation words: per device, bounded, cleared on request
    ops = gpe_amd.ops
    assert ops.watched_words('cuda:0') == [] and ops.HalfActGuard.LIMIT == AG.LIMIT
    ops.clear_watched_words('cuda:0')

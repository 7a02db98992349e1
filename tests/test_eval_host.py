"""not-gpu: the evaluation pass (include/gpe_hip_eval.h, ops.EvalAccumulator / quality_pool, metrics.*.eval_keys,
evaluation.Evaluator) as far as it goes without a device:
  (1) gpe_hip_eval.h parses, its symbols are exported and bound with the parsed types through _lib.EVAL_HEADERS, the ABI version is
      7, and the three older headers and the two older tuples are what they were;
  (2) every entry point refuses bad arguments with -22 before it touches a pointer;
  (3) the restatement of the reference's rule (tests/eval_restate.py) on a hand-worked example;
  (4) eval_keys(epoch) names exactly the keys of the loss dict the reference recorded in every tests/golden/quality_*.pt;
  (5) the Python argument checks that need no device."""
import copy
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import gpe_amd
from gpe_amd import _lib, evaluation, metrics, ops
import eval_restate as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, 'golden', 'quality_*.pt')))
EVAL = ('gpe_eval_add', 'gpe_eval_pool')


def test_the_eval_header_is_bound_and_exported():
    main, ext = _lib.parse_header(), _lib.parse_header(_lib.EXT_HEADER_PATH)
    fit, ev = _lib.parse_header(_lib.FIT_HEADER_PATH), _lib.parse_header(_lib.EVAL_HEADER_PATH)
    assert set(ev) == set(EVAL) and not set(ev) & (set(main) | set(ext) | set(fit))
    assert len(main) == 123 and set(fit) == {'gpe_fit_leaves', 'gpe_fit_part', 'gpe_fit_finish'}
    assert set(ext) == {'gpe_grad_norm_slots', 'gpe_grad_norm_part', 'gpe_grad_norm_finish', 'gpe_adam_step_guarded',
                        'gpe_adam_step_guarded_dev'}
    assert _lib.HEADERS == (_lib.HEADER_PATH, _lib.EXT_HEADER_PATH) and _lib.FEATURE_HEADERS == (_lib.FIT_HEADER_PATH,)
    assert _lib.EVAL_HEADERS == (_lib.EVAL_HEADER_PATH,)
    assert ev['gpe_eval_add'] == ('i', ['p', 'i'] * 4 + ['i', 'p', 'p', 'i', 'p', 'p', 'p', 'p', 'i', 'p', 'p'])
    assert ev['gpe_eval_pool'] == ('i', ['p', 'p', 'l', 'i', 'i', 'i', 'i', 'p', 'p', 'p'])
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ev:
        assert hasattr(raw, name), 'libgpe_hip.so does not export %s' % name
    l = _lib.lib()
    assert l.gpe_abi_version() == 7
    for name, (res, args) in ev.items():
        fn = getattr(l, name)
        assert fn.restype is _lib._CT[res] and list(fn.argtypes) == [_lib._CT[a] for a in args], name


def test_an_eval_symbol_that_is_not_exported_fails_loudly(tmp_path, monkeypatch):
    h = tmp_path / 'eval.h'
    h.write_text('int gpe_eval_not_in_the_library(const float* x, void* stream);\n')
    monkeypatch.setattr(_lib, 'EVAL_HEADERS', (_lib.EVAL_HEADER_PATH, str(h)))
    monkeypatch.setattr(_lib, '_lib', None)
    with pytest.raises(AttributeError, match='gpe_eval_not_in_the_library'):
        _lib.lib()


def _key(idx, src, gate=0):
    return idx | (src << 8) | (gate << 16)


def test_bad_arguments_are_rejected_without_a_gpu():
    """The non-NULL 'device' pointers are made-up addresses: an entry point that refuses its arguments never touches them."""
    l = _lib.lib()
    A = 0x7f0000001000
    good = (ctypes.c_int32 * 3)(_key(0, 0), _key(4, 1), _key(13, 2, 3))

    def add(**k):
        d = dict(s0=A, n0=5, s1=A, n1=5, s2=A, n2=14, s3=None, n3=0, ns=3, counts=A, keys=good, K=3, sum=A, cnt=A, batches=A,
                 slot=A, slots=2, status=A)
        d.update(k)
        return l.gpe_eval_add(d['s0'], d['n0'], d['s1'], d['n1'], d['s2'], d['n2'], d['s3'], d['n3'], d['ns'], d['counts'], d['keys'],
                              d['K'], d['sum'], d['cnt'], d['batches'], d['slot'], d['slots'], d['status'], None)

    arr = lambda *v: (ctypes.c_int32 * len(v))(*v)          # noqa: E731
    for bad in (dict(K=0), dict(K=-1), dict(K=65), dict(ns=5), dict(ns=-1), dict(slots=0), dict(slots=-3), dict(keys=None),
                dict(sum=None), dict(cnt=None), dict(batches=None), dict(slot=None), dict(status=None),
                dict(counts=None),                                   # a gated key without counts
                dict(ns=2),                                          # a key of source 2 with two sources
                dict(n1=4),                                          # index 4 of a source of 4
                dict(s1=None),                                       # a source with a length and no pointer
                dict(n0=-1), dict(n2=257),
                dict(keys=arr(_key(0, 3), 0, 0)),                    # source 3 of three
                dict(keys=arr(_key(0, 0, 5), 0, 0)),                 # gate 5: counts has four words
                dict(keys=arr(1 << 12, 0, 0)), dict(keys=arr(-1, 0, 0))):
        assert add(**bad) == -22, bad

    def pool(**k):
        d = dict(table=A, group=A, G=100, n_groups=3, P=23, L=14, flags=63, out=A, counts=A)
        d.update(k)
        return l.gpe_eval_pool(d['table'], d['group'], d['G'], d['n_groups'], d['P'], d['L'], d['flags'], d['out'], d['counts'], None)

    for bad in (dict(n_groups=-1), dict(n_groups=65536), dict(flags=128), dict(flags=-1), dict(flags=1 << 20), dict(G=0), dict(G=-5),
                dict(G=2 ** 31), dict(P=0), dict(L=0), dict(table=None), dict(out=None), dict(counts=None), dict(group=None)):
        assert pool(**bad) == -22, bad


def test_restatement_on_a_hand_worked_example():
    """three batches; `a` has a value in all, `c` a None in the second, `n` a NaN in the third, `never` no value at all, `late` first
    appears in the third batch"""
    f = np.float32
    batches = [(f(1.5), {'a': f(0.1), 'c': f(4.0), 'n': f(1.0), 'never': None}),
               (f(2.25), {'a': f(0.2), 'c': None, 'n': f(2.0), 'never': None}),
               (f(0.25), {'a': f(0.3), 'c': f(1.0), 'n': f(np.nan), 'never': None, 'late': 7})]
    got = R.aggregate(batches)
    assert list(got) == ['full_loss', 'a', 'c', 'n', 'never', 'late']
    assert got['full_loss'] == f(4.0) / f(3) and got['full_loss'].dtype == np.float32
    assert got['a'] == f(f(f(0.1) + f(0.2)) + f(0.3)) / f(3)           # float32 adds in batch order, each rounded
    assert got['c'] == f(2.5) and got['never'] is None and np.isnan(got['n']) and got['late'] == f(7)
    s, n = R.sums(batches)
    assert n == {'full_loss': 3, 'a': 3, 'c': 2, 'n': 3, 'never': 0, 'late': 1} and s['c'] == f(5) and s['never'] == f(0)
    # the order matters in float32: a large value first swallows the small ones
    big = [(f(0), {'x': f(2 ** 24)}), (f(0), {'x': f(1)}), (f(0), {'x': f(1)})]
    assert R.aggregate(big)['x'] == f(2 ** 24) / f(3) and R.aggregate(big[::-1])['x'] == f(2 ** 24 + 2) / f(3)
    # the gate table
    assert R.gate('corr_rotation_l2', 1.0, [0, 5, 5, 5]) is None and R.gate('corr_rotation_l2', 1.0, [1, 0, 0, 0]) == 1.0
    assert R.gate('corr_panel_shape_l2', 1.0, [3, 0, 1, 1]) is None and R.gate('corr_stitch_recall', 1.0, [3, 3, 0, 3]) is None
    assert R.gate('corr_num_edges_accuracy', np.nan, [0, 0, 0, 0]) is not None and R.gate('corr_rotation_l2', 1.0, None) is None
    assert R.GATES == ops.QUALITY_GATES
    assert R.same(None, None) and not R.same(None, f(0)) and R.same(f(np.nan), f(np.nan)) and not R.same(f(0.0), f(-0.0))


@pytest.mark.parametrize('path', FIXTURES, ids=[os.path.basename(f)[8:-3] for f in FIXTURES])
def test_eval_keys_are_the_keys_of_the_recorded_loss_dict(path):
    fx = torch.load(path, weights_only=False)
    loss = metrics.ComposedPatternLoss(copy.deepcopy(fx['data_config']), copy.deepcopy(fx['loss_config']))
    keys, gates = loss.eval_keys(fx['epoch'])
    names = [k[0] for k in keys]
    assert names[0] == 'full_loss' and len(set(names)) == len(names)
    assert set(names[1:]) == set(fx['loss_dict'])
    assert gates == {k: g for k, g in R.GATES.items() if k in names}
    for name, src, idx in keys:
        assert 0 <= src < ops.EVAL_MAX_SOURCES
        if name in ops.QUALITY_KEYS:
            assert (src, idx) == (2, ops.QUALITY_KEYS.index(name))
    # a key that the reference's dict gives None must be a gated one
    assert all(k in gates for k, v in fx['loss_dict'].items() if v is None)
    loss.with_quality_eval = False
    assert not set(k[0] for k in loss.eval_keys(fx['epoch'])[0]) & set(ops.QUALITY_KEYS)


def test_pair_loss_keys():
    loss = metrics.ComposedLoss({}, {'loss_components': ['edge_pair_class'],
                                     'quality_components': ['edge_pair_class', 'edge_pair_stitch_recall']})
    keys, gates = loss.eval_keys()
    assert [k[0] for k in keys] == ['full_loss', 'edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall']
    assert gates == {} and [k[1:] for k in keys] == [(0, 0), (0, 0), (0, 1), (0, 2), (0, 3)]
    with pytest.raises(ValueError, match='full_loss'):
        metrics.ComposedLoss({}, {'loss_components': [], 'quality_components': ['edge_pair_class']}).eval_keys()


def test_python_checks_need_no_device():
    K = [('a', 0, 0), ('b', 1, 3)]
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.EvalAccumulator(K, {}, device='cpu')
    for bad_keys, gates in (([], {}), ([('a', 0, 0)] * 2, {}), ([('a', 4, 0)], {}), ([('a', 0, 256)], {}), ([('a', 0, 0)], {'a': 4}),
                            ([('a', 0, 0)], {'b': 0}), ([('k%d' % i, 0, i) for i in range(65)], {})):
        with pytest.raises(ValueError, match='EvalAccumulator'):
            ops.EvalAccumulator(bad_keys, gates, device='cuda')
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match='slots'):
            ops.EvalAccumulator(K, {}, slots=bad, device='cuda')
    with pytest.raises(ValueError, match='table must be'):
        ops.quality_pool(torch.zeros(4, 15, dtype=torch.float64), None, 0, 23, 14, 63)
    with pytest.raises(ValueError, match='table must be'):
        ops.quality_pool(torch.zeros(4, 16), None, 0, 23, 14, 63)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.quality_pool(torch.zeros(4, 16, dtype=torch.float64), None, 0, 23, 14, 63)
    assert gpe_amd.evaluation is evaluation and callable(evaluation.eval_metrics)
    with pytest.raises(TypeError, match='ComposedPatternLoss or ComposedLoss'):
        evaluation.Evaluator(torch.nn.Linear(2, 2))

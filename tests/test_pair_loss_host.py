"""not-gpu: the training loss of the edge-pair classifier (ops.pair_class_loss / the device path of metrics.ComposedLoss) and the
extras of graph.StepGraph, as far as they can be checked without a device.
  (1) the fp64 restatement (tests/pair_loss_restate.py) agrees with torch's float64 binary_cross_entropy_with_logits and its
      autograd at 1e-12, and reproduces what the reference's own classes recorded over three training steps
      (tests/golden/stitch_train_small.pt, scripts/make_stitch_train_golden.py): counts and ratios exactly, the loss within the
      rounding bound of the reference's float32 arithmetic;
  (2) the C ABI: the two new symbols are declared and exported, -22 on bad arguments without a GPU;
  (3) ops.pair_class_loss has no CPU path; ComposedLoss on CPU tensors returns what it always returned;
  (4) StepGraph splits a tuple return into the loss and the detached extras."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gpe_amd
from gpe_amd import _lib
import pair_loss_restate as PL

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'stitch_train_small.pt')
SYMBOLS = ('gpe_pair_loss_fwd', 'gpe_pair_loss_bwd')


@pytest.fixture(scope='module')
def fx():
    return torch.load(FIXTURE, weights_only=False)


def test_fixture_is_what_the_generator_promises(fx):
    assert os.path.getsize(FIXTURE) < (1 << 20)
    assert fx['data_config'] == {'element_size': 12} and fx['nn_config'] == {'stitch_hidden_size': 72, 'stitch_mlp_n_layers': 2}
    assert tuple(fx['pairs'].shape) == (3, 271, 12) and fx['labels'].dtype == torch.bool and len(fx['steps']) == 3
    assert fx['loss_config']['loss_components'] == ['edge_pair_class']
    assert fx['loss_config']['quality_components'] == ['edge_pair_class', 'edge_pair_stitch_recall']
    assert 0.15 < fx['labels'].float().mean().item() < 0.35
    assert all(v < 0.25 for v in fx['fp32_vs_fp64_in_bars'].values()) and fx['logit_margin'] > 1e-3 and fx['pre_margin'] > 1e-3
    losses = [s['full_loss'] for s in fx['steps']]
    assert losses[0] > losses[1] > losses[2]                    # the labels can be learnt
    for s in fx['steps']:
        assert s['logits'].abs().min().item() > 1e-3
        assert set(s['loss_dict']) == set(PL.METRICS) and set(s['grads']) == {k for k in s['state_before'] if 'running' not in k and 'num_batches' not in k}
    # a step starts where the previous one ended: Adam moved every parameter, the forward moved the running statistics
    for a, b in zip(fx['steps'], fx['steps'][1:] + [{'state_before': fx['state_after']}]):
        assert all(not torch.equal(a['state_before'][k], b['state_before'][k]) for k in a['state_before'])


@pytest.mark.parametrize('labels', ['bool', 'soft'])
def test_restatement_agrees_with_torch_float64(labels):
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(700, generator=g, dtype=torch.float64) * 6, torch.tensor([0.0, 1e-5, -1e-5, 104.0, -104.0], dtype=torch.float64)])
    y = (torch.rand(705, generator=g) < 0.3).double() if labels == 'bool' else torch.rand(705, generator=g, dtype=torch.float64)
    xt = x.clone().requires_grad_(True)
    want = torch.nn.functional.binary_cross_entropy_with_logits(xt, y)
    want.backward()
    got = PL.evaluate(x.numpy(), y.numpy())
    assert abs(got['loss'] - want.item()) <= 1e-12
    assert np.abs(got['grad'] - xt.grad.numpy()).max() <= 1e-12
    cls = torch.round(torch.sigmoid(x))
    c = got['counts']
    assert c['pairs'] == 705 and c['correct'] == int((cls == y).sum()) and c['predicted_positives'] == int((cls == 1).sum())
    assert c['gt_positives'] == int((y == 1).sum()) and c['true_positives'] == int(((cls == 1) & (y == 1)).sum())


def test_restatement_conventions():
    got = PL.evaluate([-3.0, 2.0, 1.0, -0.5, 0.0], [0, 1, 0, 0, 0])
    assert tuple(got['counts'][k] for k in PL.COUNTS) == (5, 4, 1, 2, 1)
    want = np.log1p(np.exp(-3.0)) + np.log1p(np.exp(-2.0)) + (1.0 + np.log1p(np.exp(-1.0))) + np.log1p(np.exp(-0.5)) + np.log(2.0)
    assert abs(got['loss'] - want / 5) < 1e-15
    m = got['metrics']
    assert m['edge_pair_class_acc'] == np.float32(4) / np.float32(5) and m['stitch_precision'] == np.float32(0.5) and m['stitch_recall'] == 1
    empty_pred = PL.evaluate([-1.0, -2.0], [1, 0])['metrics']
    assert empty_pred['stitch_precision'] == 0 and empty_pred['stitch_recall'] == 0 and empty_pred['edge_pair_class_acc'] == 0.5
    assert PL.evaluate([1.0], [0])['metrics']['stitch_recall'] == 0
    none = PL.evaluate([], [])
    assert np.isnan(none['loss']) and set(none['counts'].values()) == {0} and none['metrics']['edge_pair_class_acc'] == 0
    # at +-104 exp(-|x|) underflows in float32 and the term is |x| or 0
    assert PL.bce_terms([104.0, -104.0, 104.0], [0, 0, 1]).tolist() == pytest.approx([104.0, 0.0, 0.0], abs=1e-40)


def test_restatement_reproduces_the_references_recorded_steps(fx):
    labels = fx['labels'].numpy()
    for i, s in enumerate(fx['steps']):
        got = PL.evaluate(s['logits'].numpy(), labels)
        assert got['counts'] == s['counts'], i
        for k in PL.METRICS[1:]:
            assert s['loss_types'][k] == 'Tensor' and got['metrics'][k] == np.float32(s['loss_dict'][k]), (i, k)
        ref, bound = s['loss_dict']['edge_pair_class_loss'], PL.reference_arithmetic_bound(s['logits'].numpy())
        print('step %d: reference (float32) %.9g  exact %.12g  |difference| %.3g  (rounding bound %.3g)' % (i, ref, got['loss'], abs(got['loss'] - ref), bound))
        assert ref == s['full_loss'] and abs(got['loss'] - ref) <= bound
        # the gradient the reference's autograd handed to the last block: through the bias-free route of the output BatchNorm
        # it is not recorded, but its sum is the gradient of that BatchNorm's bias
        bn_bias = [k for k in s['grads'] if k.endswith('.2.bias')][-1]
        assert abs(got['grad'].sum() - s['grads'][bn_bias].item()) <= 1e-6


def test_header_declares_and_library_exports_the_symbols():
    sigs = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in sigs and hasattr(raw, name), name
        res, args = sigs[name]
        assert res == 'i' and args[-1] == 'p'
    assert sigs['gpe_pair_loss_fwd'][1] == list('ppilipppp') + ['p'] and sigs['gpe_pair_loss_bwd'][1] == list('ppilpp') + ['p']
    assert _lib.lib().gpe_abi_version() == 7


def test_bad_arguments_are_rejected_without_a_gpu():
    l = _lib.lib()
    buf = (ctypes.c_double * 64)()                      # host memory stands in for the pointers that are checked, never followed
    p = ctypes.addressof(buf)
    assert l.gpe_pair_loss_fwd(None, None, 0, 8, 64, None, None, None, None, None) == -22
    assert l.gpe_pair_loss_bwd(None, None, 0, 8, None, None, None) == -22
    for args in ((None, p, 0, 8, 64, p, p, p, p), (p, None, 0, 8, 64, p, p, p, p), (p, p, 2, 8, 64, p, p, p, p), (p, p, 0, -1, 64, p, p, p, p),
                 (p, p, 0, 1 << 31, 64, p, p, p, p), (p, p, 0, 8, 0, p, p, p, p), (p, p, 0, 8, 257, p, p, p, p), (p, p, 0, 8, 64, None, p, p, p),
                 (p, p, 0, 8, 64, p + 4, p, p, p), (p, p, 0, 8, 64, p, None, p, p), (p, p, 0, 8, 64, p, p, None, p), (p, p, 0, 8, 64, p, p, p, None)):
        assert l.gpe_pair_loss_fwd(*args, None) == -22, args
    for args in ((None, p, 0, 8, p, p), (p, None, 1, 8, p, p), (p, p, 3, 8, p, p), (p, p, 0, -2, p, p), (p, p, 0, 8, None, p), (p, p, 0, 8, p, None)):
        assert l.gpe_pair_loss_bwd(*args, None) == -22, args
    assert l.gpe_pair_loss_bwd(None, None, 0, 0, p, p, None) == 0           # no rows: nothing to launch ...
    assert l.gpe_pair_loss_bwd(None, None, 0, 0, p, None, None) == 0        # ... and an empty gradient may be NULL


def test_pair_class_loss_has_no_cpu_path():
    x, y = torch.randn(3, 5), torch.rand(3, 5) < 0.5
    with pytest.raises(RuntimeError, match='no CPU path'):
        gpe_amd.ops.pair_class_loss(x, y)
    with pytest.raises(RuntimeError, match='no CPU path'):
        gpe_amd.ops.PairClassLossFn.apply(x, y.float())
    assert gpe_amd.ops.PAIR_LOSS_METRICS == PL.METRICS and gpe_amd.ops.PAIR_LOSS_COUNTS == PL.COUNTS
    assert 1 <= gpe_amd.ops.PAIR_LOSS_SLOTS <= 256


def test_composed_loss_on_cpu_tensors_is_unchanged(fx):
    """the torch expressions stay for CPU tensors: same keys, tensors where the reference has tensors, the Python int 0 on an empty
    denominator, and the reference's recorded numbers bit for bit (the same float32 torch calls on the same logits)"""
    loss = gpe_amd.metrics.ComposedLoss(fx['data_config'], dict(fx['loss_config']))
    s = fx['steps'][0]
    x = s['logits'].clone().requires_grad_(True)
    full, d, changed = loss(x, fx['labels'])
    assert changed is False and list(d) == list(PL.METRICS) and full.item() == s['full_loss']
    for k in PL.METRICS:
        assert isinstance(d[k], torch.Tensor) and d[k].item() == s['loss_dict'][k], k
    full.backward()
    assert np.abs(x.grad.double().numpy().reshape(-1) - PL.evaluate(s['logits'].numpy(), fx['labels'].numpy())['grad']).max() < 1e-9
    _, d, _ = loss(torch.tensor([-2.0, -1.0]), torch.tensor([False, False]))
    assert type(d['stitch_precision']) is int and d['stitch_precision'] == 0 and type(d['stitch_recall']) is int
    _, d, _ = loss(torch.tensor([-2.0, -1.0]), torch.tensor([True, False]))
    assert type(d['stitch_precision']) is int and isinstance(d['stitch_recall'], torch.Tensor) and d['stitch_recall'].item() == 0
    loss.with_quality_eval = False
    assert list(loss(x, fx['labels'])[1]) == ['edge_pair_class_loss']


class _Opt:
    step_captured = advance_captured = None

    def step(self):
        pass


def test_step_graph_splits_the_loss_from_the_extras(monkeypatch):
    """host side of graph.StepGraph's extras: the first element is the loss, what follows is kept detached in its own nesting"""
    from gpe_amd import graph
    sg = graph.StepGraph.__new__(graph.StepGraph)              # (the constructor opens a device stream)
    w = torch.ones(3, requires_grad=True)

    def fl(a):
        loss = (w * a).sum()
        return loss, {'twice': loss * 2, 'nested': [a + 1, {'w': w * 3}]}, 'tag'

    sg.forward_loss, sg.static_in, sg.opt, sg.extras = fl, (torch.arange(3.0),), _Opt(), 'stale'
    loss = sg._eager()
    assert loss.item() == 3.0 and torch.equal(w.grad, torch.arange(3.0))
    d, tag = sg.extras
    assert tag == 'tag' and d['twice'].item() == 6.0 and not d['twice'].requires_grad and not d['nested'][1]['w'].requires_grad
    assert isinstance(d['nested'], list) and torch.equal(d['nested'][0], torch.arange(3.0) + 1)
    sg.forward_loss = lambda a: [(w * a).sum()]
    assert sg._eager().item() == 3.0 and sg.extras == ()
    sg.forward_loss = lambda a: (w * a).sum()
    assert sg._eager().item() == 3.0 and sg.extras is None
    sg.forward_loss = lambda a: ()
    with pytest.raises(ValueError, match='empty'):
        sg._eager()

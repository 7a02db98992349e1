"""ops.pair_class_loss / ops.PairClassLossFn (gpe_pair_loss_fwd / _bwd) against the fp64 restatement tests/pair_loss_restate.py on
the same fp32 logits: counts and ratios exactly, the loss within 2^-20 max(1, loss), the gradient within 2^-20 of sigmoid(x) - y
(gpe_sigmoid is an expf, an add and a divide on values <= 1: about 4 float32 ulps = 2^-22), bit-reproducible, independent of the
view's shape and of a compute-unit reservation; and the device path of metrics.ComposedLoss on top of it.

Logits are exactly 0 or at least 1e-5 in magnitude (sigmoid(1e-5) - 0.5 is about 40 float32 ulps: a few-ulp sigmoid cannot misplace
such a value), up to +-104 where exp(-|x|) underflows."""
import functools

import numpy as np
import pytest
import torch

import pair_loss_restate as PL

pytestmark = pytest.mark.gpu

SLOTS = 64                     # asserted against ops.PAIR_LOSS_SLOTS below: M = SLOTS * 256 + 1 gives a slot more than one pass
SIZES = [1, 63, 65, 257, 813, SLOTS * 256 + 1, 12000]
SPECIALS = [0.0, 1e-5, -1e-5, 104.0, -104.0]
GSCALE = 0.75


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    assert gpe_amd.ops.PAIR_LOSS_SLOTS == SLOTS
    return gpe_amd


@functools.lru_cache(maxsize=None)
def _case(M, pattern, negative=False):
    """-> (fp32 logits, labels as float64 0 / 1, the restatement's result), computed once and shared"""
    g = torch.Generator().manual_seed(1000 + M)
    x = (torch.randn(M, generator=g) * 5).clamp_(-104, 104)
    x = torch.where(x.abs() < 1e-5, torch.full_like(x, 1e-5), x)
    n = min(M, len(SPECIALS))
    x[:n] = torch.tensor(SPECIALS[:n])
    if negative:
        x = -x.abs() - 1e-5
    y = {'zeros': torch.zeros(M, dtype=torch.bool), 'ones': torch.ones(M, dtype=torch.bool),
         'mixed': torch.rand(M, generator=g) < 0.3}[pattern]
    return x, y, PL.evaluate(x.numpy(), y.numpy())


def _check(got_out, got_counts, want):
    out, counts = got_out.detach().cpu().numpy(), got_counts.cpu().tolist()
    assert counts == [want['counts'][k] for k in PL.COUNTS]
    for i, k in enumerate(PL.METRICS[1:], 1):
        assert out[i] == want['metrics'][k], k
    err = abs(float(out[0]) - want['loss'])
    assert err <= 2.0 ** -20 * max(1.0, want['loss']), (float(out[0]), want['loss'])
    return err


@pytest.mark.parametrize('dtype', ['bool', 'fp32'])
@pytest.mark.parametrize('pattern', ['zeros', 'ones', 'mixed'])
@pytest.mark.parametrize('M', SIZES)
def test_loss_counts_and_gradient_against_the_restatement(gpe, M, pattern, dtype):
    x, y, want = _case(M, pattern)
    if pattern == 'zeros':
        assert want['counts']['gt_positives'] == 0 and want['metrics']['stitch_recall'] == 0          # recall denominator empty
    xd = x.cuda().requires_grad_(True)
    yd = y.cuda() if dtype == 'bool' else y.float().cuda()
    out, counts = gpe.ops.pair_class_loss(xd, yd, return_counts=True)
    assert out.shape == (4,) and out.dtype == torch.float32 and counts.dtype == torch.int32 and not counts.requires_grad
    err = _check(out, counts, want)
    (out[0] * GSCALE).backward(retain_graph=True)
    g1 = xd.grad.clone()
    gerr = np.abs(M * g1.cpu().double().numpy() / GSCALE - M * want['grad']).max()
    print('M=%d %s %s: |loss - fp64| %.3g (bar %.3g)  |M gx / gscale - (sigmoid - y)| %.3g (bar %.3g)'
          % (M, pattern, dtype, err, 2.0 ** -20 * max(1.0, want['loss']), gerr, 2.0 ** -20))
    assert gerr <= 2.0 ** -20
    # a second backward over the same graph: nothing was overwritten
    xd.grad = None
    (out[0] * GSCALE).backward()
    assert torch.equal(xd.grad, g1)
    # the ratios carry no gradient
    xd.grad = None
    out2 = gpe.ops.pair_class_loss(xd, yd)
    out2[1:].sum().backward()
    assert torch.count_nonzero(xd.grad).item() == 0


@pytest.mark.parametrize('dtype', ['bool', 'fp32'])
def test_no_predicted_positive(gpe, dtype):
    """all logits negative: the precision denominator is empty"""
    x, y, want = _case(813, 'mixed', negative=True)
    assert want['counts']['predicted_positives'] == 0 and want['counts']['gt_positives'] > 0
    out, counts = gpe.ops.pair_class_loss(x.cuda(), y.cuda() if dtype == 'bool' else y.float().cuda(), return_counts=True)
    _check(out, counts, want)
    assert out[2].item() == 0 and out[3].item() == 0


def test_no_rows(gpe):
    x = torch.zeros(0, device='cuda', requires_grad=True)
    out, counts = gpe.ops.pair_class_loss(x, torch.zeros(0, device='cuda', dtype=torch.bool), return_counts=True)
    assert torch.isnan(out[0]).item() and out[1:].tolist() == [0, 0, 0] and counts.tolist() == [0] * 5
    out[0].backward()
    assert x.grad.shape == (0,)


def test_label_types_and_refusals(gpe):
    x, y, want = _case(257, 'mixed')
    xd = x.cuda()
    base = gpe.ops.pair_class_loss(xd, y.cuda())
    for yd in (y.cuda().to(torch.uint8), y.cuda().long(), y.cuda().double(), y.cuda().half()):
        assert torch.equal(gpe.ops.pair_class_loss(xd, yd), base), yd.dtype
    with pytest.raises(ValueError, match='labels'):
        gpe.ops.pair_class_loss(xd, y.cuda()[:-1])
    with pytest.raises(RuntimeError, match='no CPU path'):
        gpe.ops.pair_class_loss(xd, y)
    with pytest.raises(RuntimeError, match='fp32'):
        gpe.ops.pair_class_loss(xd.double(), y.cuda())
    # soft labels: the general term
    soft = torch.rand(257, generator=torch.Generator().manual_seed(3))
    got = gpe.ops.pair_class_loss(xd, soft.cuda())
    ws = PL.evaluate(x.numpy(), soft.numpy())
    assert abs(got[0].item() - ws['loss']) <= 2.0 ** -20 * max(1.0, ws['loss'])


def test_reproducible_and_independent_of_shape_and_reservation(gpe):
    x, y, _ = _case(12000, 'mixed')

    def run(xs, ys):
        xs = xs.clone().requires_grad_(True)
        out, counts = gpe.ops.pair_class_loss(xs, ys, return_counts=True)
        out[0].backward()
        return out.detach().clone(), counts.clone(), xs.grad.reshape(-1).clone()

    xd, yd = x.cuda(), y.cuda()
    a = run(xd, yd)
    for other in (run(xd, yd), run(xd.view(30, 400), yd.view(30, 400)), run(xd.view(30, 400), yd), run(xd.view(8, 15, 100), yd.float().view(8, 15, 100))):
        assert all(torch.equal(p, q) for p, q in zip(a, other))
    prev = gpe.set_reserved_cus(16)
    try:
        reserved = run(xd, yd)
    finally:
        gpe.set_reserved_cus(prev)
    assert all(torch.equal(p, q) for p, q in zip(a, reserved))
    # a strided view is read through one dense copy: same numbers
    wide = torch.zeros(12000, 2, device='cuda')
    wide[:, 0] = xd
    assert all(torch.equal(p, q) for p, q in zip(a, run(wide[:, 0], yd)))
    # the ticket is left zero: the next launch on the stream finds its last arriver again
    assert gpe.ops._ticket(xd.device).item() == 0


@pytest.mark.parametrize('loss_config,quality,want', [
    ({}, True, ['edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall']),
    ({}, False, ['edge_pair_class_loss']),
    ({'quality_components': ['edge_pair_class']}, True, ['edge_pair_class_loss', 'edge_pair_class_acc']),
    ({'quality_components': ['edge_pair_stitch_recall']}, True, ['edge_pair_class_loss', 'stitch_precision', 'stitch_recall']),
    ({'loss_components': [], 'quality_components': ['edge_pair_class']}, True, ['edge_pair_class_acc']),
    ({'loss_components': [], 'quality_components': []}, True, []),
])
def test_composed_loss_on_device_tensors(gpe, loss_config, quality, want):
    """metrics.ComposedLoss on fp32 device tensors: the keys of the configuration, every value a 0-dim fp32 view of the kernel's one
    output, the numbers of the restatement, the gradient on the logits"""
    config = {'loss_components': ['edge_pair_class'], 'quality_components': ['edge_pair_class', 'edge_pair_stitch_recall']}
    config.update(loss_config)
    loss = gpe.metrics.ComposedLoss({'element_size': 12}, config)
    loss.with_quality_eval = quality
    x, y, ref = _case(813, 'mixed')
    xd = x.cuda().view(3, 271).requires_grad_(True)
    full, d, changed = loss(xd, y.view(3, 271))                     # (labels on the host: moved, as ever)
    assert changed is False and list(d) == want
    for k, v in d.items():
        assert v.is_cuda and v.dim() == 0 and v.dtype == torch.float32, k
        if k == 'edge_pair_class_loss':
            assert abs(v.item() - ref['loss']) <= 2.0 ** -20 * max(1.0, ref['loss'])
        else:
            assert v.item() == ref['metrics'][k] and not v.requires_grad, k
    assert len({v.untyped_storage().data_ptr() for v in d.values()}) <= 1
    if 'edge_pair_class_loss' in want:
        assert full is d['edge_pair_class_loss']
        full.backward()
        assert np.abs(813 * xd.grad.cpu().double().numpy().reshape(-1) - 813 * ref['grad']).max() <= 2.0 ** -20
    else:
        assert full == 0.


def test_composed_loss_empty_denominators_are_device_zeros(gpe):
    loss = gpe.metrics.ComposedLoss({'element_size': 12}, {'loss_components': ['edge_pair_class'],
                                                           'quality_components': ['edge_pair_class', 'edge_pair_stitch_recall']})
    _, d, _ = loss(torch.tensor([-2.0, -1.0], device='cuda'), torch.tensor([False, False], device='cuda'))
    for k in ('stitch_precision', 'stitch_recall'):
        assert isinstance(d[k], torch.Tensor) and d[k].is_cuda and d[k].item() == 0
    assert d['edge_pair_class_acc'].item() == 1
    # other dtypes keep the torch expressions (and the reference's Python 0)
    _, d, _ = loss(torch.tensor([-2.0, -1.0], device='cuda', dtype=torch.float64), torch.tensor([False, False], device='cuda'))
    assert type(d['stitch_precision']) is int

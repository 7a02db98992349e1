"""-m gpu: the training pairs of the edge-pair classifier drawn on the device (csrc/gpe_stitch_sample.hip through
ops.stitch_pairs_sample / staging.StitchPairSampler) against the integer-exact host restatement (tests/stitch_sample_restate.py,
which tests/test_stitch_sample_host.py holds against the reference's recorded counts): rows, labels and status bit for bit, the
invariants on the device output alone, the generator state, stream capture, and a short training run on fresh pairs.

The resident set is the six garments of tests/golden/stitch_pairs_*.pt padded to [6, 23, 14, 8] (junk in unused slots and behind the
stitch counts, int64 counts and ids: the widening path), ground truth from their planted stitches."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import stitch_sample_restate as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SMALL, GAPS, NONE, ONE, CLAIMED, FULL = range(6)
SEED = 0xfeedc0de12345678                     # a non-zero high half
CARRY = 2 ** 32 - 1                           # the next draw carries into the counter's fourth word


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


@functools.lru_cache(maxsize=None)
def _set():
    gs = R.resident_set(GOLDEN)
    assert gs['tags'] == ['small', 'gaps', 'none', 'one', 'claimed', 'full'] and gs['edges'].shape == (6, 23, 14, 8)
    gs['Sv'] = [len(R.valid_stitches(gs['num_edges'][g], 14, gs['gt'][g], gs['gt_num'][g])) for g in range(6)]
    assert gs['Sv'] == [4, 6, 0, 1, 3, 40]
    return gs


def _device_set(gs=None):
    gs = gs or _set()
    return [torch.from_numpy(gs[k]).cuda() for k in ('edges', 'num_edges', 'gt', 'gt_num')]


def _sampler(gpe, n_st, n_non, flags=3, seed=SEED, gs=None):
    gs = gs or _set()
    return gpe.staging.StitchPairSampler(*_device_set(gs), {'f_shift': gs['shift'], 'f_scale': gs['scale']}, n_st, n_non,
                                         bool(flags & 1), bool(flags & 2), seed=seed)


@functools.lru_cache(maxsize=None)
def _want(index, n_st, n_non, flags, seed, draw):
    """computed once per case and shared"""
    gs = _set()
    return R.sample_batch(gs['edges'], gs['num_edges'], gs['gt'], gs['gt_num'], list(index), n_st, n_non, flags, gs['shift'], gs['scale'],
                          seed, draw)[:3]


def _same(got, want, what):
    rows, labels, status = got
    assert rows.dtype == torch.float32 and labels.dtype == torch.bool and status.dtype == torch.int32
    assert status.cpu().tolist() == want[2].tolist(), what
    assert np.array_equal(labels.cpu().numpy(), want[1]), what
    assert np.array_equal(rows.cpu().numpy().view(np.int32), want[0].view(np.int32)), what


CASES = [
    # (n_stitched, n_non_stitched, index): R = 1; S_v stitches and one more row; 5 + 7 on `small` (two slots of it, and `gaps`, which has
    # six stitches: status -1); no stitches at all; R = 257; the shipped 400
    (1, 0, (ONE,)),
    (4, 1, (SMALL,)),
    (40, 1, (FULL,)),
    (5, 7, (SMALL, GAPS, SMALL)),
    (0, 64, (NONE, SMALL, NONE)),
    (40, 217, (FULL, SMALL, GAPS)),
    (200, 200, (FULL, CLAIMED, FULL)),
]


@pytest.mark.parametrize('flags', [0, 1, 2, 3])
@pytest.mark.parametrize('n_st,n_non,index', CASES, ids=['%d+%d' % c[:2] for c in CASES])
def test_bit_exact_against_the_restatement(gpe, n_st, n_non, index, flags):
    s = _sampler(gpe, n_st, n_non, flags)
    s.reseed(SEED, CARRY)
    idx = torch.tensor(index).cuda()
    for draw in (CARRY, CARRY + 1):
        rows, labels = s.sample(idx)
        assert rows.shape == (len(index), n_st + n_non, 16)
        _same((rows, labels, s.status), _want(index, n_st, n_non, flags, SEED, draw), (draw, flags))
    if len(index) == 3 and index[0] == index[2]:
        assert int(s.status[0]) == 0 and not torch.equal(rows[0], rows[2])          # the same garment in two slots: two draws


@pytest.mark.parametrize('n_st,n_non', [(40, 217), (200, 200)])
def test_thirty_slots_bit_exact(gpe, n_st, n_non):
    index = tuple((3 * b + b // 6) % 6 for b in range(30))
    s = _sampler(gpe, n_st, n_non, 3, seed=3 << 61)
    rows, labels = s.sample(torch.tensor(index, dtype=torch.int32).cuda())
    _same((rows, labels, s.status), _want(index, n_st, n_non, 3, 3 << 61, 0), 'B = 30')
    assert s.state.cpu().tolist()[1] == 1


@pytest.mark.parametrize('flags', [0, 3])
def test_invariants_of_the_device_output(gpe, flags):
    gs = _set()
    index = (SMALL, GAPS, NONE, ONE, CLAIMED, FULL, SMALL)
    for n_st, n_non in ((40, 23), (6, 10)):
        s = _sampler(gpe, n_st, n_non, flags, seed=11)
        rows, labels = s.sample(torch.tensor(index).cuda())
        rows, labels, status = rows.cpu().numpy(), labels.cpu().numpy(), s.status.cpu().tolist()
        for b, g in enumerate(index):
            assert status[b] == (-1 if gs['Sv'][g] > n_st else 0), (b, g)
            R.check_slot(rows[b], labels[b], status[b], gs['edges'][g], gs['num_edges'][g], gs['gt'][g], gs['gt_num'][g], n_st, n_non,
                         flags, gs['shift'], gs['scale'])
        assert not labels[2].any()                                                   # no stitches: all rows are non-stitched


def test_status_paths(gpe):
    gs = dict(_set())
    ne = gs['num_edges'].copy()
    ne[ONE] = 0
    ne[ONE, 7] = 1                                                                   # a single present edge: nothing to pair
    gs['num_edges'] = ne
    s = _sampler(gpe, 3, 5, 3, gs=gs)
    index = (-1, SMALL, 6, ONE, CLAIMED, -7, 10 ** 9)
    rows, labels = s.sample(torch.tensor(index).cuda())
    torch.cuda.synchronize()                                                         # the call returns: 64 attempts, not a loop
    status = s.status.cpu().tolist()
    assert status == [-2, -1, -2, 8, 0, -2, -2]
    for b in (0, 1, 2, 3, 5, 6):
        assert not rows[b].any() and not labels[b].any(), b
    R.check_slot(rows[4].cpu().numpy(), labels[4].cpu().numpy(), 0, gs['edges'][CLAIMED], ne[CLAIMED], gs['gt'][CLAIMED],
                 gs['gt_num'][CLAIMED], 3, 5, 3, gs['shift'], gs['scale'])
    _same((rows, labels, s.status), R.sample_batch(gs['edges'], ne, gs['gt'], gs['gt_num'], list(index), 3, 5, 3, gs['shift'],
                                                   gs['scale'], SEED, 0)[:3], 'status paths')


def test_state_advances_and_reseed_reproduces(gpe):
    s = _sampler(gpe, 6, 10, 3, seed=SEED)
    idx = torch.tensor([SMALL, CLAIMED, SMALL]).cuda()
    assert s.state.cpu().tolist() == [SEED - 2 ** 64, 0]
    a = s.sample(idx) + (s.status,)
    assert s.state.cpu().tolist()[1] == 1
    b = s.sample(idx) + (s.status,)
    assert s.state.cpu().tolist() == [SEED - 2 ** 64, 2] and int(s.ticket) == 0
    assert not torch.equal(a[0], b[0])
    s.reseed(SEED)
    prev = gpe.set_reserved_cus(16)
    try:
        a2 = s.sample(idx) + (s.status,)
    finally:
        gpe.set_reserved_cus(prev)
    b2 = s.sample(idx) + (s.status,)
    for x, y in zip(a + b, a2 + b2):
        assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x.view(torch.int32),
                           y.view(torch.uint8) if y.dtype == torch.bool else y.view(torch.int32))
    assert s.state.cpu().tolist()[1] == 2 and int(s.ticket) == 0
    s.reseed(SEED, 1)
    assert torch.equal(s.sample(idx)[0], b[0])
    s.reseed(SEED + 1)
    assert not torch.equal(s.sample(idx)[0], a[0])
    cfg = {'stitched_edge_pairs_num': 6, 'non_stitched_edge_pairs_num': 10, 'shuffle_pairs': True, 'shuffle_pairs_order': True,
           'standardize': {'f_shift': _set()['shift'], 'f_scale': _set()['scale']}, 'random_pairs_mode': True}
    t = gpe.staging.StitchPairSampler.from_config(*_device_set(), cfg, seed=SEED)
    assert torch.equal(t.sample(idx)[0], a[0])
    d = gpe.staging.StitchPairSampler(*_device_set(), cfg['standardize'])
    assert (d.stitched_edge_pairs_num, d.non_stitched_edge_pairs_num, d.shuffle_pairs, d.shuffle_pairs_order) == (200, 200, True, True)


def test_captured_call_draws_anew_on_every_replay(gpe):
    s = _sampler(gpe, 6, 10, 3, seed=SEED)
    idx = torch.tensor([FULL, SMALL, SMALL]).cuda()
    eager = []
    for _ in range(3):
        rows, labels = s.sample(idx)
        eager.append((rows.clone(), labels.clone(), s.status.clone()))
    s.reseed(SEED)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    replayed = []
    with torch.cuda.stream(side):
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, stream=side):
            rows, labels = s.sample(idx)
        for _ in range(3):
            cg.replay()
            replayed.append((rows.clone(), labels.clone(), s.status.clone()))
    side.synchronize()
    for i, (e, r) in enumerate(zip(eager, replayed)):
        for x, y in zip(e, r):
            assert torch.equal(x, y), i
        _same(r, _want((FULL, SMALL, SMALL), 6, 10, 3, SEED, i), i)
    assert s.state.cpu().tolist()[1] == 3 and int(s.ticket) == 0
    assert not torch.equal(replayed[0][0], replayed[1][0])


def test_captured_step_with_the_sampler_inside(gpe):
    """five steps of StepGraph(warmup=2) drawing their own pairs equal five eager steps: shipped architecture, f32, R = 24, B = 3"""
    from gpe_amd import optim, graph
    prev = gpe.set_math('f32')
    try:
        torch.manual_seed(5)
        model_a = gpe.nets.StitchOnEdge3DPairs({'element_size': 16}, {}, {}).cuda().train()
        assert model_a.config['stitch_hidden_size'] == 200 and model_a.config['stitch_mlp_n_layers'] == 3
        model_b = copy.deepcopy(model_a)
        opt_a = optim.FusedAdam(optim.FlatArena(model_a), lr=2e-3, schedule=optim.OneCycle(2e-3, 40))
        opt_b = optim.FusedAdam(optim.FlatArena(model_b), lr=2e-3, schedule=optim.OneCycle(2e-3, 40))
        sa, sb = _sampler(gpe, 12, 12, 3), _sampler(gpe, 12, 12, 3)
        idx = torch.tensor([SMALL, CLAIMED, GAPS]).cuda()
        metrics = ('edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall')
        eager = []
        for _ in range(5):
            rows, labels = sa.sample(idx)
            loss, d = model_a.loss(model_a(rows), labels)[:2]
            loss.backward()
            opt_a.step()
            eager.append([loss.detach().clone()] + [d[k].detach().clone() for k in metrics])
        sg = graph.StepGraph(lambda i: (lambda r, y: model_b.loss(model_b(r), y)[:2])(*sb.sample(i)), opt_b, warmup=2)
        replayed = []
        for _ in range(5):
            loss = sg.step(idx)
            replayed.append([loss.detach().clone()] + [sg.extras[0][k].clone() for k in metrics])
        sg.synchronize()
        torch.cuda.synchronize()
        assert sg.captures == 1 and sg.replays == 3
        for i, (e, r) in enumerate(zip(eager, replayed)):
            for k, x, y in zip(('loss',) + metrics, e, r):
                assert torch.equal(x, y), (i, k, float(x), float(y))
        assert len({float(e[0]) for e in eager}) == 5
        for (n, p), q in zip(model_a.named_parameters(), model_b.parameters()):
            assert torch.equal(p, q), n
        assert sa.state.cpu().tolist() == sb.state.cpu().tolist() == [SEED - 2 ** 64, 5]
    finally:
        gpe.set_math(prev)


def test_training_on_fresh_pairs_lowers_the_all_pairs_loss(gpe):
    """twenty FusedAdam steps on small + claimed + full, new pairs every step: the pooled loss of evaluate_stitches on those garments
    ends below its initial value (a direction, not a threshold)"""
    from gpe_amd import optim
    gs = _set()
    torch.manual_seed(3)
    model = gpe.nets.StitchOnEdge3DPairs({'element_size': 16}, {}, {}).cuda()
    opt = optim.FusedAdam(optim.FlatArena(model), lr=2e-3)
    pick = [SMALL, CLAIMED, FULL]
    edges, ne, gt, num = [t[pick] for t in _device_set()]
    stats = {'f_shift': gs['shift'], 'f_scale': gs['scale']}

    def pooled():
        model.eval()
        loss = model.evaluate_stitches(edges, ne, gt, num, stats)[1]['edge_pair_class_loss'].item()
        model.train()
        return loss
    before = pooled()
    s = _sampler(gpe, 60, 60, 3, seed=1)
    idx = torch.tensor(pick + pick).cuda()
    losses = []
    for _ in range(20):
        rows, labels = s.sample(idx)
        loss = model.loss(model(rows), labels)[0]
        loss.backward()
        opt.step()
        losses.append(loss.item())
    after = pooled()
    print('pooled all-pairs loss %.4f -> %.4f; training losses %s' % (before, after, ' '.join('%.3f' % v for v in losses)))
    assert s.status.cpu().tolist() == [0] * 6 and s.state.cpu().tolist()[1] == 20
    assert after < before

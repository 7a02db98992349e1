"""Epochs fed from the device (csrc/gpe_epoch_feed.hip, staging.BalancedBatchSchedule / EpochFeeder):
  (1) the schedule of three consecutive epochs, bit-exact against the host restatement (tests/batch_schedule_restate.py), on the
      shapes of tests/test_epoch_feed_host.py and on class sizes [1025, 513, 64] at B = 30 (the ranking crosses workgroups and key
      tiles), again under a CU reservation;
  (2) the per-step feed: the index rows in order, wrapping, and every gathered table equal to torch.index_select, for row sizes
      4 .. 2576 bytes on the 16-byte and the 4-byte copy path; a -1 entry gives a row of zeros and is counted;
  (3) a captured training step that feeds itself equals, bit for bit, the same step handed the same rows from the host: the stitch
      classifier on the six stitch_pairs_* garments, and GarmentFullPattern3D on the meshes of tests/test_gpu_mesh_sample.py.
      The clouds have N = 64 points, the smallest size at which another test runs the encoder's kernels (test_knn_bit_exact): what
      _check_cloud admits goes down to N = k = 5, a shape of kernels this feature does not touch and no test has run."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import batch_schedule_restate as R
import stitch_sample_restate as SR
from test_epoch_feed_host import CASES, SIZES, class_lists

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SEED = 0xfeedc0de12345678                     # a non-zero high half
CARRY = 2 ** 32 - 2                           # the third epoch carries into the counter's fourth word
WIDE = ([1025, 513, 64], 30, True)


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _ids(sizes):
    return class_lists(sizes, first=5, step=3)


@functools.lru_cache(maxsize=None)
def _want(sizes, B, drop_last, epoch):
    """computed once per case and shared"""
    d = R.draw(_ids(list(sizes)), R.quotas(list(sizes), B), B, drop_last, SEED, epoch)
    return d['table'], d['batch_len']


def _schedule(gpe, sizes, B, drop_last, epoch0):
    s = gpe.staging.BalancedBatchSchedule({'type %d' % c: l for c, l in enumerate(_ids(sizes))}, B, drop_last=drop_last, seed=SEED)
    s.reseed(SEED, epoch0)
    return s


def _three_epochs(gpe, sizes, B, drop_last):
    s = _schedule(gpe, sizes, B, drop_last, CARRY)
    G = sum(sizes)
    assert s.quotas == R.quotas(sizes, B) and len(s) == G // B + (1 if (not drop_last and G % B) else 0)
    out = []
    for e in range(3):
        s.draw()
        out.append((s.table.cpu().numpy().copy(), s.batch_len.cpu().numpy().copy()))
    assert s.state.cpu().tolist() == [SEED - 2 ** 64, CARRY + 3] and int(s.cursor) == 0
    return out


@pytest.mark.parametrize('sizes, B, drop_last', CASES + [WIDE], ids=lambda v: str(v).replace(' ', ''))
def test_schedule_bit_exact_against_the_restatement(gpe, sizes, B, drop_last):
    got = _three_epochs(gpe, sizes, B, drop_last)
    for e, (table, blen) in enumerate(got):
        want = _want(tuple(sizes), B, drop_last, CARRY + e)
        assert table.dtype == np.int32 and np.array_equal(blen, want[1]), e
        assert np.array_equal(table, want[0]), e
    assert not np.array_equal(got[0][0], got[1][0])
    prev = gpe.set_reserved_cus(160)
    try:
        again = _three_epochs(gpe, sizes, B, drop_last)
    finally:
        gpe.set_reserved_cus(prev)
    for (t0, l0), (t1, l1) in zip(got, again):
        assert t0.tobytes() == t1.tobytes() and l0.tobytes() == l1.tobytes()


def test_host_table_and_reseed(gpe):
    s = _schedule(gpe, SIZES, 5, False, 7)
    s.draw()
    first = s.host_table()
    assert first.dtype == torch.int32 and tuple(first.shape) == (5, 5) and first[4].tolist().count(-1) == 1
    assert np.array_equal(first.numpy(), _want(tuple(SIZES), 5, False, 7)[0])
    s.draw()
    assert not torch.equal(s.host_table(), first)
    s.reseed(SEED, 7)
    s.draw()
    assert torch.equal(s.host_table(), first)


def _tables(G, misaligned):
    """row sizes 4, 12, 16, 224 and 2576 bytes in mixed dtypes; the last is the row of a [23, 14, 2] fp32 outline table.  misaligned:
    the 4-byte tables start 4 bytes past a 16-byte boundary, so their rows of 224 and 2576 bytes too take the 4-byte copies"""
    g = torch.Generator().manual_seed(G)
    made = [torch.randint(-5, 50, (G,), generator=g, dtype=torch.int32),
            torch.randn(G, 3, generator=g),
            torch.randint(-2 ** 40, 2 ** 40, (G, 2), generator=g, dtype=torch.int64),
            (torch.rand(G, 224, generator=g) < 0.5).to(torch.uint8),                   # a bool mask as bytes, padded to 4
            torch.randn(G, 23, 14, 2, generator=g)]
    out = []
    for t in made:
        if misaligned and t.dtype != torch.int64:
            n = t.numel() * t.element_size()
            raw = torch.zeros(n + 16, dtype=torch.uint8, device='cuda')
            view = raw[4:4 + n].view(t.dtype).view(t.shape)
            view.copy_(t)
            assert view.data_ptr() % 16 == 4
            out.append(view)
        else:
            out.append(t.cuda())
    return out


@pytest.mark.parametrize('misaligned', [False, True], ids=['aligned', 'misaligned'])
def test_feed_bit_exact(gpe, misaligned):
    ops = gpe.ops
    B = 5
    s = _schedule(gpe, SIZES, B, False, 0)                       # five rows, the last a kept remainder of four: one -1
    s.draw()
    host = s.host_table()
    rows = host.shape[0]
    ids = torch.tensor(sorted(g for l in _ids(SIZES) for g in l))
    G = int(ids.max()) + 1
    tables = _tables(G, misaligned)
    outs = [torch.full((B,) + tuple(t.shape[1:]), 77, dtype=t.dtype, device='cuda') for t in tables]
    jobs, widest = ops.feed_jobs(tables, outs)
    assert widest == 2576 and jobs.cpu()[:, 2].tolist() == [4, 12, 16, 224, 2576]
    index = torch.full((B,), -7, dtype=torch.int32, device='cuda')
    status = torch.full((1,), -7, dtype=torch.int32, device='cuda')

    def check(call, G_eff):
        want = host[call % rows]
        assert torch.equal(index.cpu(), want), call
        valid = (want >= 0) & (want < G_eff)
        assert int(status) == int((~valid).sum()), call
        for t, o in zip(tables, outs):
            ref = torch.zeros_like(o).cpu()
            ref[valid] = torch.index_select(t.cpu(), 0, want[valid].long())
            assert torch.equal(o.cpu(), ref), (call, t.dtype, tuple(t.shape))
        assert int(s.cursor) == call + 1
        return int((~valid).sum())

    for call in range(rows + 2):
        ops.feed_next(s.table, s.cursor, G, jobs, widest, index, status)
        assert check(call, G) == (1 if call % rows == rows - 1 else 0)
    # an entry past the tables is a row of zeros as well, and the index alone can be fed (no job)
    ops.feed_next(s.table, s.cursor, 20, jobs, widest, index, status)
    assert check(rows + 2, 20) > 0
    ops.feed_next(s.table, s.cursor, G, None, 0, index, status)
    assert torch.equal(index.cpu(), host[(rows + 3) % rows]) and int(s.cursor) == rows + 4 and int(status) == 0


class _EchoSampler:
    """stands in for a sampler: the clouds are the index"""

    def __init__(self, G):
        self.edges3d = torch.empty(G, 1)

    def sample(self, index):
        return index.clone(), index.clone()


def test_feeder_outputs_and_checks(gpe):
    staging = gpe.staging
    s = _schedule(gpe, SIZES, 5, True, 3)
    G = 80
    g = torch.Generator().manual_seed(1)
    gt = {'outlines': torch.randn(G, 23, 14, 2, generator=g), 'empty_panels_mask': torch.rand(G, 23, generator=g) < 0.5,
          'num_panels': torch.randint(1, 23, (G,), generator=g), 'tiny': torch.randint(-9, 9, (G, 3), generator=g, dtype=torch.int16)}
    f = staging.EpochFeeder(s, _EchoSampler(G), gt)
    assert len(f) == 4 and f.index.dtype == torch.int32 and f.jobs.shape[0] == 4
    f.begin_epoch()
    host = s.host_table()
    kept = {k: v for k, v in f.gt.items()}
    for step in range(len(f) + 1):
        feats, batch = f.next()
        want = host[step % 4].long()
        assert torch.equal(feats.cpu().long(), want) and int(f.status) == 0
        assert set(batch) == set(gt) | {'segmentation'} and batch is f.last_gt
        for k, v in gt.items():
            assert batch[k] is kept[k] and batch[k].dtype == v.dtype and tuple(batch[k].shape) == (5,) + tuple(v.shape[1:])
            assert torch.equal(batch[k].cpu(), v[want]), (step, k)
    f.begin_epoch()
    assert int(s.cursor) == 0 and not torch.equal(s.host_table(), host)
    with pytest.raises(ValueError, match='full batches'):
        staging.EpochFeeder(_schedule(gpe, SIZES, 5, False, 0), _EchoSampler(G), gt)
    with pytest.raises(ValueError, match='garments'):
        staging.EpochFeeder(s, _EchoSampler(G), {'a': torch.zeros(G, 2), 'b': torch.zeros(G + 1, 2)})
    with pytest.raises(ValueError, match='16'):
        staging.EpochFeeder(s, _EchoSampler(G), {'t%d' % i: torch.zeros(G, 2) for i in range(17)})


# ---- (3) captured and self-fed equals host-fed ---------------------------------------------------------------------------------------

NSTEPS = 7                                    # two warm-up steps, one capture, four replays


def _params_equal(a, b):
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n
    for (n, p), q in zip(a.named_buffers(), b.buffers()):
        assert torch.equal(p, q), n


def test_captured_stitch_training_equals_host_fed(gpe):
    from gpe_amd import optim, graph, staging
    gs = SR.resident_set(GOLDEN)
    dev = [torch.from_numpy(gs[k]).cuda() for k in ('edges', 'num_edges', 'gt', 'gt_num')]
    stats = {'f_shift': gs['shift'], 'f_scale': gs['scale']}
    ids = {'upper': [0, 1, 2], 'lower': [3, 4, 5]}
    prev = gpe.set_math('f32')
    try:
        torch.manual_seed(5)
        model_a = gpe.nets.StitchOnEdge3DPairs({'element_size': 16}, {}, {}).cuda().train()
        model_b = copy.deepcopy(model_a)
        opts = [optim.FusedAdam(optim.FlatArena(m), lr=2e-3, schedule=optim.OneCycle(2e-3, 40)) for m in (model_a, model_b)]
        samplers = [staging.StitchPairSampler(*dev, stats, 40, 40, seed=SEED) for _ in range(2)]
        scheds = [staging.BalancedBatchSchedule(ids, 4, seed=11) for _ in range(2)]
        assert scheds[0].quotas == [2, 2] and len(scheds[0]) == 1

        feeder = staging.EpochFeeder(scheds[0], samplers[0])
        sg_a = graph.StepGraph(lambda: (lambda r, y: model_a.loss(model_a(r), y)[:2])(*feeder.next()), opts[0], warmup=2)
        fed = []
        for step in range(NSTEPS):
            if step % len(feeder) == 0:
                feeder.begin_epoch()
            fed.append(sg_a.step().detach().clone())
        sg_a.synchronize()

        sg_b = graph.StepGraph(lambda i: (lambda r, y: model_b.loss(model_b(r), y)[:2])(*samplers[1].sample(i)), opts[1], warmup=2)
        handed, seen = [], []
        for step in range(NSTEPS):
            if step % len(scheds[1]) == 0:
                scheds[1].draw()
                rows = scheds[1].host_table()
            seen.append(rows[step % len(scheds[1])].tolist())
            handed.append(sg_b.step(rows[step % len(scheds[1])]).detach().clone())
        sg_b.synchronize()
        torch.cuda.synchronize()
        assert sg_a.captures == sg_b.captures == 1 and sg_a.replays == sg_b.replays == NSTEPS - 2
        for i, (x, y) in enumerate(zip(fed, handed)):
            assert torch.equal(x, y), (i, float(x), float(y))
        assert len({float(x) for x in fed}) == NSTEPS and len({tuple(r) for r in seen}) > 1
        _params_equal(model_a, model_b)
        assert feeder.index.cpu().tolist() == seen[-1] and int(feeder.status) == 0
        assert scheds[0].state.cpu().tolist() == scheds[1].state.cpu().tolist() == [11, NSTEPS]
        assert samplers[0].state.cpu().tolist() == samplers[1].state.cpu().tolist() == [SEED - 2 ** 64, NSTEPS]
    finally:
        gpe.set_math(prev)


def test_captured_pattern_training_equals_host_fed(gpe):
    from gpe_amd import configs, nets, optim, graph, staging
    import bench
    import test_gpu_mesh_sample as M
    prev = gpe.set_math('f32')
    try:
        dev = torch.device('cuda', 0)
        N, B = 64, 4
        data_config = configs.data_config()
        nn_cfg = configs.lstm_model_config(k_neighbors=5)
        torch.manual_seed(0)
        model_a = nets.GarmentFullPattern3D(data_config, dict(nn_cfg), dict(nn_cfg['loss'])).to(dev).train()
        model_a.loss.with_quality_eval = False
        model_b = copy.deepcopy(model_a)
        _, gt = bench.synthetic(5, N, data_config, seed=1000, device='cpu')             # the ground truth of the five meshes
        opts = [optim.FusedAdam(optim.FlatArena(m), lr=2e-3, schedule=optim.OneCycle(2e-3, 40)) for m in (model_a, model_b)]
        samplers = [M._sampler(gpe, N, stats=True, noise=0.01) for _ in range(2)]
        # twelve slots over the four meshes with labelled vertices: three rows of four per epoch, quotas 3 and 1
        ids = {'dresses': [M.PART, M.STRIP, M.TWELVE] * 3, 'skirts': [M.TRIANGLE, M.STRIP, M.PART]}
        scheds = [staging.BalancedBatchSchedule(ids, B, seed=3) for _ in range(2)]
        assert scheds[0].quotas == [3, 1] and len(scheds[0]) == 3

        feeder = staging.EpochFeeder(scheds[0], samplers[0], gt)
        sg_a = graph.StepGraph(lambda: model_a.loss(model_a(feeder.next()[0]), feeder.last_gt, epoch=0)[0], opts[0], warmup=2)
        fed = []
        for step in range(NSTEPS):
            if step % len(feeder) == 0:
                feeder.begin_epoch()
            torch.manual_seed(100 + step)
            fed.append(sg_a.step().detach().clone())
        sg_a.synchronize()
        assert 'segmentation' in feeder.last_gt and tuple(feeder.last_gt['segmentation'].shape) == (B, N)

        sg_b = graph.StepGraph(lambda i, g: model_b.loss(model_b(samplers[1].sample(i)[0]), g, epoch=0)[0], opts[1], warmup=2)
        handed = []
        for step in range(NSTEPS):
            if step % len(scheds[1]) == 0:
                scheds[1].draw()
                rows = scheds[1].host_table()
            row = rows[step % len(scheds[1])]
            torch.manual_seed(100 + step)
            handed.append(sg_b.step(row, {k: v[row.long()] for k, v in gt.items()}).detach().clone())
        sg_b.synchronize()
        torch.cuda.synchronize()
        assert sg_a.captures == sg_b.captures == 1 and sg_a.replays == sg_b.replays == NSTEPS - 2
        for i, (x, y) in enumerate(zip(fed, handed)):
            assert torch.equal(x, y), (i, float(x), float(y))
        assert len({float(x) for x in fed}) == NSTEPS
        _params_equal(model_a, model_b)
        assert samplers[0].status.cpu().tolist() == samplers[1].status.cpu().tolist() == [0] * B and int(feeder.status) == 0
    finally:
        gpe.set_math(prev)

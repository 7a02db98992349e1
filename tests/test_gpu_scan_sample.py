"""-m gpu: the model's clouds drawn on the device from resident raw scans and the labels handed back (csrc/gpe_scan_sample.hip through
ops.cloud_points_sample / ops.cloud_labels / staging.ScanSampler / model.predict_scans) against the integer- and float32-exact host
restatement (tests/scan_sample_restate.py, which tests/test_scan_sample_host.py holds against np.random.permutation(n)[:N]):
features, picked, status and labels bit for bit, no tolerance anywhere.  Outputs are pre-filled with NaN / -7, so an unwritten row
shows.

The resident set: clouds of 0, 1, 63, 64, 65 and 70 001 points for the mixed batch at N = 64 (an empty and a one-point scan, one
point either side of N, several workgroups per slot with a populated boundary bin), and of 2000, 2011, 5000 and 200 000 points for
the shipped N = 2000.  Every case also runs with narrow_above = 1, which sends every cloud of more than N points whose boundary bin
holds two points or more down the narrowing path of the finishing workgroup: the answer must not move."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import scan_sample_restate as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SIZES = (0, 1, 63, 64, 65, 70001, 2000, 2011, 5000, 200000)
EMPTY, ONE, C63, C64, C65, C70K, C2000, C2011, C5000, C200K = range(10)
G = len(SIZES)
SEED = 0xfeedc0de12345678                     # a non-zero high half
CARRY = 2 ** 32 - 1                           # the next draw carries into the counter's fourth word
STATS = ([0.125, -0.25, 0.0625], [0.75, 1.5, 0.4])
MIXED = (EMPTY, ONE, C63, C64, C65, C70K, -1, G, C70K)
SHIPPED = (C2000, C2011, C5000, C200K)


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


@functools.lru_cache(maxsize=None)
def _clouds():
    rs = np.random.RandomState(11)
    return [rs.uniform(-1, 1, (n, 3)).astype(np.float32) for n in SIZES]


@functools.lru_cache(maxsize=None)
def _resident():
    import gpe_amd
    return gpe_amd.ops.cloud_resident(_clouds())


@functools.lru_cache(maxsize=None)
def _want(index, N, stats, seed, draw):
    """computed once per case and shared"""
    shift, scale = STATS if stats else (None, None)
    return R.sample_batch(_clouds(), list(index), N, seed, draw, shift=shift, scale=scale)


def _sampler(gpe, N, stats=False, seed=SEED, clouds=None):
    data_stats = {'f_shift': STATS[0], 'f_scale': STATS[1]} if stats else None
    return gpe.staging.ScanSampler(clouds if clouds is not None else _resident(), data_stats, mesh_samples=N, seed=seed)


def _same(got, want, what):
    feats, picked, status = got
    assert feats.dtype == torch.float32 and picked.dtype == torch.int32 and status.dtype == torch.int32
    assert status.cpu().tolist() == want[2].tolist(), what
    assert np.array_equal(picked.cpu().numpy(), want[1]), what
    assert np.array_equal(feats.cpu().numpy().view(np.int32), want[0].view(np.int32)), what


def _draw(gpe, index, N, stats, seed, draw, narrow_above=0):
    """one call of ops.cloud_points_sample into pre-filled buffers"""
    ops, res = gpe.ops, _resident()
    out = ops.cloud_points_buffers(res, len(index), N)
    out[0].fill_(float('nan')), out[1].fill_(-7), out[2].fill_(-7)
    state, ticket = ops.stitch_sample_state(seed, draw, res.device), torch.zeros(1, device=res.device, dtype=torch.int32)
    shift, scale = STATS if stats else (None, None)
    got = ops.cloud_points_sample(res, torch.tensor(index, dtype=torch.int32).cuda(), N, state, ticket, shift, scale, out=out,
                                  narrow_above=narrow_above)
    assert got[0] is out[0] and got[1] is out[1] and got[2] is out[2]
    assert state.cpu().tolist()[1] == draw + 1 and int(ticket) == 0
    return got


@pytest.mark.parametrize('narrow_above', [0, 1], ids=['listed', 'narrowed'])
@pytest.mark.parametrize('stats', [False, True], ids=['raw', 'standardized'])
def test_mixed_batch(gpe, stats, narrow_above):
    N = 64
    got = _draw(gpe, MIXED, N, stats, SEED, CARRY, narrow_above)
    want = _want(MIXED, N, stats, SEED, CARRY)
    assert want[2].tolist() == [-1, 63, 1, 0, 0, 0, -2, -2, 0]
    _same(got, want, 'mixed')
    feats, picked = got[0].cpu(), got[1].cpu()
    for b in (0, 6, 7):
        assert not feats[b].any() and (picked[b] == -1).all(), b
    assert not torch.equal(picked[5], picked[8])                                     # the same cloud in two slots: two draws
    assert len(set(picked[5].tolist())) == N and (picked[1] == 0).all()


@pytest.mark.parametrize('narrow_above', [0, 1], ids=['listed', 'narrowed'])
@pytest.mark.parametrize('stats', [False, True], ids=['raw', 'standardized'])
def test_shipped_shape(gpe, stats, narrow_above):
    N = 2000
    got = _draw(gpe, SHIPPED, N, stats, SEED, 3, narrow_above)
    want = _want(SHIPPED, N, stats, SEED, 3)
    assert want[2].tolist() == [0, 0, 0, 0]
    _same(got, want, 'shipped')
    assert sorted(got[1][0].cpu().tolist()) == list(range(2000))                     # n = N: a permutation of the whole scan


def test_largest_sample_count(gpe):
    """N = 2048, the largest the sort's image takes, on clouds below, at and above it"""
    index = (C2000, C5000, C200K, ONE)
    _same(_draw(gpe, index, 2048, True, 5, 0), _want(index, 2048, True, 5, 0), 'N = 2048')
    state, ticket = gpe.ops.stitch_sample_state(5, 0, 'cuda'), torch.zeros(1, device='cuda', dtype=torch.int32)
    with pytest.raises(ValueError, match='1 .. 2048 points'):
        gpe.ops.cloud_points_sample(_resident(), torch.tensor(index, dtype=torch.int32).cuda(), 2049, state, ticket)


def test_sequence_and_reseed(gpe):
    N, index = 64, (C70K, C65, ONE, C70K)
    s = _sampler(gpe, N, stats=True)
    idx = torch.tensor(index).cuda()
    assert s.state.cpu().tolist() == [SEED - 2 ** 64, 0]
    s.reseed(SEED, CARRY)
    a = s.sample(idx) + (s.status,)
    b = s.sample(idx) + (s.status,)
    assert s.state.cpu().tolist() == [SEED - 2 ** 64, CARRY + 2] and int(s.ticket) == 0
    assert not torch.equal(a[1], b[1]) and not torch.equal(a[0], b[0])
    _same(a, _want(index, N, True, SEED, CARRY), 'draw d')
    _same(b, _want(index, N, True, SEED, CARRY + 1), 'draw d + 1')
    s.reseed(SEED, CARRY)
    a2 = s.sample(idx) + (s.status,)
    for x, y in zip(a, a2):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    s.reseed(SEED + 1, CARRY)
    assert not torch.equal(s.sample(idx)[1], a[1])
    cfg = {'mesh_samples': N, 'point_noise_w': 0.125, 'standardize': {'f_shift': STATS[0], 'f_scale': STATS[1]}}
    t = gpe.staging.ScanSampler.from_config(s.resident, cfg, seed=SEED)
    t.reseed(SEED, CARRY)
    got = t.sample(idx)
    assert torch.equal(got[0], a[0]) and torch.equal(got[1], a[1])
    d = gpe.staging.ScanSampler.from_config(s.resident, {})
    assert (d.mesh_samples, d.f_shift, d.f_scale) == (2000, None, None)


def test_captured_call_draws_anew_on_every_replay(gpe):
    N, index = 64, (C70K, C63, EMPTY, C5000)
    s = _sampler(gpe, N, stats=True)
    idx = torch.tensor(index).cuda()
    eager = s.sample(idx) + (s.status,)
    _same(eager, _want(index, N, True, SEED, 0), 'eager')
    s.reseed(SEED)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    replayed = []
    with torch.cuda.stream(side):
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, stream=side):
            feats, picked = s.sample(idx)
        for _ in range(2):
            cg.replay()
            replayed.append((feats.clone(), picked.clone(), s.status.clone()))
    side.synchronize()
    for i, r in enumerate(replayed):
        _same(r, _want(index, N, True, SEED, i), i)
    assert s.state.cpu().tolist()[1] == 2 and int(s.ticket) == 0
    assert not torch.equal(replayed[0][1], replayed[1][1])


def test_identical_under_cu_reservations(gpe):
    N, index = 2000, (C200K, C2011, C70K)
    prev = gpe.get_reserved_cus()
    got = []
    try:
        for cus in (0, 16, 64):
            gpe.set_reserved_cus(cus)
            got.append(_draw(gpe, index, N, True, SEED, 9))
    finally:
        gpe.set_reserved_cus(prev)
    assert gpe.get_reserved_cus() == prev
    for g in got[1:]:
        for x, y in zip(got[0], g):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    _same(got[0], _want(index, N, True, SEED, 9), 'reserved')


# ---- labels ------------------------------------------------------------------------------------------------------------------------------
def _label_clouds():
    """0: 300 points of which 200 are duplicates of the first 100, then A, B and the point M exactly midway between them, far from the
    rest; 1: five points (a short cloud); 2: 700 points nobody asks for; 3: empty; 4: 1100 points (three workgroups)"""
    rs = np.random.RandomState(23)
    base = (rs.randint(-8, 9, (100, 3)) / 8.0).astype(np.float32)
    c0 = np.concatenate([base, base, base[::-1], np.float32([[10, 0, 0], [11, 0, 0], [10.5, 0, 0]])])
    return [c0, (rs.randint(-8, 9, (5, 3)) / 8.0).astype(np.float32), rs.uniform(-1, 1, (700, 3)).astype(np.float32),
            np.zeros((0, 3), dtype=np.float32), rs.uniform(-1, 1, (1100, 3)).astype(np.float32)]


def test_labels(gpe):
    ops, N, P = gpe.ops, 64, 7
    clouds = _label_clouds()
    res = ops.cloud_resident(clouds)
    index = (0, 1, 3, -1, 5, 4, 0)                                                   # cloud 0 twice: slot 6 stands
    rs = np.random.RandomState(29)
    picked = np.stack([rs.randint(0, max(len(clouds[g]), 1) if 0 <= g < 5 else 1, N) for g in index]).astype(np.int32)
    for b in (0, 6):                                                                 # neither draw holds M; rows 0 and 1 are B and A
        picked[b] = rs.randint(0, 300, N)
        picked[b, 0], picked[b, 1] = 301, 300
    picked[1] = R.picked_of(5, N, 1, SEED, 0)[0]                                     # the short cloud: whole permutations repeat
    picked[2] = picked[3] = picked[4] = -1
    att = (rs.randint(0, 4, (len(index), N, P)) / 4.0).astype(np.float32)            # tied weights in almost every row
    assert ((att == att.max(axis=2, keepdims=True)).sum(axis=2) > 1).mean() > 0.5
    want = R.labels(clouds, list(index), picked, att, out=np.full(res.T, -7))
    out = torch.full((res.T,), -7, device='cuda', dtype=torch.int32)
    got = ops.cloud_labels(res, torch.tensor(index, dtype=torch.int32).cuda(), torch.from_numpy(picked).cuda(), torch.from_numpy(att).cuda(),
                           out=out)
    assert got is out and np.array_equal(got.cpu().numpy(), want)
    off = res.off.cpu().tolist()
    assert (want[off[2]:off[3]] == -7).all() and (want[:off[2]] >= 0).all() and (want[off[4]:] >= 0).all()   # cloud 2 is not in the batch
    assert want[302] == np.argmax(att[6, 0]) and want[300] == np.argmax(att[6, 1])   # M: rows 0 and 1 tie at d = 0.25, the lower wins
    # a new tensor starts at -1; bad slots alone write nothing
    fresh = ops.cloud_labels(res, torch.tensor([3, -1, 5], dtype=torch.int32).cuda(), torch.zeros(3, N, dtype=torch.int32).cuda(),
                             torch.from_numpy(att[:3]).cuda())
    assert fresh.shape == (res.T,) and (fresh == -1).all()


def test_labels_of_a_drawn_batch(gpe):
    """the sampler's own picked rows: every drawn point takes its own row's label (the lowest row when rows repeat)"""
    N, P = 64, 5
    clouds = _label_clouds()
    s = gpe.staging.ScanSampler(clouds, None, mesh_samples=N, seed=SEED)
    index = (4, 1, 0)
    with pytest.raises(RuntimeError, match='sample'):
        s.labels(torch.zeros(3, N, P).cuda())
    feats, picked = s.sample(torch.tensor(index).cuda())
    want_draw = R.sample_batch(clouds, list(index), N, SEED, 0)
    _same((feats, picked, s.status), want_draw, 'label batch')
    att = torch.from_numpy(np.random.RandomState(31).uniform(0, 1, (3, N, P)).astype(np.float32)).cuda()
    got = s.labels(att).cpu().numpy()
    assert np.array_equal(got, R.labels(clouds, list(index), want_draw[1], att.cpu().numpy()))
    off = s.resident.off.cpu().tolist()
    assert (got[off[2]:off[4]] == -1).all()


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def _models(gpe, tag, segmentation):
    fx = torch.load(os.path.join(GOLDEN, tag + '.pt'), weights_only=False)
    loss = copy.deepcopy(fx['loss_config'])
    if segmentation:
        loss['loss_components'] = list(loss['loss_components']) + ['segmentation']
    torch.manual_seed(fx['seed'])
    model = getattr(gpe.nets, fx['model'])(fx['data_config'], copy.deepcopy(fx['nn_config']), loss)
    model.load_state_dict(fx['state_dict'])
    known = torch.load(os.path.join(GOLDEN, 'stitch_pairs_known_answer.pt'), weights_only=False)
    stitch = gpe.nets.StitchOnEdge3DPairs(known['data_config'], dict(known['nn_config']), {})
    stitch.load_state_dict(known['state_dict'])
    full = torch.load(os.path.join(GOLDEN, 'stitch_pairs_full.pt'), weights_only=False)
    return fx, model.cuda().eval(), stitch.cuda().eval(), {'f_shift': full['f_shift'], 'f_scale': full['f_scale']}


def _bits_equal(a, b):
    assert tuple(a) == tuple(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), k


def _scans(fx):
    rs = np.random.RandomState(41)
    shift, scale = np.float32(fx['data_config']['standardize']['f_shift']), np.float32(fx['data_config']['standardize']['f_scale'])
    return [(rs.normal(0, 1, (n, 3)) * scale + shift).astype(np.float32) for n in (300, 517)]


def test_predict_scans_segmentation_model(gpe):
    fx, model, stitch, stats = _models(gpe, 'segment3d_small', True)
    dc = fx['data_config']
    N = fx['features'].shape[1]
    s = gpe.staging.ScanSampler.from_config(_scans(fx), {'mesh_samples': N, 'standardize': dc['standardize']}, seed=SEED)
    idx = torch.tensor([1, 0]).cuda()
    torch.manual_seed(5)                                     # the decoders draw their start states on the CPU generator
    d = model.predict_scans(s, idx, dc, stitch, stats)
    s.reseed(SEED, 0)
    feats, picked = s.sample(idx)
    torch.manual_seed(5)
    want = model.predict_garment(feats, dc, stitch, stats)
    torch.manual_seed(5)
    preds = model.predict(feats)
    torch.cuda.synchronize()
    _bits_equal(d.tensors, want.tensors)
    _bits_equal(d.placed, want.placed)
    _bits_equal(d.pairs, want.pairs)
    assert preds['att_weights'].shape == (2, N, dc['max_pattern_len'])
    assert torch.equal(d.scan_picked, picked) and d.scan_labels.dtype == torch.int32 and d.scan_labels.shape == (817,)
    assert torch.equal(d.scan_labels, gpe.ops.cloud_labels(s.resident, idx, picked, preds['att_weights']))
    assert int(d.scan_labels.min()) >= 0 and int(d.scan_labels.max()) < dc['max_pattern_len']
    # without a stitch model: predict_pattern(...).place()
    s.reseed(SEED, 0)
    torch.manual_seed(5)
    e = model.predict_scans(s, idx, dc)
    _bits_equal(e.tensors, want.tensors)
    _bits_equal(e.placed, want.placed)
    assert e.pairs is None and torch.equal(e.scan_labels, d.scan_labels)
    stitch.train()
    with pytest.raises(RuntimeError, match='eval'):
        model.predict_scans(s, idx, dc, stitch, stats)


def test_predict_scans_without_attention_weights(gpe):
    fx, model, stitch, stats = _models(gpe, 'full3d_small', False)
    dc = fx['data_config']
    N = fx['features'].shape[1]
    s = gpe.staging.ScanSampler.from_config(_scans(fx), {'mesh_samples': N, 'standardize': dc['standardize']}, seed=SEED)
    idx = torch.tensor([0, 1]).cuda()
    torch.manual_seed(5)
    d = model.predict_scans(s, idx, dc, stitch, stats)
    s.reseed(SEED, 0)
    torch.manual_seed(5)
    want = model.predict_garment(s.sample(idx)[0], dc, stitch, stats)
    torch.cuda.synchronize()
    _bits_equal(d.tensors, want.tensors)
    _bits_equal(d.pairs, want.pairs)
    assert d.scan_labels is None and d.scan_picked is None

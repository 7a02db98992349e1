"""-m gpu: the encoder's input point clouds drawn on the device (csrc/gpe_mesh_sample.hip through ops.mesh_points_sample /
staging.MeshPointSampler) against the integer-exact host restatement (tests/mesh_sample_restate.py, which
tests/test_mesh_sample_host.py holds against the analytic distribution): features, segmentation and status bit for bit without
noise, the noisy points under a derived bar with the labels exact on the device's own points, the status paths, the generator state,
stream capture, and a captured training step of the pattern model that draws its own clouds.

The resident set is five synthetic garments with coordinates in [-1, 1]: one triangle; the twelve faces of the host tests (one
degenerate); a bent strip of 514 vertices and 511 faces (two LDS tiles of 256 vertices and two more); a mesh whose vertices are all
unlabelled; a grid with every tenth vertex unlabelled."""
import copy
import functools

import numpy as np
import pytest
import torch

import mesh_sample_restate as R

pytestmark = pytest.mark.gpu

TRIANGLE, TWELVE, STRIP, BARE, PART = range(5)
SEED = 0xfeedc0de12345678                     # a non-zero high half
CARRY = 2 ** 32 - 1                           # the next draw carries into the counter's fourth word
STATS = ([0.125, -0.25, 0.0625], [0.75, 1.5, 0.4])
TILE = 256                                    # MS_TILE of csrc/gpe_mesh_sample.hip


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _grid(nx, ny, bend):
    """nx x ny vertices on a bent sheet inside [-1, 1]^3, two triangles per cell"""
    u, v = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny), indexing='ij')
    verts = np.stack([0.9 * np.cos(bend * u) * (0.4 + 0.6 * u), 0.9 * np.sin(bend * u) * (0.4 + 0.6 * u), 1.6 * v - 0.8 + 0.1 * u], axis=-1)
    idx = np.arange(nx * ny).reshape(nx, ny)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)])
    return verts.reshape(-1, 3).astype(np.float32), faces.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _meshes():
    tv, tf, tl = R.twelve_faces()
    tv = tv * np.float32(0.25)                                                       # a power of two: face 7 stays degenerate
    sv, sf = _grid(257, 2, 9.0)
    sf = sf[:-1]
    assert len(sv) == 2 * TILE + 2 and len(sf) == 511
    bv, bf = _grid(4, 3, 1.0)
    pv, pf = _grid(12, 12, 2.0)
    pl = (np.arange(144) // 12) // 4 * 3 + (np.arange(144) % 12) // 4
    pl[3::10] = -1
    meshes = [(np.asarray([[-0.5, -0.25, 0.0], [0.75, 0.0, 0.5], [0.0, 1.0, -1.0]], dtype=np.float32), np.asarray([[0, 1, 2]]),
               np.asarray([2, 2, 5])),
              (tv, tf, tl),
              (sv, sf, np.arange(514) // 2 // 37),
              (bv, bf, np.full(len(bv), -1)),
              (pv, pf, pl)]
    assert all(np.abs(m[0]).max() <= 1 for m in meshes) and (pl < 0).sum() == 15
    return meshes


def _sampler(gpe, N, stats=False, noise=0.0, seed=SEED, meshes=None):
    data_stats = {'f_shift': STATS[0], 'f_scale': STATS[1]} if stats else None
    return gpe.staging.MeshPointSampler(meshes or _meshes(), data_stats, mesh_samples=N, point_noise_w=noise, seed=seed)


@functools.lru_cache(maxsize=None)
def _want(index, N, stats, seed, draw):
    """computed once per case and shared"""
    shift, scale = STATS if stats else (None, None)
    return R.sample_batch(_meshes(), list(index), N, seed, draw, shift=shift, scale=scale)[:3]


def _same(got, want, what):
    feats, seg, status = got
    assert feats.dtype == torch.float32 and seg.dtype == torch.int64 and status.dtype == torch.int32
    assert status.cpu().tolist() == want[2].tolist(), what
    assert np.array_equal(seg.cpu().numpy(), want[1]), what
    assert np.array_equal(feats.cpu().numpy().view(np.int32), want[0].view(np.int32)), what


INDEX = {1: (STRIP,), 3: (PART, TWELVE, PART), 30: tuple((3 * b + b // 5) % 5 for b in range(30))}


@pytest.mark.parametrize('stats', [False, True], ids=['raw', 'standardized'])
@pytest.mark.parametrize('B', [1, 3, 30])
@pytest.mark.parametrize('N', [1, 63, 64, 257, 1024])
def test_bit_exact_against_the_restatement(gpe, N, B, stats):
    index = INDEX[B]
    assert B < 30 or set(index) == set(range(5))
    s = _sampler(gpe, N, stats)
    s.reseed(SEED, CARRY)
    idx = torch.tensor(index).cuda()
    for draw in (CARRY, CARRY + 1):
        feats, seg = s.sample(idx)
        assert feats.shape == (B, N, 3) and seg.shape == (B, N)
        _same((feats, seg, s.status), _want(index, N, stats, SEED, draw), (draw, N, B))
    if B == 3 and N > 1:
        assert not torch.equal(feats[0], feats[2])                                   # the same garment in two slots: two draws
    assert s.state.cpu().tolist() == [SEED - 2 ** 64, CARRY + 2] and int(s.ticket) == 0


def test_noisy_points_and_their_labels(gpe):
    """|p_dev - (p_clean + w z64)| <= w 1e-5 + 2^-23 max|p|: logf, sqrtf and sincospif are each within 2 ulp and 2 u2 is exact, so with
    |z| <= 5.77 the device's z is within 3.1e-6 of the float64 one; the bar is three times that plus the rounding of the add.  The
    labels are the restatement's two passes on the device's own points."""
    w, N = 0.25, 1024
    index = (TRIANGLE, TWELVE, STRIP, BARE, PART, STRIP)
    s = _sampler(gpe, N, noise=w, seed=SEED)
    feats, seg = s.sample(torch.tensor(index, dtype=torch.int32).cuda())
    feats, seg, status = feats.cpu().numpy(), seg.cpu().numpy(), s.status.cpu().tolist()
    dec = R.sample_batch(_meshes(), list(index), N, SEED, 0, noise_w=w)[3]
    want = np.stack([d['clean'].astype(np.float64) + w * d['z'] for d in dec])
    err, bar = np.abs(feats - want).max(), w * 1e-5 + 2.0 ** -23 * np.abs(want).max()
    print('noisy points: max |p_dev - (p_clean + w z64)| = %.3e (bar %.3e), max |w z| = %.3f' % (err, bar, w * max(np.abs(d['z']).max() for d in dec)))
    assert err <= bar
    assert np.abs(feats - np.stack([d['clean'] for d in dec])).max() > 0.5           # the noise is there
    meshes = _meshes()
    for b, g in enumerate(index):
        labels, fell = R.labels_of(feats[b], meshes[g][0], meshes[g][2])
        assert status[b] == fell == (N if g == BARE else 0), b
        assert np.array_equal(seg[b], labels), b
    assert (seg[4] >= 0).all() and (seg >= 0).all()


def test_status_paths(gpe):
    N = 70
    s = _sampler(gpe, N, stats=True)
    index = (-1, BARE, 5, TWELVE, -7, 10 ** 9)
    feats, seg = s.sample(torch.tensor(index).cuda())
    assert s.status.cpu().tolist() == [-2, N, -2, 0, -2, -2]
    for b in (0, 2, 4, 5):
        assert not feats[b].any() and not seg[b].any(), b
    assert not seg[1].any() and feats[1].any()
    _same((feats, seg, s.status), R.sample_batch(_meshes(), list(index), N, SEED, 0, shift=STATS[0], scale=STATS[1])[:3], 'status paths')
    # a garment whose faces are all degenerate, in front of a sound one
    tv = _meshes()[TWELVE][0]
    flat = (tv, np.asarray([[0, 0, 1], [4, 4, 4], [21, 22, 23]]), np.zeros(len(tv), dtype=np.int64))
    two = [flat, _meshes()[TRIANGLE]]
    s = _sampler(gpe, N, meshes=two)
    feats, seg = s.sample(torch.tensor([0, 1, 0], dtype=torch.int32).cuda())
    assert s.status.cpu().tolist() == [-1, 0, -1]
    assert not feats[0].any() and not feats[2].any() and not seg[0].any() and not seg[2].any() and feats[1].any()
    _same((feats, seg, s.status), R.sample_batch(two, [0, 1, 0], N, SEED, 0)[:3], 'degenerate')


def test_state_advances_and_reseed_reproduces(gpe):
    s = _sampler(gpe, 600, stats=True, noise=0.125)
    idx = torch.tensor([PART, STRIP, PART]).cuda()
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
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert s.state.cpu().tolist()[1] == 2 and int(s.ticket) == 0
    s.reseed(SEED, 1)
    assert torch.equal(s.sample(idx)[0], b[0])
    s.reseed(SEED + 1)
    assert not torch.equal(s.sample(idx)[0], a[0])
    cfg = {'mesh_samples': 600, 'point_noise_w': 0.125, 'standardize': {'f_shift': STATS[0], 'f_scale': STATS[1]}, 'obj_filetag': 'sim'}
    t = gpe.staging.MeshPointSampler.from_config(s.resident, cfg, seed=SEED)
    got = t.sample(idx)
    assert torch.equal(got[0], a[0]) and torch.equal(got[1], a[1])
    d = gpe.staging.MeshPointSampler.from_config(s.resident, {})
    assert (d.mesh_samples, d.point_noise_w, d.f_shift, d.f_scale) == (2000, 0.0, None, None)


def test_captured_call_draws_anew_on_every_replay(gpe):
    index = (PART, TWELVE, STRIP, PART)
    s = _sampler(gpe, 257, stats=True)
    idx = torch.tensor(index).cuda()
    eager = []
    for _ in range(3):
        feats, seg = s.sample(idx)
        eager.append((feats.clone(), seg.clone(), s.status.clone()))
    s.reseed(SEED)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    replayed = []
    with torch.cuda.stream(side):
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, stream=side):
            feats, seg = s.sample(idx)
        for _ in range(3):
            cg.replay()
            replayed.append((feats.clone(), seg.clone(), s.status.clone()))
    side.synchronize()
    for i, (e, r) in enumerate(zip(eager, replayed)):
        for x, y in zip(e, r):
            assert torch.equal(x, y), i
        _same(r, _want(index, 257, True, SEED, i), i)
    assert s.state.cpu().tolist()[1] == 3 and int(s.ticket) == 0
    assert not torch.equal(replayed[0][0], replayed[1][0]) and not torch.equal(replayed[1][0], replayed[2][0])


def test_captured_step_with_the_sampler_inside(gpe):
    """five steps of StepGraph(warmup=2) of GarmentFullPattern3D drawing their own clouds equal five eager steps: f32, N = 256,
    batch 4, k = 5, ground truth from bench.synthetic"""
    from gpe_amd import configs, nets, optim, graph
    import bench
    prev = gpe.set_math('f32')
    try:
        dev = torch.device('cuda', 0)
        data_config = configs.data_config()
        nn_cfg = configs.lstm_model_config(k_neighbors=5)
        torch.manual_seed(0)
        model_a = nets.GarmentFullPattern3D(data_config, dict(nn_cfg), dict(nn_cfg['loss'])).to(dev).train()
        model_a.loss.with_quality_eval = False
        model_b = copy.deepcopy(model_a)
        _, gt = bench.synthetic(4, 256, data_config, seed=1000, device=dev)
        opt_a = optim.FusedAdam(optim.FlatArena(model_a), lr=2e-3, schedule=optim.OneCycle(2e-3, 40))
        opt_b = optim.FusedAdam(optim.FlatArena(model_b), lr=2e-3, schedule=optim.OneCycle(2e-3, 40))
        sa, sb = _sampler(gpe, 256, stats=True, noise=0.01), _sampler(gpe, 256, stats=True, noise=0.01)
        idx = torch.tensor([PART, STRIP, TWELVE, PART]).cuda()
        eager = []
        for i in range(5):
            torch.manual_seed(100 + i)
            loss = model_a.loss(model_a(sa.sample(idx)[0]), gt, epoch=0)[0]
            loss.backward()
            opt_a.step()
            eager.append(loss.detach().clone())
        sg = graph.StepGraph(lambda i, g: model_b.loss(model_b(sb.sample(i)[0]), g, epoch=0)[0], opt_b, warmup=2)
        replayed = []
        for i in range(5):
            torch.manual_seed(100 + i)
            replayed.append(sg.step(idx, gt).detach().clone())
        sg.synchronize()
        torch.cuda.synchronize()
        assert sg.captures == 1 and sg.replays == 3
        for i, (e, r) in enumerate(zip(eager, replayed)):
            assert torch.equal(e, r), (i, float(e), float(r))
        assert len({float(e) for e in eager}) == 5
        for (n, p), q in zip(model_a.named_parameters(), model_b.parameters()):
            assert torch.equal(p, q), n
        assert sa.state.cpu().tolist() == sb.state.cpu().tolist() == [SEED - 2 ** 64, 5]
        assert sa.status.cpu().tolist() == sb.status.cpu().tolist() == [0] * 4
    finally:
        gpe.set_math(prev)

"""-m gpu: the statistics fit on the device (csrc/gpe_fit_stats.hip through ops.FitAccumulator, staging.MeshPointSampler /
StitchPairSampler.fit_feature_stats and staging.fit_pattern_standardization) against the float64 restatement of the reference's
formulas (tests/fit_stats_restate.py, which tests/test_fit_stats_host.py holds against the reference's own results) on the same
fp32 inputs.

Bars: n, min, max and norm_scale are bit-equal after the one rounding to fp32.  mean and std lie within one fp32 ulp of the
fp32-rounded restatement: the device's fp64 sums and merges are accurate to about n 1e-16 relative to max|x|, far below half an fp32
ulp of a std that is >= 1e-3 max|x| and a mean that is >= 1e-4 max|x| (_compare checks that every input is built that way), and
the single ulp covers a value that sits on a rounding boundary.  std is exactly 0 on a constant column.  The result block is bit-identical for every grid size, CU reservation
and chunking."""
import functools
import os

import numpy as np
import pytest
import torch

import fit_stats_restate as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SEED = 0xfeedc0de12345678


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _input(S, N, C, padded, seed=0):
    """fp32 [S, N, C]: column c is normal with sigma 2^c / 8 around +-2 sigma (|mean| and std both well above 1e-3 max|x|); the last
    column of C >= 3 is constant (as long as no padding is put in).  padded: about a third of the rows are zero and a tenth lie under
    _unpad's tolerance in every column (dropped), a twentieth have one column over it (kept); row 0 of set 0 is always kept."""
    rng = np.random.default_rng(1000 * C + 10 * N + S + (500000 if padded else 0) + seed)
    sigma = 2.0 ** np.arange(C) / 8
    x = (rng.normal(0, 1, (S, N, C)) * sigma + 2 * sigma * (-1) ** np.arange(C)).astype(np.float32)
    if C >= 3:
        x[..., C - 1] = -3.25
    if padded:
        u = rng.random((S, N))
        x[u < 0.33] = 0
        tiny = (u >= 0.33) & (u < 0.43)
        x[tiny] = (rng.uniform(-1, 1, (int(tiny.sum()), C)) * 9e-6).astype(np.float32)
        near = (u >= 0.43) & (u < 0.48)
        x[near] = 0
        x[near, 0] = 2e-5
        x[0, 0] = sigma * 3 + 1
    return x


def _fit(gpe, x, padded, chunks=None):
    """-> (result block fp64 on the device, the accumulator)"""
    S, N, C = x.shape
    acc = gpe.ops.FitAccumulator(C, S, N, 'cuda', padded=padded)
    d = torch.from_numpy(x).cuda()
    s0 = 0
    for n in chunks or (S,):
        acc.add(d[s0:s0 + n])
        s0 += n
    return acc.finish(), acc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _compare(got, x, padded, what, constant=()):
    w = R.all_stats(x, padded)
    assert got['n'] == w['n'] and got['status'] == 0, what
    top = np.abs(R.unpad(x) if padded else R.rows(x)).max(axis=0)
    assert (((w['std'] >= 1e-3 * top) | (w['min'] == w['max'])) & (np.abs(w['mean']) >= 1e-4 * top)).all(), what     # the inputs the bars are for
    for k in ('min', 'max', 'norm_scale'):
        assert np.array_equal(_bits(got[k]), _bits(R.f32(w[k]))), (what, k, got[k], w[k])
    for k in ('mean', 'std'):
        want = R.f32(w[k])
        d, ulp = np.abs(got[k].astype(np.float64) - want.astype(np.float64)), R.ulp32(want)
        print('%s %s: |device - restatement| in ulps %s' % (what, k, d / ulp))
        assert got[k].dtype == np.float32 and (d <= ulp).all(), (what, k, got[k], want)
    for c in constant:
        assert got['std'][c] == 0.0 and w['std'][c] == 0.0, (what, c)


@pytest.mark.parametrize('C', [1, 3, 4, 16])
@pytest.mark.parametrize('N', [1, 511, 512, 513, 1025])
def test_parity_with_the_restatement(gpe, N, C):
    for S in (1, 3):
        for padded in (False, True):
            x = _input(S, N, C, padded)
            block, acc = _fit(gpe, x, padded)
            assert block.dtype == torch.float64 and block.shape == (2 + 5 * C,) and block.is_cuda
            assert acc.leaves == S * ((N + 511) // 512)
            _compare(acc.read(), x, padded, (S, N, C, padded), constant=(C - 1,) if C >= 3 and not padded else ())


@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('S,N,C', [(300, 23, 4), (2500, 5, 3)])
def test_more_leaves_than_finishing_threads_and_than_workgroups(gpe, S, N, C, padded):
    """300 x 23: the ground-truth shape, 300 one-leaf sets; 2500 x 5: more leaves than the largest grid (8 per CU), so workgroups
    take several leaves, and more than the 1024 threads of the finish"""
    x = _input(S, N, C, padded)
    _compare(_fit(gpe, x, padded)[1].read(), x, padded, (S, N, C, padded), constant=() if padded else (C - 1,))


def test_an_empty_leaf_and_an_empty_fit(gpe):
    x = _input(1, 1025, 3, True)
    x[0, 512:1024] = 0                                      # the second of three leaves keeps no row
    block, acc = _fit(gpe, x, True)
    rec = acc.part.cpu().numpy()
    assert rec.shape == (3, 13) and rec[1, 0] == 0 and rec[0, 0] > 0 and rec[2, 0] in (0, 1)
    assert rec[1, 1:].reshape(3, 4).tolist() == [[0.0, 0.0, float('inf'), float('-inf')]] * 3
    _compare(acc.read(), x, True, 'empty leaf')
    z = np.zeros((2, 600, 3), dtype=np.float32)
    z[1, 17] = [9e-6, -1e-5, 0]                             # at the tolerance: still padding
    block, acc = _fit(gpe, z, True)
    b = block.cpu().numpy()
    assert b[0] == 0 and int(b[1]) == gpe.ops.FIT_STATUS_EMPTY and np.isnan(b[2:]).all()
    with pytest.raises(ValueError, match='no row'):
        acc.read()
    # the same rows count when padding is not looked for
    got = _fit(gpe, z, False)[1].read()
    assert got['n'] == 1200 and got['norm_scale'].tolist()[2] == 1.0 and got['max'].tolist()[0] == float(np.float32(9e-6))


def test_a_nan_marks_its_column_and_the_status(gpe):
    x = _input(3, 513, 4, False)
    x[1, 512, 1] = np.nan
    got = _fit(gpe, x, False)[1].read()
    w = R.all_stats(x, False)
    assert got['status'] == gpe.ops.FIT_STATUS_NONFINITE and got['n'] == 3 * 513
    for k in ('mean', 'std', 'min', 'max', 'norm_scale'):
        assert np.isnan(got[k]).tolist() == [False, True, False, False] == np.isnan(w[k]).tolist(), k
    for k in ('min', 'max', 'norm_scale'):
        assert np.array_equal(_bits(got[k])[[0, 2, 3]], _bits(R.f32(w[k]))[[0, 2, 3]]), k
    x[1, 512, 1] = np.inf
    got = _fit(gpe, x, False)[1].read()
    assert got['status'] == gpe.ops.FIT_STATUS_NONFINITE and got['max'][1] == np.inf and np.isfinite(got['min']).all()


@pytest.mark.parametrize('S,N,C,chunks', [(7, 1025, 3, (1, 4, 2)), (2500, 5, 3, (1200, 1, 1299)), (9, 700, 16, (2, 6, 1))])
def test_bit_identical_for_every_grid_reservation_and_chunking(gpe, S, N, C, chunks):
    x = _input(S, N, C, True, seed=7)
    same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))          # noqa: E731
    first, acc = _fit(gpe, x, True)
    part = acc.part.clone()
    again, acc2 = _fit(gpe, x, True)
    assert same(first, again) and same(part, acc2.part)
    prev = gpe.set_reserved_cus(0)
    try:
        a, acc_a = _fit(gpe, x, True)
        gpe.set_reserved_cus(64)
        b, acc_b = _fit(gpe, x, True)
    finally:
        gpe.set_reserved_cus(prev)
    assert same(first, a) and same(first, b) and same(part, acc_a.part) and same(part, acc_b.part)
    c, acc_c = _fit(gpe, x, True, chunks)
    assert sum(chunks) == S and same(first, c) and same(part, acc_c.part)
    # the accumulator's bookkeeping
    acc = gpe.ops.FitAccumulator(C, S, N, 'cuda')
    d = torch.from_numpy(x).cuda()
    with pytest.raises(ValueError, match='announced'):
        acc.finish()
    for bad in (d[:1, :N - 1], d[:1, :, :C - 1], d[:1].double(), d[0], d[:1].cpu()):
        with pytest.raises(ValueError, match='FitAccumulator.add'):
            acc.add(bad)
    acc.add(d[:S - 1])
    with pytest.raises(ValueError, match='announced'):
        acc.add(d[:2])
    with pytest.raises(ValueError, match='announced'):
        acc.read()


# ---- MeshPointSampler.fit_feature_stats --------------------------------------------------------------------------------------------

def _sheet(nx, ny, bend, scale, shift):
    u, v = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny), indexing='ij')
    verts = np.stack([np.cos(bend * u) * (0.4 + 0.6 * u), np.sin(bend * u) * (0.4 + 0.6 * u), 1.6 * v - 0.8 + 0.1 * u], axis=-1)
    idx = np.arange(nx * ny).reshape(nx, ny)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)])
    verts = (verts.reshape(-1, 3) * scale + shift).astype(np.float32)
    return verts, faces.astype(np.int64), (np.arange(nx * ny) % 3).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _meshes():
    """ten bent sheets of 12 .. 300 vertices around (0.5, 1.5, -1) with garment-like extents: every coordinate has a mean and a
    std well above 1e-3 of its largest magnitude"""
    return [_sheet(3 + g, 4 + 2 * g, 1.0 + 0.7 * g, np.asarray([0.4, 0.9, 0.3]) * (1 + 0.1 * g), np.asarray([0.5, 1.5, -1.0]))
            for g in range(10)]


MESH_INDEX = (3, 0, 9, 5, 5, 1, 7, 2, 8, 6, 4)              # every garment, one twice: 11 slots, chunks of 4, 4, 3
MESH_N, MESH_CHUNK = 600, 4


@pytest.mark.parametrize('noise', [0.0, 0.05])
def test_mesh_sampler_fit(gpe, noise):
    S = gpe.staging.MeshPointSampler
    index = torch.tensor(MESH_INDEX).cuda()
    s = S(_meshes(), None, mesh_samples=MESH_N, point_noise_w=noise, seed=SEED)
    state = s.state.clone()
    stats = s.fit_feature_stats(index, seed=SEED, chunk=MESH_CHUNK, install=False)
    assert torch.equal(s.state, state) and int(s.ticket) == 0 and s.f_shift is None and s.f_scale is None
    assert set(stats) == {'f_shift', 'f_scale'} and all(v.dtype == np.float32 and v.shape == (3,) for v in stats.values())
    # the clouds sample() returns for the same seed, chunks and no statistics (the sampler's own state is still (SEED, 0))
    clouds = np.concatenate([s.sample(index[g0:g0 + MESH_CHUNK])[0].cpu().numpy() for g0 in range(0, len(MESH_INDEX), MESH_CHUNK)])
    assert clouds.shape == (len(MESH_INDEX), MESH_N, 3)
    w = R.all_stats(clouds)
    assert (w['std'] >= 1e-3 * np.abs(clouds).max(axis=(0, 1))).all() and (np.abs(w['mean']) >= 1e-3 * np.abs(clouds).max(axis=(0, 1))).all()
    for k, key in (('f_shift', 'mean'), ('f_scale', 'std')):
        want = R.f32(w[key])
        assert (np.abs(stats[k].astype(np.float64) - want) <= R.ulp32(want)).all(), (k, stats[k], want)
    # the result is a function of (seed, chunk, index, data)
    again = S(_meshes(), None, mesh_samples=MESH_N, point_noise_w=noise, seed=1).fit_feature_stats(list(MESH_INDEX), seed=SEED, chunk=MESH_CHUNK)
    assert all(np.array_equal(_bits(again[k]), _bits(stats[k])) for k in stats)
    other = s.fit_feature_stats(index, seed=SEED, chunk=5, install=False)
    assert not np.array_equal(_bits(other['f_shift']), _bits(stats['f_shift']))

    # install: the same draws come back standardised.  y = fl((x - sh) / sc) with sh, sc within one fp32 ulp of the float64 mean and
    # std: the exact mean of (x - sh) / sc is (mean - sh) / sc, at most 2^-23 |mean| / sc, its std std / sc, within 2^-23 of 1, and
    # each y carries at most three roundings (the subtraction, a reciprocal, the product), 3 2^-24 max|y|, which moves the mean
    # and the std by no more than that; one more 2^-24 max|y| is allowed for the fp32 statistics themselves.
    s.reseed(SEED, 0)
    s.fit_feature_stats(index, seed=SEED, chunk=MESH_CHUNK)
    assert s.f_shift == [float(v) for v in stats['f_shift']] and s.f_scale == [float(v) for v in stats['f_scale']]
    assert torch.equal(s.state, state)
    y = np.concatenate([s.sample(index[g0:g0 + MESH_CHUNK])[0].cpu().numpy() for g0 in range(0, len(MESH_INDEX), MESH_CHUNK)])
    wy = R.all_stats(y)
    slack = 4 * 2.0 ** -24 * np.abs(y).max(axis=(0, 1))
    bar_mean = 2.0 ** -23 * np.abs(w['mean']) / w['std'] + slack
    bar_std = 2.0 ** -23 + slack
    print('standardised clouds: |mean| %s (bar %s), |std - 1| %s (bar %s)' % (np.abs(wy['mean']), bar_mean, np.abs(wy['std'] - 1), bar_std))
    assert (np.abs(wy['mean']) <= bar_mean).all() and (np.abs(wy['std'] - 1) <= bar_std).all()


def test_mesh_sampler_fit_reports_a_bad_garment_at_the_end(gpe):
    meshes = list(_meshes()[:3]) + [(np.zeros((3, 3), dtype=np.float32), np.asarray([[0, 1, 2]]), np.zeros(3, dtype=np.int64))]
    s = gpe.staging.MeshPointSampler(meshes, None, mesh_samples=64)
    with pytest.raises(ValueError, match='garment 4 of the index'):
        s.fit_feature_stats([0, 1, 2, 0, 3, 1], chunk=2)
    with pytest.raises(ValueError, match='garment 1 of the index'):
        s.fit_feature_stats([0, 7], chunk=2)
    assert s.f_shift is None
    assert s.fit_feature_stats([0, 1, 2], chunk=2)['f_scale'].min() > 0 and s.f_shift is not None


# ---- StitchPairSampler.fit_feature_stats -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _stitch_set():
    """the garment of tests/golden/stitch_sample_small.pt (its edges in stitch_pairs_small.pt, its stitches and settings in the
    sample fixture), tiled to five garments that differ by a power-of-two factor"""
    fx = torch.load(os.path.join(GOLDEN, 'stitch_sample_small.pt'), weights_only=False)
    pairs = torch.load(os.path.join(GOLDEN, fx['garment']), weights_only=False)
    edges, ne = pairs['edges'].numpy().astype(np.float32), pairs['num_edges'].numpy().astype(np.int64)
    G = 5
    e = np.stack([edges * np.float32(2.0 ** (g - 2)) for g in range(G)])
    gt = np.ascontiguousarray(fx['stitches'].numpy().T)[None].repeat(G, axis=0)
    return {'edges': e, 'num_edges': ne[None].repeat(G, axis=0), 'gt': gt, 'gt_num': np.full(G, gt.shape[2], dtype=np.int64),
            'n_st': int(fx['n_stitched']), 'n_non': int(fx['n_non_stitched'])}


def test_stitch_sampler_fit(gpe):
    gs = _stitch_set()
    dev = [torch.from_numpy(gs[k]).cuda() for k in ('edges', 'num_edges', 'gt', 'gt_num')]
    S = gpe.staging.StitchPairSampler
    index = torch.tensor([4, 0, 2, 2, 1, 3, 0]).cuda()
    s = S(*dev, None, gs['n_st'], gs['n_non'], seed=SEED)
    with pytest.raises(RuntimeError, match='without statistics'):
        s.sample(index[:2])
    state = s.state.clone()
    stats = s.fit_feature_stats(index, seed=SEED, chunk=3, install=False)
    assert torch.equal(s.state, state) and int(s.ticket) == 0 and s.f_shift is None
    C = 2 * gs['edges'].shape[3]
    assert all(v.dtype == np.float32 and v.shape == (C,) for v in stats.values()) and set(stats) == {'f_shift', 'f_scale'}
    # the rows a sampler with shift 0 / scale 1 returns for the same seed and chunks
    unit = S(*dev, {'f_shift': [0.0] * C, 'f_scale': [1.0] * C}, gs['n_st'], gs['n_non'], seed=SEED)
    rows = np.concatenate([unit.sample(index[g0:g0 + 3])[0].cpu().numpy() for g0 in range(0, 7, 3)])
    assert rows.shape == (7, gs['n_st'] + gs['n_non'], C) and (unit.status.cpu() >= 0).all()
    w = R.stitch_standardize(rows)
    for k in ('f_shift', 'f_scale'):
        assert np.array_equal(_bits(stats[k]), _bits(R.f32(w[k]))), (k, stats[k], w[k])
    s.fit_feature_stats(index, seed=SEED, chunk=3)
    assert s.f_shift == [float(v) for v in stats['f_shift']] and s.f_scale == [float(v) for v in stats['f_scale']]
    got, labels = s.sample(index[:3])
    assert got.shape == (3, gs['n_st'] + gs['n_non'], C) and torch.isfinite(got).all() and labels.sum().item() == 3 * gs['n_st']
    with pytest.raises(ValueError, match='garment 1 of the index'):
        s.fit_feature_stats([0, 5, 1], chunk=2)


# ---- fit_pattern_standardization ---------------------------------------------------------------------------------------------------

def test_pattern_standardization_against_the_reference(gpe):
    p = torch.load(os.path.join(GOLDEN, 'fit_stats_small.pt'), weights_only=False)['pattern']
    gt_host = {k: v.numpy() for k, v in p['gt'].items()}
    gt = {k: v.cuda() for k, v in p['gt'].items()}
    feats = p['features'].numpy()
    G, N = feats.shape[:2]
    acc = gpe.ops.FitAccumulator(3, G, N, 'cuda')
    acc.add(p['features'].cuda())
    r = acc.read()
    fstats = {'f_shift': r['mean'], 'f_scale': r['std']}
    stats = gpe.staging.fit_pattern_standardization(gt, fstats)
    keys = ('outlines', 'rotations', 'translations', 'stitch_tags')
    assert set(stats) == {'f_shift', 'f_scale', 'gt_shift', 'gt_scale'} and all(set(stats[s]) == set(keys) for s in ('gt_shift', 'gt_scale'))
    for side in ('gt_shift', 'gt_scale'):
        for k in keys:
            v = stats[side][k]
            assert isinstance(v, np.ndarray) and v.dtype == np.float32 and v.shape == (gt_host[k].shape[-1],), (side, k)
    assert stats['f_shift'].dtype == np.float32 and stats['f_shift'].shape == (3,)
    # the reference's own results, by the bars of tests/test_fit_stats_host.py
    for side, k, entry, bound in (('f_shift', None, p['f_shift'], R.sum_bound(feats)), ('f_scale', None, p['f_scale'], R.sum_bound(feats)),
                                  ('gt_shift', 'outlines', p['gt_shift']['outlines'], R.sum_bound(gt_host['outlines'], True)),
                                  ('gt_scale', 'outlines', p['gt_scale']['outlines'], R.sum_bound(gt_host['outlines'], True))):
        got = stats[side] if k is None else stats[side][k]
        d = np.abs(got.astype(np.float64) - entry['ref'].numpy().astype(np.float64))
        print('%s %s: |device - reference| %s, bound %s' % (side, k, d, bound))
        assert (d <= bound).all(), (side, k)
    assert stats['gt_shift']['outlines'][:2].tolist() == [0.0, 0.0]
    for k in keys[1:]:
        for side in ('gt_shift', 'gt_scale'):
            assert np.array_equal(_bits(stats[side][k]), _bits(p[side][k].numpy())), (side, k)
    # ... and the restatement, by the bars of this file
    w = R.pattern_standardize(feats, gt_host)
    for got, want in ((stats['f_shift'], w['f_shift']), (stats['f_scale'], w['f_scale']),
                      (stats['gt_shift']['outlines'][2:], w['gt_shift']['outlines'][2:]), (stats['gt_scale']['outlines'], w['gt_scale']['outlines'])):
        want = R.f32(want)
        assert (np.abs(got.astype(np.float64) - want) <= R.ulp32(want)).all(), (got, want)

    # the consumers take it as it is
    P, Lm = gt_host['outlines'].shape[1:3]
    cfg = {'max_panel_len': Lm, 'max_pattern_len': P, 'standardize': stats, 'mesh_samples': 64}
    std = lambda k: ((gt[k] - torch.from_numpy(stats['gt_shift'][k]).cuda()) / torch.from_numpy(stats['gt_scale'][k]).cuda()).contiguous()   # noqa: E731
    preds = {k: std(k) for k in keys}
    preds['free_edges_mask'] = torch.zeros(G, P, Lm, device='cuda')
    dec = gpe.ops.pattern_decode(preds, stats)
    # (include/gpe_hip.h gpe_pattern_decode: a row is kept unless all four values are within 1.5 of 0, three kept rows make a panel)
    kept = ((np.abs(gt_host['outlines']) > 1.5).any(axis=3).sum(axis=2) >= 3).sum(axis=1)
    assert dec['num_panels'].cpu().tolist() == kept.tolist() and kept.min() >= 1
    loss = gpe.metrics.ComposedPatternLoss(cfg, {'loss_components': ['shape', 'loop', 'rotation', 'translation'], 'quality_components': [],
                                                 'panel_order_inariant_loss': False, 'panel_origin_invariant_loss': False})
    num_edges = torch.from_numpy((np.abs(gt_host['outlines']) > 1e-5).any(axis=3).sum(axis=2)).cuda()
    with torch.no_grad():
        full, parts, _ = loss({k: preds[k] for k in keys[:3]}, {**{k: preds[k].clone() for k in keys[:3]}, 'num_edges': num_edges}, epoch=0)
    assert torch.isfinite(full).item() and all(torch.isfinite(torch.as_tensor(v)).all() for v in parts.values())
    s = gpe.staging.MeshPointSampler.from_config(_meshes()[:2], cfg)
    assert s.f_shift == [float(v) for v in stats['f_shift']] and s.mesh_samples == 64

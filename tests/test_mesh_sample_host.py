"""not-gpu: the host restatement of the mesh point sampler (tests/mesh_sample_restate.py, the yardstick of
tests/test_gpu_mesh_sample.py) against the analytic distribution — faces in proportion to their areas, points uniform in the
triangle, standard normal and independent noise — its nearest-vertex pass against scipy's cKDTree in float64, the re-label rule and
the status paths; ops.mesh_resident's thresholds against the restatement's; and the argument checks of gpe_mesh_points_sample /
ops.mesh_points_sample / staging.MeshPointSampler, which need no GPU.

The statistical bars are the 0.9999 chi-square quantiles (Wilson-Hilferty, tests/stitch_sample_restate.py).  Seed, draw and slot
are 0 everywhere and both sides are deterministic, so a test either always passes or always fails."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mesh_sample_restate as R

DRAWS = 20000


def face_areas(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    return 0.5 * np.linalg.norm(np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]), axis=1)


def chi2(counts, expected):
    counts, expected = np.asarray(counts, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    return float(((counts - expected) ** 2 / expected).sum())


@pytest.fixture(scope='module')
def twelve():
    verts, faces, labels = R.twelve_faces()
    d = R.draw(verts, faces, R.thresholds(verts, faces), 0, DRAWS, 0, 0)
    return verts, faces, labels, d


THRESHOLD_CASES = {
    'leading': [[0, 0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 4]],
    'inner': [[0, 1, 2], [1, 1, 3], [3, 3, 3], [1, 2, 3], [2, 3, 4]],
    'trailing': [[0, 1, 2], [1, 2, 3], [2, 3, 4], [4, 4, 0], [2, 2, 2]],
    'one face': [[0, 1, 2]],
    'all degenerate': [[0, 0, 1], [2, 2, 2]],
}


@pytest.mark.parametrize('case', sorted(THRESHOLD_CASES))
def test_thresholds_of_the_resident_set_equal_the_restatement(case):
    import gpe_amd
    verts = np.random.RandomState(0).randn(5, 3).astype(np.float32)
    faces = np.asarray(THRESHOLD_CASES[case], dtype=np.int64)
    want = R.thresholds(verts, faces)
    other = (verts[::-1].copy(), np.asarray([[0, 1, 2], [2, 3, 4]]), np.zeros(5, dtype=np.int64))
    res = gpe_amd.ops.mesh_resident([other, (verts, faces, np.arange(5) - 1), other], device='cpu')
    assert res.face_off.tolist() == [0, 2, 2 + len(faces), 4 + len(faces)] and res.vert_off.tolist() == [0, 5, 10, 15]
    got = res.face_cdf.numpy().view(np.uint32)[2:2 + len(faces)]
    assert got.tolist() == want.tolist()
    assert res.vert_label.tolist()[5:10] == [-1, 0, 1, 2, 3] and res.has_unlabelled
    assert np.array_equal(res.verts.numpy()[5:10], verts) and np.array_equal(res.faces.numpy()[2:2 + len(faces)], faces)
    area = face_areas(verts, faces)
    if case == 'all degenerate':
        assert want.tolist() == [0, 0]
        return
    last = int(np.nonzero(area > 0)[0][-1])
    assert (want[last:] == 1 << 31).all() and (want[:last] < 1 << 31).all() and (np.diff(want.astype(np.int64)) >= 0).all()
    prev = np.concatenate([[0], want[:-1].astype(np.int64)])
    for f in np.nonzero(area == 0)[0]:
        assert f > last or want[f] == prev[f], f                       # no w with prev <= w < T[f]: never drawn
    # the first face with T[f] > w, at both ends of the range and at every step
    T = want.astype(np.int64)
    for w in [0, (1 << 31) - 1] + [int(t) for t in T[:last]] + [int(t) - 1 for t in T[:last] if t > 0]:
        f = int(np.searchsorted(T, w, side='right'))
        assert area[f] > 0 and T[f] > w and (f == 0 or T[f - 1] <= w)


def test_face_counts_follow_the_area_shares(twelve):
    verts, faces, _, d = twelve
    area = face_areas(verts, faces)
    assert area[7] == 0 and area[area > 0].max() / area[area > 0].min() == pytest.approx(50.0, rel=1e-5)
    counts = np.bincount(d['face'], minlength=12)
    assert counts.sum() == DRAWS and counts[7] == 0
    pos = area > 0
    x = chi2(counts[pos], DRAWS * area[pos] / area.sum())
    print('face counts %s, chi-square %.2f (10 degrees of freedom, bar %.2f)' % (counts.tolist(), x, R.chi2_quantile(10, 0.9999)))
    assert x < R.chi2_quantile(10, 0.9999)


def test_barycentric_coordinates_are_uniform_and_exact(twelve):
    d = twelve[3]
    bary = d['bary']
    assert bary.dtype == np.float32 and (bary >= 0).all()
    assert ((bary[:, 0] + bary[:, 1]) + bary[:, 2] == np.float32(1)).all()
    assert (d['iu'] >= 0).all() and (d['iv'] >= 0).all() and (d['iu'] + d['iv'] <= R.ONE).all()
    # the 16 congruent triangles of two midpoint subdivisions: cell (i, j) of the quarter grid in (b1, b2), lower or upper half
    q = R.ONE // 4
    i, j = np.minimum(d['iu'] // q, 3), np.minimum(d['iv'] // q, 3)
    upper = (d['iu'] - i * q) + (d['iv'] - j * q) >= q
    ids = {}
    for a in range(4):
        for b in range(4 - a):
            ids[(a, b, False)] = len(ids)
            if a + b < 3:
                ids[(a, b, True)] = len(ids)
    assert len(ids) == 16
    cell = np.asarray([ids.get((int(a), int(b), bool(u)), ids.get((int(a), int(b), False), -1)) for a, b, u in zip(i, j, upper)])
    assert (cell >= 0).all()
    counts = np.bincount(cell, minlength=16)
    x = chi2(counts, np.full(16, DRAWS / 16.0))
    print('sub-triangle counts %s, chi-square %.2f (15 degrees of freedom, bar %.2f)' % (counts.tolist(), x, R.chi2_quantile(15, 0.9999)))
    assert x < R.chi2_quantile(15, 0.9999)
    # the points are what the coordinates say, in float64 up to the three roundings of the float32 sum
    verts, faces = twelve[0].astype(np.float64), twelve[1]
    f = d['face']
    exact = (bary[:, :1].astype(np.float64) * verts[faces[f, 0]] + bary[:, 1:2].astype(np.float64) * verts[faces[f, 1]]
             + bary[:, 2:].astype(np.float64) * verts[faces[f, 2]])
    assert np.abs(d['points'] - exact).max() <= 3 * 2.0 ** -24 * np.abs(verts).max()


def test_noise_is_standard_normal_and_independent():
    z = R.normals(0, DRAWS, 0, 0)
    assert z.dtype == np.float64 and z.shape == (DRAWS, 3) and np.isfinite(z).all()
    assert np.abs(z).max() <= math.sqrt(2 * 24 * math.log(2)) + 1e-12            # u1 >= 2^-24: |z| <= 5.77
    u = 0.5 * (1.0 + np.vectorize(math.erf)(z / math.sqrt(2.0)))
    for axis in range(3):
        counts = np.bincount(np.minimum((u[:, axis] * 16).astype(int), 15), minlength=16)
        x = chi2(counts, np.full(16, DRAWS / 16.0))
        print('axis %d: bin counts %s, chi-square %.2f (15 degrees of freedom, bar %.2f)' % (axis, counts.tolist(), x, R.chi2_quantile(15, 0.9999)))
        assert x < R.chi2_quantile(15, 0.9999), axis
    q = np.minimum((u * 4).astype(int), 3)
    counts = np.bincount(q[:, 0] * 16 + q[:, 1] * 4 + q[:, 2], minlength=64)
    x = chi2(counts, np.full(64, DRAWS / 64.0))
    print('4 x 4 x 4 table: chi-square %.2f (63 degrees of freedom, bar %.2f)' % (x, R.chi2_quantile(63, 0.9999)))
    assert x < R.chi2_quantile(63, 0.9999)
    # the two kinds and two slots of one (seed, draw) are different streams
    assert not np.array_equal(R.words(R.FACE, np.arange(4), 0, 0, 0), R.words(R.NOISE, np.arange(4), 0, 0, 0))
    assert not np.array_equal(R.normals(0, 8, 0, 0), R.normals(1, 8, 0, 0))


def test_nearest_vertex_against_a_kd_tree_and_the_tie_rule():
    from scipy.spatial import cKDTree
    rng = np.random.RandomState(0)
    verts = rng.uniform(-1, 1, (700, 3)).astype(np.float32)
    points = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    dist, idx = cKDTree(verts.astype(np.float64)).query(points.astype(np.float64), k=2)
    clear = dist[:, 1] - dist[:, 0] > 1e-5                                         # float32 cannot turn these round
    assert clear.sum() > 450
    assert np.array_equal(R.snap(points, verts)[clear], idx[clear, 0])
    # constructed ties: a midpoint, a repeated vertex, and both at once; the lower index wins whatever the order
    tie = np.asarray([[2, 0, 0], [0, 0, 0], [0, 0, 0], [0, 2, 0], [2, 0, 0]], dtype=np.float32)
    p = np.asarray([[1, 0, 0], [0, 0.25, 0], [0, 1, 0], [1.75, 0, 0]], dtype=np.float32)
    assert R.snap(p, tie).tolist() == [0, 1, 1, 0]
    assert R.snap(p, tie[::-1]).tolist() == [0, 2, 1, 0]
    d = R.distances(p, tie)
    assert d.dtype == np.float32 and d[0, 0] == d[0, 1] == d[0, 2] == d[0, 4] == 1


def test_relabel_rule():
    pts = np.asarray([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [10, 0, 0]], dtype=np.float32)
    out, fell = R.relabel(pts, [5, -1, 7, -1, -1])
    assert out.tolist() == [5, 5, 7, 7, 7] and fell == 0                           # point 1 is as far from 0 as from 2: 0 wins
    out, fell = R.relabel(pts, [-1, -1, 7, -1, 4])
    assert out.tolist() == [7, 7, 7, 7, 4] and fell == 0                           # an unlabelled neighbour is no candidate
    out, fell = R.relabel(pts, [-1] * 5)
    assert out.tolist() == [0] * 5 and fell == 5
    out, fell = R.relabel(pts, [3, 2, 1, 0, 0])
    assert out.tolist() == [3, 2, 1, 0, 0] and fell == 0


def test_status_paths_of_the_restatement(twelve):
    verts, faces, labels, _ = twelve
    flat = (verts, np.asarray([[0, 0, 1], [3, 3, 3]]), labels)
    bare = (verts, faces, np.full(len(verts), -1))
    feats, seg, status, dec = R.sample_batch([(verts, faces, labels), flat, bare], [0, 1, 2, 3, -1, 0], 64, 0, 0)
    assert status.tolist() == [0, -1, 64, -2, -2, 0]
    for b in (1, 3, 4):
        assert not feats[b].any() and not seg[b].any() and dec[b] is None
    assert not seg[2].any() and feats[2].any()
    assert not np.array_equal(feats[0], feats[5])                                  # one garment in two slots: two draws
    assert np.array_equal(seg[0], dec[0]['face'])                                  # the label of this mesh is the face
    sh, sc = [0.5, -0.25, 0.125], [2.0, 3.0, 0.7]
    std = R.sample_batch([(verts, faces, labels)], [0], 64, 0, 0, shift=sh, scale=sc)[0]
    assert np.array_equal(std[0], (feats[0] - np.float32(sh)) / np.float32(sc)) and std.dtype == np.float32


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    from gpe_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    good = dict(verts=p, faces=p, voff=p, foff=p, cdf=p, G=1, index=p, B=1, N=8, w=0.0, sh=p, sc=p, relabel=1, ws=p, state=p, ticket=p,
                feats=p, seg=p, status=p)

    def call(**kw):
        a = dict(good, **kw)
        return l.gpe_mesh_points_sample(a['verts'], a['faces'], a['voff'], a['foff'], a['cdf'], a['G'], a['index'], a['B'], a['N'],
                                        a['w'], a['sh'], a['sc'], a['relabel'], a['ws'], a['state'], a['ticket'], a['feats'], a['seg'],
                                        a['status'], None)
    for name in ('verts', 'faces', 'voff', 'foff', 'cdf', 'index', 'state', 'ticket', 'feats', 'seg', 'status', 'ws', 'sh', 'sc'):
        assert call(**{name: None}) == -22, name
    assert call(B=0) == -22 and call(B=-1) == -22 and call(B=1 << 24) == -22
    assert call(N=0) == -22 and call(N=-5) == -22 and call(N=1 << 28) == -22
    assert call(G=0) == -22 and call(G=-1) == -22
    assert call(verts=p + 4) == -22 and call(ws=p + 8) == -22 and call(state=p + 4) == -22
    assert call(B=(1 << 24) - 1, N=(1 << 28) - 1) == -22                           # the grid would not fit


def test_op_has_no_cpu_path_and_checks_its_arguments(twelve):
    import gpe_amd
    ops, staging = gpe_amd.ops, gpe_amd.staging
    verts, faces, labels, _ = twelve
    mesh = (verts, faces, labels)
    for bad in ([], [(verts, faces)], [(verts[:, :2], faces, labels)], [(verts, faces.astype(np.float32), labels)],
                [(verts, faces, labels[:-1])], [(verts, faces, labels.astype(np.float32))], [(verts.astype(np.int64), faces, labels)]):
        with pytest.raises(ValueError):
            ops.mesh_resident(bad, device='cpu')
    for f in (len(verts), -1):                                                     # a face outside the garment's vertices
        broken = faces.copy()
        broken[5, 1] = f
        with pytest.raises(ValueError, match='outside 0'):
            ops.mesh_resident([mesh, (verts, broken, labels)], device='cpu')
    with pytest.raises(ValueError, match='-1'):
        ops.mesh_resident([(verts, faces, labels - 2)], device='cpu')
    nan = verts.copy()
    nan[3, 1] = np.nan
    with pytest.raises(ValueError, match='finite'):
        ops.mesh_resident([(nan, faces, labels)], device='cpu')
    res = ops.mesh_resident([(torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(labels))], device='cpu')
    assert ops.mesh_resident(res) is res and not res.has_unlabelled and res.G == 1
    index, state, ticket = torch.tensor([0, 0]), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.mesh_points_sample(res, index, 16, state, ticket)
    with pytest.raises(RuntimeError, match='no CPU path'):
        staging.MeshPointSampler(res)
    for kw in (dict(resident=mesh), dict(mesh_samples=0), dict(mesh_samples=1 << 28), dict(index=index.float()), dict(index=index[:0]),
               dict(index=index.view(1, 2)), dict(state=state.int()), dict(state=state[:1]), dict(ticket=ticket.long()),
               dict(f_shift=[0.0] * 3), dict(f_shift=[0.0] * 2, f_scale=[1.0] * 2)):
        a = dict(dict(resident=res, index=index, mesh_samples=16, state=state, ticket=ticket), **kw)
        with pytest.raises(ValueError):                                            # before the device check
            ops.mesh_points_sample(**a)

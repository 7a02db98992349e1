"""not-gpu: the host restatement of the scan sampler (tests/scan_sample_restate.py, the yardstick of tests/test_gpu_scan_sample.py) —
its distribution against np.random.permutation(n)[:N], its structure — and what include/gpe_hip_scan.h promises without a GPU: the
header binds through _lib.SCAN_HEADERS, the symbols are exported, the host-only workspace size, -22 on every documented bad
argument; then the host builders of ops (cloud_resident) and staging (ScanSampler, load_scan_points).

The statistical bars are derived, not fitted: a point of a cloud of n is among the N drawn with probability p = N / n and is row 0
with probability 1 / n, independently from draw to draw, so over D draws each count is Binomial(D, p) with sigma = sqrt(D p (1 - p)).
With 2 x 24 counts, a 5 sigma bar is crossed by a sound sampler with probability < 1e-4.  Both sides are deterministic (seed 7, draws
0 .. D - 1; RandomState(601)), so the test either always passes or always fails."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scan_sample_restate as R

SEED = 7


def _deviations(draws, n, N):
    """draws int [D, N] -> (largest inclusion deviation, largest row-0 deviation), in sigmas"""
    D = len(draws)
    out = []
    for counts, p in ((np.bincount(draws.ravel(), minlength=n), N / n), (np.bincount(draws[:, 0], minlength=n), 1 / n)):
        sigma = np.sqrt(D * p * (1 - p))
        out.append(float(np.abs(counts - D * p).max() / sigma))
    return out


def test_distribution_matches_a_uniform_permutation_prefix():
    n, N, D = 24, 8, 4096
    rs = np.random.RandomState(601)
    ref = np.stack([rs.permutation(n)[:N] for _ in range(D)])
    got = np.stack([R.picked_of(n, N, 0, SEED, d)[0] for d in range(D)])
    dev_ref, dev_got = _deviations(ref, n, N), _deviations(got, n, N)
    print('numpy: inclusion %.1f sigma, row 0 %.1f sigma; Philox-key ranking: inclusion %.1f sigma, row 0 %.1f sigma'
          % tuple(dev_ref + dev_got))
    assert max(dev_ref) <= 5 and max(dev_got) <= 5
    assert len({tuple(r) for r in got}) > D - 4                                      # the draws differ from each other


@pytest.mark.parametrize('n, N', [(1, 8), (3, 8), (7, 8), (8, 8), (9, 8), (24, 8), (100, 64), (5, 64)])
def test_structure(n, N):
    for draw in range(6):
        for b in (0, 3):
            picked, status = R.picked_of(n, N, b, SEED, draw)
            assert picked.shape == (N,) and picked.min() >= 0 and picked.max() < n
            counts = np.bincount(picked, minlength=n)
            if n >= N:
                assert status == 0 and counts.max() == 1 and counts.sum() == N       # N distinct points
            else:
                assert status == N - n and set(counts.tolist()) <= {N // n, -(-N // n)}
                assert np.array_equal(picked, picked[np.arange(N) % n])             # whole permutations repeat
    assert not np.array_equal(R.picked_of(24, 8, 0, SEED, 0)[0], R.picked_of(24, 8, 1, SEED, 0)[0])     # the slot is in the key
    assert R.picked_of(0, 4, 0, SEED, 0)[1] == -1 and (R.picked_of(0, 4, 0, SEED, 0)[0] == -1).all()


def test_restated_batch_and_labels():
    rs = np.random.RandomState(5)
    clouds = [rs.uniform(-1, 1, (n, 3)).astype(np.float32) for n in (0, 5, 40)]
    shift, scale = [0.1, -0.2, 0.3], [0.5, 2.0, 1.5]
    feats, picked, status = R.sample_batch(clouds, [2, 1, 0, 3, -1, 2], 8, SEED, 1, shift, scale)
    assert status.tolist() == [0, 3, -1, -2, -2, 0]
    assert not feats[2:5].any() and (picked[2:5] == -1).all()
    want = (clouds[2][picked[0]] - np.float32(shift)) / np.float32(scale)
    assert np.array_equal(feats[0], want.astype(np.float32)) and not np.array_equal(picked[0], picked[5])
    # a point that was drawn is its own nearest row (the lower one when the row repeats), and takes that row's first maximum
    att = rs.uniform(0, 1, (6, 8, 4)).astype(np.float32)
    att[1, :, 1] = att[1, :, 2] = 2.0                                                # tied maxima: the first wins
    lab = R.labels(clouds, [2, 1, 0, 3, -1, 2], picked, att)
    assert lab.shape == (45,) and (lab[:5] == 1).all()
    for r, i in enumerate(picked[5]):
        assert lab[5 + i] == np.argmax(att[5, r])                                    # slot 5 stands, not slot 0
    assert np.array_equal(R.nearest_rows(np.float32([[0, 0, 0]]), np.float32([[1, 0, 0], [-1, 0, 0], [0, 0.5, 0], [0, -0.5, 0]])), [2])


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------------

def test_scan_header_binds():
    from gpe_amd import _lib
    assert _lib.SCAN_HEADERS == (_lib.SCAN_HEADER_PATH,) and os.path.basename(_lib.SCAN_HEADER_PATH) == 'gpe_hip_scan.h'
    sigs = _lib.parse_header(_lib.SCAN_HEADER_PATH)
    assert sigs == {'gpe_scan_sample_ws_bytes': ('l', ['l', 'i', 'l']),
                    'gpe_scan_sample': ('i', ['p', 'p', 'i', 'l', 'p', 'i', 'i', 'p', 'p', 'i', 'p', 'l'] + ['p'] * 6),
                    'gpe_scan_labels': ('i', ['p', 'p', 'i', 'l', 'p', 'i', 'i', 'p', 'p', 'i', 'p', 'p'])}
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in sigs:
        assert hasattr(raw, name), 'libgpe_hip.so does not export %s' % name
    for h in (_lib.HEADERS + _lib.FEATURE_HEADERS + _lib.EVAL_HEADERS + _lib.PLACE_HEADERS + _lib.FRAMEWORK_HEADERS
              + _lib.FEED_HEADERS):
        assert not set(sigs) & set(_lib.parse_header(h))                              # declared once
    l = _lib.lib()
    assert l.gpe_scan_sample.argtypes[3] is ctypes.c_long and l.gpe_scan_sample_ws_bytes.restype is ctypes.c_long
    assert l.gpe_abi_version() == 7
    common = open(os.path.join(os.path.dirname(_lib.LIB_PATH), 'csrc', 'gpe_common.h')).read()
    assert 'include/gpe_hip_scan.h"' in common                                        # every definition is checked against it


def test_workspace_size():
    from gpe_amd import _lib
    l = _lib.lib()
    ws = l.gpe_scan_sample_ws_bytes
    assert ws(1, 1, 1) >= 16 + 4 + 2048 * 4 and ws(1, 1, 1) % 16 == 0
    for N in (1, 64, 2000, 2048):
        sizes = [ws(B, N, 200000) for B in (1, 2, 3, 32, 33, 1000)]
        assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes                   # monotone in B
        assert all(ws(32, N, a) <= ws(32, N, b) for a, b in zip((1, 1000, 200000), (1000, 200000, (1 << 28) - 1)))   # ... and n_max
    assert ws((1 << 24) - 1, 2048, (1 << 28) - 1) > 0
    for B, N, n in ((0, 64, 10), (-1, 64, 10), (1 << 24, 64, 10), (4, 0, 10), (4, 2049, 10), (4, 64, 0), (4, 64, 1 << 28)):
        assert ws(B, N, n) == -22, (B, N, n)


def test_compute_entries_reject_bad_arguments_without_a_gpu():
    from gpe_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 15) & ~15
    stats = (ctypes.c_float * 3)(1, 1, 1)
    need = l.gpe_scan_sample_ws_bytes(2, 64, 100)
    good = dict(points4=p, off=p, G=3, n_max=100, index=p, B=2, N=64, shift=stats, scale=stats, narrow=0, ws=p, ws_bytes=need, state=p,
                ticket=p, features=p, picked=p, status=p)

    def sample(**kw):
        a = dict(good, **kw)
        return l.gpe_scan_sample(a['points4'], a['off'], a['G'], a['n_max'], a['index'], a['B'], a['N'], a['shift'], a['scale'],
                                 a['narrow'], a['ws'], a['ws_bytes'], a['state'], a['ticket'], a['features'], a['picked'], a['status'],
                                 None)
    for name in ('points4', 'off', 'index', 'ws', 'state', 'ticket', 'features', 'picked', 'status', 'shift', 'scale'):
        assert sample(**{name: None}) == -22, name
    assert sample(points4=p + 4) == -22 and sample(ws=p + 8) == -22 and sample(state=p + 4) == -22
    assert sample(G=0) == -22 and sample(B=0) == -22 and sample(B=1 << 24) == -22
    assert sample(N=0) == -22 and sample(N=2049) == -22 and sample(n_max=0) == -22 and sample(n_max=1 << 28) == -22
    assert sample(narrow=-1) == -22 and sample(ws_bytes=need - 1) == -22

    goodl = dict(points4=p, off=p, G=3, n_max=100, index=p, B=2, N=64, picked=p, att=p, P=5, labels=p)

    def labels(**kw):
        a = dict(goodl, **kw)
        return l.gpe_scan_labels(a['points4'], a['off'], a['G'], a['n_max'], a['index'], a['B'], a['N'], a['picked'], a['att'], a['P'],
                                 a['labels'], None)
    for name in ('points4', 'off', 'index', 'picked', 'att', 'labels'):
        assert labels(**{name: None}) == -22, name
    assert labels(points4=p + 4) == -22
    assert labels(G=0) == -22 and labels(B=0) == -22 and labels(B=1 << 24) == -22 and labels(N=0) == -22 and labels(N=1 << 28) == -22
    assert labels(P=0) == -22 and labels(P=4097) == -22 and labels(n_max=0) == -22 and labels(n_max=1 << 28) == -22


# ---- the host builders ---------------------------------------------------------------------------------------------------------------

def test_cloud_resident():
    from gpe_amd import ops, ops_scan
    rs = np.random.RandomState(1)
    clouds = [rs.uniform(-1, 1, (5, 3)), np.zeros((0, 3)), torch.from_numpy(rs.uniform(-1, 1, (7, 3)).astype(np.float32))]
    r = ops.cloud_resident(clouds, device='cpu')
    assert isinstance(r, ops.CloudResident) and ops.cloud_resident(r) is r
    assert (r.G, r.T, r.sizes, r.n_max) == (3, 12, (5, 0, 7), 7)                      # the empty cloud is kept; the sizes stay on the host
    assert r.off.dtype == torch.int32 and r.off.tolist() == [0, 5, 5, 12]
    assert r.points4.dtype == torch.float32 and r.points4.shape[1] == 4 and not r.points4[:, 3].any()
    assert np.array_equal(r.points[:5].numpy(), clouds[0].astype(np.float32)) and torch.equal(r.points[5:12], clouds[2])
    bad = rs.uniform(-1, 1, (4, 3))
    bad[2, 1] = np.nan
    for wrong in ([bad], [np.where(np.isnan(bad), np.inf, bad)], [np.zeros((4, 2))], [np.zeros(6)], [np.zeros((2, 3, 1))], []):
        with pytest.raises(ValueError):
            ops.cloud_resident(wrong, device='cpu')
    e = ops.cloud_resident([np.zeros((0, 3))], device='cpu')
    assert (e.G, e.T, e.n_max) == (1, 0, 1)
    for name in ('CloudResident', 'cloud_resident', 'cloud_points_buffers', 'cloud_points_sample', 'cloud_labels'):
        assert getattr(ops, name) is getattr(ops_scan, name) and name in ops_scan.__all__


def test_no_cpu_path():
    from gpe_amd import ops, staging
    r = ops.cloud_resident([np.zeros((5, 3))], device='cpu')
    with pytest.raises(RuntimeError, match='no CPU path'):
        staging.ScanSampler(r)
    state, ticket = torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.cloud_points_sample(r, torch.zeros(1, dtype=torch.int32), 4, state, ticket)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.cloud_labels(r, torch.zeros(1, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, 3))
    with pytest.raises(ValueError):
        ops.cloud_points_sample([np.zeros((5, 3))], torch.zeros(1, dtype=torch.int32), 4, state, ticket)


def test_load_scan_points(tmp_path):
    from gpe_amd import staging
    path = tmp_path / 'scan.txt'
    path.write_text('0.5 -1.25 3 0.75\n1e-3 2 -7.5 0.1\n\n  4 5 6 7 8\n')
    pts = staging.load_scan_points(str(path))
    assert pts.dtype == np.float64 and np.array_equal(pts, [[0.5, -1.25, 3], [1e-3, 2, -7.5], [4, 5, 6]])
    (tmp_path / 'short.txt').write_text('1 2 3\n4 5\n')
    with pytest.raises(ValueError):
        staging.load_scan_points(str(tmp_path / 'short.txt'))
    (tmp_path / 'empty.txt').write_text('')
    assert staging.load_scan_points(str(tmp_path / 'empty.txt')).shape == (0, 3)

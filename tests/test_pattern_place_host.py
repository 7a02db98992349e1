"""not-gpu: the panels of a decoded prediction placed in 3D (include/gpe_hip_place.h, ops.pattern_place,
patterns.DecodedPatterns.place) as far as it goes without a device:
  (1) the restatement (tests/pattern_place_restate.py) against the reference's own results (tests/golden/pattern_place_small.pt,
      scripts/make_pattern_place_golden.py): translation, vertices in 3D and rotation matrices within 1e-9 absolute, the fp32 edge rows
      within 1 ulp of the reference's all_edge_pairs rows, the midpoint chosen exactly;
  (2) the round trip: R . (mid, 0) + translation gives back the universal translation within 1e-9;
  (3) the tie order of the midpoints on a constructed exact tie;
  (4) gpe_hip_place.h parses, its one declaration is exported and bound through _lib.PLACE_HEADERS, the ABI version is 7, the older
      tuples are what they were, and off-menu arguments return -22 before a pointer is touched;
  (5) the Python argument checks that need no device.

The tolerances are derived, not measured: the fp64 chain from the decoded numbers to a 3D coordinate is about 50 operations on
magnitudes <= 1e3, so two correct evaluations differ by <~ 1e-12 — far below 1e-9 and far below half an fp32 ulp (>= 6e-8 relative), so
the fp32 rows differ from the reference's by at most one ulp, and only where the fp64 value straddles a rounding boundary.
No panel is skipped: the fixture's inputs keep a margin >= 1e-3 at every panel's one decision (asserted here and by the script)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from gpe_amd import _lib, ops, patterns
import pattern_decode_restate as D
import pattern_place_restate as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'pattern_place_small.pt')


@pytest.fixture(scope='module')
def fx():
    f = torch.load(FIXTURE, weights_only=False)
    decoded = D.restate(f['preds'], f['data_config']['standardize'], False)[0]
    placed, margins = R.restate(decoded)
    return f, decoded, placed, margins


def ordered(a):
    """fp32 -> integers in the order of the values: |difference| is the distance in ulps"""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def pair_rows(edges3d, num_edges):
    """all_edge_pairs' rows (nn/data/pattern_converter.py:471-484) from one garment's edges3d [P, L, 8]: panels i < j in order,
    row-major over (edge of i, edge of j)"""
    slots = [p for p in range(len(num_edges)) if num_edges[p] > 0]
    out = []
    for a, i in enumerate(slots):
        for j in slots[a + 1:]:
            ei, ej = edges3d[i, :num_edges[i]], edges3d[j, :num_edges[j]]
            out.append(np.concatenate([np.repeat(ei, len(ej), 0), np.tile(ej, (len(ei), 1))], 1))
    return np.concatenate(out)


def test_the_fixture_is_what_the_script_promises(fx):
    f, decoded, placed, margins = fx
    B, P = decoded['num_edges'].shape
    assert (B, P, decoded['curved'].shape[2]) == (6, 23, 14)
    real = decoded['num_edges'] > 0
    assert np.array_equal(np.isfinite(margins), real) and margins[real].min() >= 1e-3
    assert torch.equal(f['margins'], torch.from_numpy(margins))
    assert set(placed['top_mid'][real].tolist()) == {0, 1, 2, 3} and (placed['top_mid'][~real] == -1).all()
    assert os.path.getsize(FIXTURE) < 512 * 1024


def test_restatement_against_the_reference(fx):
    f, decoded, placed, _ = fx
    B, P = decoded['num_edges'].shape
    assert not placed['place_flags'].any()
    for b, g in enumerate(f['garments']):
        ne, nv = decoded['num_edges'][b], decoded['num_verts'][b]
        slots = [p for p in range(P) if ne[p] > 0]
        assert g['pattern']['panel_order'] == ['panel_%d' % p for p in slots]
        for p in slots:
            name = 'panel_%d' % p
            panel, rows = g['pattern']['panels'][name], g['edge_rows'][name]
            n = int(ne[p])
            assert rows.shape == (n, 8) and placed['top_mid'][b, p] == g['top_mid'][name]
            assert np.abs(placed['translation'][b, p] - np.asarray(panel['translation'])).max() <= 1e-9
            assert np.abs(placed['rot_matrix'][b, p] - g['rot_matrix'][name]).max() <= 1e-9
            # the reference's vertices in 3D are the end points of its fp64 edge rows
            v3 = placed['vertices3d'][b, p]
            ends = [k + 1 if k + 1 < nv[p] else 0 for k in range(n)]
            assert np.abs(v3[:n] - rows[:, 0:3]).max() <= 1e-9 and np.abs(v3[ends] - rows[:, 3:6]).max() <= 1e-9
            assert (v3[nv[p]:] == 0).all() and (placed['edges3d'][b, p, n:] == 0).all()
            # the curvature is taken or dropped, never computed
            assert np.array_equal(placed['edges3d'][b, p, :n, 6:8], rows[:, 6:8].astype(np.float32))
        want = g['pair_rows'].numpy()
        got = pair_rows(placed['edges3d'][b], ne)
        assert got.shape == want.shape and got.dtype == want.dtype == np.float32
        assert np.abs(ordered(got) - ordered(want)).max() <= 1


def test_round_trip_to_the_universal_translation(fx):
    _, decoded, placed, _ = fx
    B, P = decoded['num_edges'].shape
    for b in range(B):
        for p in range(P):
            nv = decoded['num_verts'][b, p]
            if decoded['num_edges'][b, p] == 0:
                continue
            mid = R.side_midpoints(decoded['vertices'][b, p, :nv])[placed['top_mid'][b, p]]
            back = placed['rot_matrix'][b, p] @ np.array([mid[0], mid[1], 0.0]) + placed['translation'][b, p]
            assert np.abs(back - decoded['translations'][b, p]).max() <= 1e-9
            # a rotation: orthonormal, determinant + 1
            Rm = placed['rot_matrix'][b, p]
            assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rm) - 1.0) <= 1e-12


def _square(quat, n_panels=1):
    """a 20 x 10 rectangle from (0, 0): every side midpoint and every product below is exact in fp64"""
    verts = np.zeros((1, n_panels, 5, 2))
    verts[0, :, :4] = [[0, 0], [20, 0], [20, 10], [0, 10]]
    rot = np.tile(np.asarray(quat, np.float64), (1, n_panels, 1))
    return {'num_edges': np.full((1, n_panels), 4, np.int32), 'num_verts': np.full((1, n_panels), 4, np.int32), 'vertices': verts,
            'curvature': np.zeros((1, n_panels, 4, 2)), 'curved': np.zeros((1, n_panels, 4), np.int32), 'rotations': rot,
            'translations': np.zeros((1, n_panels, 3))}


def test_tie_order_on_exact_ties():
    """`first strict maximum` in the order top, bottom, right, left.  The rule itself on small integers (any 2 x 2 block serves as
    R[1][0:2]: the rule reads nothing else), then ties that a rotation can produce exactly."""
    rect = _square([0, 0, 0, 1])['vertices'][0, 0, :4]              # midpoints: top (10, 10), bottom (10, 0), right (20, 5), left (0, 5)
    row = lambda a, b: np.array([[0.0, 0, 0], [a, b, 0], [0, 0, 0]])     # noqa: E731
    for (a, b), heights, first in (((1, 2), [30, 10, 30, 10], 0),         # top = right: top
                                   ((-1, -2), [-30, -10, -30, -10], 1),   # bottom = left: bottom
                                   ((1, -2), [-10, 10, 10, -10], 1),      # bottom = right: bottom
                                   ((-1, 2), [10, -10, -10, 10], 0),      # top = left: top
                                   ((0, 0), [0, 0, 0, 0], 0),             # all four: top
                                   ((2, 0), [20, 20, 40, 0], 2),          # no tie at the top: right
                                   ((-2, 0), [-20, -20, -40, 0], 3)):     # left
        mids = R.side_midpoints(rect)
        assert (a * mids[:, 0] + b * mids[:, 1]).tolist() == heights
        k, mid, margin = R.top_mid(row(a, b), rect)
        assert k == first and mid.tolist() == mids[first].tolist(), (a, b)
        assert margin == np.sort(heights)[-1] - np.sort(heights)[-2]
    # right = left alone at the top is impossible (their mean is the mean of top and bottom); a box of zero width makes them one point
    h = np.sqrt(0.5)
    # the panel lies flat (90 degrees about x: R[1][0] = R[1][1] = 0 exactly): 0 = 0 = 0 = 0, top is the first
    o, m = R.restate(_square([h, 0, 0, h]))
    assert o['rot_matrix'][0, 0, 1, 0] == 0 and o['rot_matrix'][0, 0, 1, 1] == 0
    assert o['top_mid'][0, 0] == 0 and m[0, 0] == 0
    # a box of zero height under the identity and under 180 degrees about x: the four points have one 3D height
    d = _square([0, 0, 0, 1])
    d['vertices'][0, 0, :4, 1] = 7.0
    assert R.restate(d)[0]['top_mid'][0, 0] == 0 and R.restate(d)[1][0, 0] == 0
    d['rotations'][0, 0] = [1, 0, 0, 0]
    assert R.restate(d)[0]['top_mid'][0, 0] == 0 and R.restate(d)[1][0, 0] == 0
    # a box of zero width turned by + and - 90 degrees about z (R[1][1] = 0 exactly: 3D y = +- c x with one x): all four tie again
    for z in (h, -h):
        d = _square([0, 0, z, h])
        d['vertices'][0, 0, :4, 0] = 5.0
        o, m = R.restate(d)
        assert o['rot_matrix'][0, 0, 1, 1] == 0 and o['top_mid'][0, 0] == 0 and m[0, 0] == 0


def test_restatement_rotations_by_hand():
    h = np.sqrt(0.5)
    for quat, top, want_t in (([0, 0, 0, 1], 0, [-10, -10, 0]),           # identity: top (10, 10)
                              ([1, 0, 0, 0], 1, [-10, 0, 0]),             # 180 about x: bottom (10, 0) -> (10, 0, 0)
                              ([0, 0, h, h], 2, [5, -20, 0]),             # + 90 about z: right (20, 5) -> (-5, 20, 0)
                              ([0, 0, -h, h], 3, [-5, 0, 0])):            # - 90 about z: left (0, 5) -> (5, 0, 0)
        o, _ = R.restate(_square(quat))
        assert o['top_mid'][0, 0] == top and np.abs(o['translation'][0, 0] - want_t).max() <= 1e-14, quat
        scaled, _ = R.restate(_square([3 * v for v in quat]))
        for k in R.KEYS:
            assert np.abs(scaled[k].astype(np.float64) - o[k]).max() <= 1e-12, k
    o, _ = R.restate(_square([0, 0, 0, 0]))
    assert o['place_flags'][0, 0] == R.BAD_QUAT and np.array_equal(o['rot_matrix'][0, 0], np.eye(3))
    for bad in ([np.nan, 0, 0, 1], [np.inf, 0, 0, 1], [1e200, 1e200, 0, 0]):
        assert R.restate(_square(bad))[0]['place_flags'][0, 0] == R.BAD_QUAT


def test_the_place_header_is_bound_and_exported():
    place = _lib.parse_header(_lib.PLACE_HEADER_PATH)
    others = {}
    for h in _lib.HEADERS + _lib.FEATURE_HEADERS + _lib.EVAL_HEADERS:
        others.update(_lib.parse_header(h))
    assert set(place) == {'gpe_pattern_place'} and not set(place) & set(others)
    assert _lib.PLACE_HEADERS == (_lib.PLACE_HEADER_PATH,)
    assert _lib.HEADERS == (_lib.HEADER_PATH, _lib.EXT_HEADER_PATH) and _lib.FEATURE_HEADERS == (_lib.FIT_HEADER_PATH,)
    assert _lib.EVAL_HEADERS == (_lib.EVAL_HEADER_PATH,)
    assert place['gpe_pattern_place'] == ('i', ['p'] * 7 + ['i'] * 3 + ['p'] * 7)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'gpe_pattern_place'), 'libgpe_hip.so does not export gpe_pattern_place'
    l = _lib.lib()
    assert l.gpe_abi_version() == 7
    fn = l.gpe_pattern_place
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_void_p] * 7 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 7
    # the definition is compiled against the declaration, and the build knows the header
    here = os.path.dirname(os.path.abspath(_lib.__file__))
    assert 'gpe_hip_place.h' in open(os.path.join(here, 'csrc', 'gpe_common.h')).read()
    assert 'gpe_hip_place.h' in open(os.path.join(here, 'build.py')).read()


def test_a_place_symbol_that_is_not_exported_fails_loudly(tmp_path, monkeypatch):
    h = tmp_path / 'place.h'
    h.write_text('int gpe_pattern_place_not_in_the_library(const double* x, void* stream);\n')
    monkeypatch.setattr(_lib, 'PLACE_HEADERS', (_lib.PLACE_HEADER_PATH, str(h)))
    monkeypatch.setattr(_lib, '_lib', None)
    with pytest.raises(AttributeError, match='gpe_pattern_place_not_in_the_library'):
        _lib.lib()


def test_off_menu_arguments_are_rejected_without_a_gpu():
    """The non-NULL 'device' pointers are made-up addresses: an entry point that refuses its arguments never touches them."""
    l = _lib.lib()
    A = 0x7f0000001000
    names = ('num_edges', 'num_verts', 'vertices', 'curvature', 'curved', 'rotations', 'translations', 'B', 'P', 'L', 'rot_matrix',
             'translation', 'top_mid', 'vertices3d', 'edges3d', 'place_flags')

    def place(**k):
        d = {n: A for n in names}
        d.update(B=6, P=23, L=14)
        d.update(k)
        return l.gpe_pattern_place(*[d[n] for n in names], None)

    for bad in ([dict(B=0), dict(B=-1), dict(P=0), dict(L=0), dict(P=-3), dict(L=-3), dict(P=25, L=41), dict(P=1025, L=1),
                 dict(P=1, L=1025), dict(P=65536, L=65536)] + [{n: None} for n in names if len(n) > 1]):
        assert place(**bad) == -22, bad


def test_python_checks_need_no_device():
    d = {k: torch.from_numpy(v) for k, v in _square([0, 0, 0, 1]).items()}
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.pattern_place(d)
    assert ops.PATTERN_PLACE_KEYS == R.KEYS
    dec = patterns.DecodedPatterns(dict(d, edge_slot=torch.zeros(1, 1, 4, dtype=torch.int32)))
    assert dec.placed is None and dec.pairs is None
    with pytest.raises(AttributeError):
        dec.edges3d
    with pytest.raises(ValueError, match='classifier'):
        dec.as_spec(0, stitches='classifier')
    with pytest.raises(ValueError, match="'tags' or 'classifier'"):
        dec.as_spec(0, stitches='both')

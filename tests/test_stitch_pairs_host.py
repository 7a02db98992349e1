"""not-gpu: stitch recovery from the edge-pair classifier (ops.stitch_pairs / StitchOnEdge3DPairs.predict_stitches).
  (1) the fp64 restatement (tests/stitch_pairs_restate.py) is pinned to the reference's own recorded output
      (tests/golden/stitch_pairs_*.pt, scripts/make_stitch_pairs_golden.py): enumeration order, the loop, the tie rule — with the
      reference's indexing of pattern_converter.py:432; the product implements the intended indexing;
  (2) the per-edge arg-max the kernels implement equals the literal double loop, on the fixtures and on hand-built ties;
  (3) the C ABI: symbols declared and exported, -22 on bad arguments without a GPU;
  (4) the host-side refusals."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import gpe_amd
from gpe_amd import _lib
import stitch_pairs_restate as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(f for f in glob.glob(os.path.join(HERE, 'golden', 'stitch_pairs_*.pt')) if 'known_answer' not in f)
IDS = [os.path.basename(f)[len('stitch_pairs_'):-3] for f in FIXTURES]
SYMBOLS = ('gpe_stitch_pairs_pack', 'gpe_stitch_pairs_planes', 'gpe_stitch_pairs_fwd', 'gpe_stitch_pairs_rows', 'gpe_stitch_pairs_reduce', 'gpe_stitch_select')


def _load(path):
    fx = torch.load(path, weights_only=False)
    fx['pairs'] = [tuple(int(v) for v in row) for row in fx['ref_order'].tolist()]
    return fx


def test_the_fixture_set_covers_the_cases():
    assert set(IDS) >= {'small', 'gaps', 'none', 'one', 'claimed', 'full'}
    fxs = {i: _load(f) for i, f in zip(IDS, FIXTURES)}
    assert fxs['none']['positives'] == 0 and fxs['one']['positives'] == 1
    assert fxs['full']['num_edges'].tolist() == [14] * 23 and len(fxs['full']['pairs']) == 49588
    ne = fxs['gaps']['num_edges'].tolist()
    assert 0 in ne[1:-1] and ne[0] == 0
    for fx in fxs.values():                 # the decision margins are a condition of a stored garment
        assert fx['margin_zero'] >= 4 * fx['tol'] and fx['margin_edge'] >= 4 * fx['tol']
    known = torch.load(os.path.join(HERE, 'golden', 'stitch_pairs_known_answer.pt'), weights_only=False)
    for f in FIXTURES:
        assert os.path.getsize(f) < os.path.getsize(os.path.join(HERE, 'golden', 'stitch_pairs_known_answer.pt'))
    # an edge claimed by several positives
    fx = fxs['claimed']
    lg = R.logits64(known['state_dict'], R.pair_rows(fx['edges'].numpy(), fx['pairs']), fx['f_shift'], fx['f_scale'])
    claims = {}
    for k in np.nonzero(lg > 0)[0]:
        for e in R._edges_of(fx['pairs'][k]):
            claims[e] = claims.get(e, 0) + 1
    assert max(claims.values()) >= 2


@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
def test_enumeration_is_the_references(path):
    fx = _load(path)
    assert R.enumerate_pairs(fx['num_edges'].tolist()) == fx['pairs']
    if 'ref_rows' in fx:
        rows = R.pair_rows(fx['edges'].numpy(), fx['pairs'])
        assert np.array_equal(rows.astype(np.float32), fx['ref_rows'].numpy())


@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
def test_restatement_reproduces_the_reference(path):
    fx = _load(path)
    logits = fx['ref_logits'].numpy()
    if fx['positives'] < 2:
        # zero positives: an empty list; one: the reference raises (`.squeeze().tolist()` is an int) — not reproduced
        assert (fx['ref_stitches'] == []) if fx['positives'] == 0 else (fx['ref_stitches'] is None and 'TypeError' in fx['ref_error'])
        assert len(R.stitches(fx['pairs'], logits, reference_indexing=False)) == fx['positives']
        return
    for loop in (False, True):
        got = R.stitches(fx['pairs'], logits, reference_indexing=True, loop=loop)
        assert [g[0] for g in got] == [tuple(r[0]) for r in fx['ref_stitches']]
        assert [np.float32(g[1]) for g in got] == [np.float32(r[1]) for r in fx['ref_stitches']]


@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
def test_fp64_logits_match_the_references(path):
    fx = _load(path)
    known = torch.load(os.path.join(HERE, 'golden', 'stitch_pairs_known_answer.pt'), weights_only=False)
    lg = R.logits64(known['state_dict'], R.pair_rows(fx['edges'].numpy(), fx['pairs']), fx['f_shift'], fx['f_scale'])
    assert np.abs(lg - fx['ref_logits'].double().numpy()).max() < R.tol_of(lg)
    assert R.positives(lg) == R.positives(fx['ref_logits'].numpy())


@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
@pytest.mark.parametrize('reference_indexing', [False, True])
def test_argmax_selection_is_the_double_loop(path, reference_indexing):
    fx = _load(path)
    logits = fx['ref_logits'].numpy()
    a = R.stitches(fx['pairs'], logits, reference_indexing, loop=False)
    b = R.stitches(fx['pairs'], logits, reference_indexing, loop=True)
    assert a == b
    if not reference_indexing:
        keys = [p for p, _ in a]
        assert keys == sorted(keys)                                       # list order = ascending order key
        edges = [e for p, _ in a for e in R._edges_of(p)]
        assert len(edges) == len(set(edges))                              # no edge in two survivors


def test_tie_rule_on_hand_built_cases():
    """exactly equal scores on a shared edge: the earlier pair of the list stays (the loop marks `other` unless base is LOWER)"""
    pairs = R.enumerate_pairs([2, 2, 2])
    pos = {p: k for k, p in enumerate(pairs)}
    cases = [
        ({(0, 1, 0, 0): 5.0, (0, 2, 0, 1): 5.0}, [(0, 1, 0, 0)]),
        ({(0, 1, 0, 0): 5.0, (0, 2, 0, 1): 5.0, (1, 2, 0, 1): 5.0}, [(0, 1, 0, 0)]),          # marks against the FULL list:
        ({(0, 1, 0, 0): 4.0, (0, 2, 0, 1): 5.0, (1, 2, 1, 1): 5.0}, [(0, 2, 0, 1)]),          # a marked stitch still marks
        ({(0, 1, 0, 0): 5.0, (0, 1, 1, 1): 5.0, (1, 2, 0, 0): 7.0}, [(0, 1, 1, 1), (1, 2, 0, 0)]),
        ({(0, 1, 0, 0): 5.0, (1, 2, 0, 0): 5.0, (0, 2, 1, 0): 5.0}, [(0, 1, 0, 0), (0, 2, 1, 0)]),
        ({(0, 2, 1, 1): 3.0}, [(0, 2, 1, 1)]),
        ({}, []),
    ]
    for scores, want in cases:
        logits = np.full(len(pairs), -8.5, dtype=np.float32)
        for p, s in scores.items():
            logits[pos[p]] = s
        for loop in (False, True):
            assert [p for p, _ in R.stitches(pairs, logits, loop=loop)] == want, (scores, loop)
    # randomised, scores drawn from three values so that ties are everywhere
    rng = np.random.default_rng(5)
    pairs = R.enumerate_pairs([3, 0, 4, 2, 3])
    for _ in range(200):
        logits = rng.choice(np.asarray([-8.5, 2.0, 2.0, 3.0], dtype=np.float32), size=len(pairs))
        for ri in (False, True):
            assert R.stitches(pairs, logits, ri, loop=False) == R.stitches(pairs, logits, ri, loop=True)


def test_header_declares_and_library_exports_the_entry_points():
    sigs = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in sigs and hasattr(raw, name), name
        res, args = sigs[name]
        assert res == 'i' and args[-1] == 'p', name
    assert _lib.lib().gpe_abi_version() == 7


def test_bad_arguments_are_rejected_without_a_gpu():
    l = _lib.lib()
    one = ctypes.c_void_p(16)       # a non-NULL pointer that is never dereferenced: the dimension checks come first
    assert l.gpe_stitch_pairs_pack(None, 4, 4, 4, None, None, 4, None) == -22
    assert l.gpe_stitch_pairs_pack(one, 4, 4, 4, None, one, 2, None) == -22                          # ldo < N
    assert l.gpe_stitch_pairs_fwd(None, 400, 200, 3, None, None, None, None, None, 1, 4, 4, None, None, None) == -22
    assert l.gpe_stitch_pairs_fwd(one, 400, 200, 3, one, None, None, one, one, 1, 33, 4, one, None, None) == -22   # P > 32
    assert l.gpe_stitch_pairs_fwd(one, 400, 200, 3, one, None, None, one, one, 1, 4, 17, one, None, None) == -22   # L > 16
    assert l.gpe_stitch_pairs_fwd(one, 400, 202, 3, one, None, None, one, one, 1, 4, 4, one, None, None) == -22    # H % 4
    assert l.gpe_stitch_pairs_fwd(one, 400, 200, 5, one, None, None, one, one, 1, 4, 4, one, None, None) == -22    # depth
    assert l.gpe_stitch_pairs_fwd(one, 600, 260, 3, one, None, None, one, one, 1, 4, 4, one, None, None) == -22    # H > 256
    assert l.gpe_stitch_pairs_planes(None, 200, 208, None, None, None) == -22
    assert l.gpe_stitch_pairs_planes(one, 200, 200, one, one, None) == -22                             # ldw % 16
    assert l.gpe_stitch_pairs_rows(None, None, 1, 4, 4, 8, None, None, 0, 4, 100, None, None) == -22
    sh = (ctypes.c_float * 16)(*([0.0] * 16))
    assert l.gpe_stitch_pairs_rows(one, one, 1, 4, 4, 8, sh, sh, 0, 17, 1000, one, None) == -22       # chunk beyond E
    assert l.gpe_stitch_pairs_rows(one, one, 1, 4, 4, 8, sh, sh, 0, 4, 3, one, None) == -22           # rows_chunk too small
    assert l.gpe_stitch_pairs_reduce(None, 1, None, 1, 4, 4, 0, 4, 48, None, None, None) == -22
    assert l.gpe_stitch_pairs_reduce(one, 1, one, 0, 4, 4, 0, 4, 48, one, None, None) == -22
    assert l.gpe_stitch_select(None, 1, 4, 4, None, None, None, None) == -22
    assert l.gpe_stitch_select(one, 1, 40, 4, one, one, one, None) == -22


def _model(element_size=16, hidden=200, layers=3):
    torch.manual_seed(3)
    return gpe_amd.nets.StitchOnEdge3DPairs({'element_size': element_size}, {'stitch_hidden_size': hidden, 'stitch_mlp_n_layers': layers},
                                            {}).eval()


STATS = {'f_shift': [0.0] * 16, 'f_scale': [1.0] * 16}


def test_cpu_tensors_are_refused():
    m = _model()
    with pytest.raises(RuntimeError, match='no CPU path'):
        m.predict_stitches(torch.zeros(1, 4, 5, 8), torch.full((1, 4), 5), STATS)
    with pytest.raises(RuntimeError, match='no CPU path'):
        gpe_amd.ops.stitch_pairs(torch.zeros(1, 4, 5, 8), torch.full((1, 4), 5), m.mlp, STATS['f_shift'], STATS['f_scale'], route='rows')


def test_host_side_refusals():
    m = _model()
    ne = lambda B, P, n: torch.full((B, P), n)
    with pytest.raises(ValueError):
        m.predict_stitches(torch.zeros(1, 33, 5, 8), ne(1, 33, 5), STATS)                 # P > 32
    with pytest.raises(ValueError):
        m.predict_stitches(torch.zeros(1, 4, 17, 8), ne(1, 4, 17), STATS)                 # L > 16
    with pytest.raises(ValueError):
        _model(element_size=15).predict_stitches(torch.zeros(1, 4, 5, 7), ne(1, 4, 5), {'f_shift': [0.0] * 15, 'f_scale': [1.0] * 15})
    with pytest.raises(ValueError):
        _model(hidden=30, layers=5).predict_stitches(torch.zeros(1, 4, 5, 8), ne(1, 4, 5), STATS, route='fused')
    with pytest.raises(ValueError):
        m.predict_stitches(torch.zeros(1, 4, 5, 8), ne(1, 4, 5), STATS, route='eager')
    assert gpe_amd.ops.stitch_pairs_on_menu(m.mlp) and not gpe_amd.ops.stitch_pairs_on_menu(_model(hidden=30, layers=5).mlp)
    assert not gpe_amd.ops.stitch_pairs_on_menu(_model(hidden=30, layers=2).mlp)           # 30 % 4
    assert gpe_amd.ops.stitch_pairs_on_menu(_model(hidden=256, layers=4).mlp)
    with pytest.raises(RuntimeError, match='eval'):
        m.train().predict_stitches(torch.zeros(1, 4, 5, 8), ne(1, 4, 5), STATS)

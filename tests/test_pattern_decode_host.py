"""-m "not gpu": the decode of a prediction to a sewing pattern on the host side —
  (1) the fp64 restatement (tests/pattern_decode_restate.py) reproduces what the reference's own functions made of the recorded
      predictions (tests/golden/pattern_decode_*.pt, scripts/make_pattern_decode_golden.py) exactly: vertices and curvature with ==
      on fp64, endpoints, panel order, stitches and whether InvalidPatternDefError was raised;
  (2) patterns.DecodedPatterns.as_spec on the restatement's tensors equals the recorded `pattern` dict, `rotation` included (the
      same scipy call on bit-equal input), gives the reference's truncated stitch list with strict=False and raises with strict=True;
  (3) the C entry points refuse off-menu shapes before any launch (no GPU needed to be refused)."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

import pattern_decode_restate as R
import quality_restate

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, 'golden', 'pattern_decode_*.pt')))
IDS = [os.path.basename(f)[15:-3] for f in FIXTURES]
_CACHE = {}


def _case(path):
    """fixture + its restatement, computed once and shared"""
    if path not in _CACHE:
        fx = torch.load(path, weights_only=False)
        dc = fx['data_config']
        out, margin = R.restate(fx['preds'], dc['standardize'], dc['explicit_stitch_tags'], stitches=fx['stitches'])
        _CACHE[path] = (fx, out, margin)
    return _CACHE[path]


def _decoded(out):
    import gpe_amd
    return gpe_amd.patterns.DecodedPatterns({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()})


def test_fixtures_exist():
    assert len(FIXTURES) == 3, FIXTURES


@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
def test_restatement_reproduces_the_reference(path):
    fx, out, margin = _case(path)
    assert margin >= quality_restate.MARGIN
    L = fx['data_config']['max_panel_len']
    seen = set()
    for b, (pat, raised) in enumerate(zip(fx['patterns'], fx['raised'])):
        slots = [p for p in range(out['new_panel_id'].shape[1]) if out['new_panel_id'][b, p] >= 0]
        assert pat['panel_order'] == ['panel_%d' % p for p in slots]
        assert [int(out['new_panel_id'][b, p]) for p in slots] == list(range(len(slots))) == list(range(out['num_panels'][b]))
        for p in slots:
            ref = pat['panels']['panel_%d' % p]
            n, nv = int(out['num_edges'][b, p]), int(out['num_verts'][b, p])
            want_v = np.asarray(ref['vertices'], np.float64)
            assert want_v.shape == (nv, 2) and (out['vertices'][b, p, :nv] == want_v).all()          # == on fp64
            assert (out['vertices'][b, p, nv:] == 0).all()
            assert len(ref['edges']) == n
            for k, e in enumerate(ref['edges']):
                assert e['endpoints'] == [k, k + 1 if k + 1 < nv else 0]
                assert ('curvature' in e) == bool(out['curved'][b, p, k])
                if 'curvature' in e:
                    assert (out['curvature'][b, p, k] == np.asarray(e['curvature'], np.float64)).all()
            assert bool(out['closed'][b, p]) == (ref['edges'][-1]['endpoints'][1] == 0)
            seen.add(('open', 'closed')[int(out['closed'][b, p])])
            seen.add('compacted' if (out['edge_slot'][b, p, :n] != np.arange(n)).any() else 'dense')
        if slots and slots != list(range(len(slots))):
            seen.add('renumbered')
        # stitches: the reference keeps those before the first invalid one, and raised exactly then
        first = int(out['first_invalid'][b])
        assert raised == (first >= 0)
        ns = first if raised else int(out['num_stitches'][b])
        got = [[{'panel': 'panel_%d' % (int(e) // L), 'edge': int(e) % L} for e in out['stitches'][b, :, k]] for k in range(ns)]
        assert got == pat['stitches']
        seen.add('raised' if raised else 'clean')
        if (out['stitch_flags'][b] & 2).any():
            seen.add('dropped_slot')
    assert {'closed', 'dense', 'raised', 'clean'} <= seen
    if 'lstm' in path:
        assert {'open', 'compacted', 'renumbered', 'dropped_slot'} <= seen, seen


@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
def test_as_spec_equals_the_recorded_pattern(path):
    fx, out, _ = _case(path)
    dec = _decoded(out)
    assert len(dec) == len(fx['patterns'])
    for b, (pat, raised) in enumerate(zip(fx['patterns'], fx['raised'])):
        spec = dec.as_spec(b)
        for panel in spec['panels'].values():
            tr = panel.pop('universal_translation')             # not the reference's key: the reference was given no translation
            assert len(tr) == 3 and 'translation' not in panel
        assert spec == pat                                      # vertices, edges, rotation, panel_order, truncated stitches
        if raised:
            assert len(spec['stitches']) == int(out['first_invalid'][b]) < int(out['num_stitches'][b])
            with pytest.raises(ValueError, match=r'stitch %d .*non-existing panel' % int(out['first_invalid'][b])):
                dec.as_spec(b, strict=True)
        else:
            strict = dec.as_spec(b, strict=True)
            assert strict['stitches'] == pat['stitches']


def test_panel_names_and_json(tmp_path):
    fx, out, _ = _case(FIXTURES[0])
    dec = _decoded(out)
    P = dec.max_pattern_len
    names = ['p%02d' % p for p in range(P)]
    spec = dec.as_spec(0, panel_names=names)
    assert spec['panel_order'] == [names[int(p[6:])] for p in fx['patterns'][0]['panel_order']]
    assert all(s['panel'] in spec['panels'] for st in spec['stitches'] for s in st)
    with pytest.raises(ValueError):
        dec.as_spec(0, panel_names=names[:-1])
    with pytest.raises(IndexError):
        dec.as_spec(len(dec))
    path = tmp_path / 'pattern.json'
    dec.to_json(0, str(path), panel_names=names)
    assert json.load(open(path)) == spec


def test_host_tensors_are_refused():
    import gpe_amd
    fx = torch.load(FIXTURES[0], weights_only=False)
    with pytest.raises(RuntimeError, match='no CPU path'):
        gpe_amd.ops.pattern_decode(fx['preds'], fx['data_config']['standardize'])
    with pytest.raises(RuntimeError, match='no CPU path'):
        gpe_amd.ops.tags_to_stitches(fx['preds']['stitch_tags'], fx['preds']['free_edges_mask'])


def test_stitch_model_has_no_patterns():
    import gpe_amd
    model = gpe_amd.nets.StitchOnEdge3DPairs({'element_size': 16}).eval()
    with pytest.raises(NotImplementedError, match='StitchOnEdge3DPairs'):
        model.predict_pattern(torch.zeros(1, 4, 16), {})


def test_off_menu_shapes_are_refused_by_the_library():
    """-22 before any launch: every pointer below is a dummy that a launch would fault on"""
    import gpe_amd
    lib = gpe_amd._lib.lib()
    stats = (ctypes.c_double * 64)()
    p = 64                                   # a non-NULL address that is never dereferenced on the host

    def decode(P, L, D, R=4, T=3, S=None, given=None):
        S = P * L // 2 if S is None else S
        return lib.gpe_pattern_decode(p, 0, 0, 0, p, 0, R, p, 0, T, p, 0, 0, 0, D, p, 0, 0, 0, given, None, 1, P, L, S, 0, stats,
                                      p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, None)

    assert decode(25, 41, 3) == -22          # P * L = 1025
    assert decode(1025, 1, 3) == -22
    assert decode(23, 14, 9) == -22          # D = 9
    assert decode(23, 14, 0) == -22
    assert decode(23, 14, 3, R=9) == -22
    assert decode(23, 14, 3, T=0) == -22
    assert decode(23, 14, 3, S=160) == -22   # the found stitches need S = P * L / 2
    assert decode(0, 14, 3) == -22
    assert lib.gpe_tags_to_stitches(p, 0, 0, 0, 3, p, 0, 0, 0, 1, 25, 41, p, p, None) == -22
    assert lib.gpe_tags_to_stitches(p, 0, 0, 0, 9, p, 0, 0, 0, 1, 23, 14, p, p, None) == -22
    assert lib.gpe_abi_version() == 7

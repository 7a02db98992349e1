"""-m gpu: the panels of a decoded prediction placed in 3D on the device (csrc/gpe_pattern_place.hip through ops.pattern_place,
DecodedPatterns.place and model.predict_garment) against
  (1) the fp64 restatement (tests/pattern_place_restate.py) on the reference fixture, over the shape menu and on the edge cases, each
      built by hand at unit statistics: integers exactly, fp64 within 1e-9 absolute, the fp32 edge rows within 1 ulp, tails exactly 0;
  (2) the reference's own `translation` per panel (tests/golden/pattern_place_small.pt) through DecodedPatterns.as_spec;
plus run-to-run and CU-reservation bit equality, model.predict_garment against its three steps bit for bit with the shipped
classifier weights, both inside a stream capture, strided views, and the refusals off the menu.

The tolerances are those of tests/test_pattern_place_host.py (derived there).  Drawn inputs keep a margin >= 1e-3 at every panel's
one decision (asserted), so fp64 on host and device decide alike; no panel is skipped."""
import copy
import os

import numpy as np
import pytest
import torch

import pattern_decode_restate as D
import pattern_place_restate as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
UNIT = {'gt_shift': {'outlines': [0, 0, 0, 0], 'rotations': [0, 0, 0, 0], 'translations': [0, 0, 0], 'stitch_tags': [0, 0, 0]},
        'gt_scale': {'outlines': [1, 1, 1, 1], 'rotations': [1, 1, 1, 1], 'translations': [1, 1, 1], 'stitch_tags': [1, 1, 1]}}
INPUTS = ('num_edges', 'num_verts', 'vertices', 'curvature', 'curved', 'rotations', 'translations')
H = float(np.sqrt(0.5))


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


@pytest.fixture(scope='module')
def fx():
    return torch.load(os.path.join(GOLDEN, 'pattern_place_small.pt'), weights_only=False)


def _cuda(d):
    return {k: (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).clone().cuda() for k, v in d.items()}


def _ordered(a):
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _compare(got, want, num_edges, num_verts):
    """the device's dict against the restatement's; -> the device's as numpy"""
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert tuple(got) == R.KEYS
    for k in R.KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, got[k].dtype)
    for k in ('top_mid', 'place_flags'):
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:5])
    for k in ('rot_matrix', 'translation', 'vertices3d'):
        assert np.isfinite(got[k]).all() and np.abs(got[k] - want[k]).max() <= 1e-9, (k, np.abs(got[k] - want[k]).max())
    assert np.abs(_ordered(got['edges3d']) - _ordered(want['edges3d'])).max() <= 1
    # tails and empty panels: zeros, exactly (+ 0.0: the bytes)
    L = want['edges3d'].shape[2]
    edge_tail = np.arange(L)[None, None, :] >= num_edges[:, :, None]
    vert_tail = np.arange(L + 1)[None, None, :] >= num_verts[:, :, None]
    assert not got['edges3d'].view(np.int32)[edge_tail].any() and not got['vertices3d'].view(np.int64)[vert_tail].any()
    empty = num_edges == 0
    assert not got['rot_matrix'].view(np.int64)[empty].any() and not got['translation'].view(np.int64)[empty].any()
    assert (got['top_mid'][empty] == -1).all()
    return got


def _check(gpe, decoded, min_margin=1e-3):
    """ops.pattern_place on decoded numbers (numpy, PATTERN_PLACE_INPUTS) against the restatement -> (device's, restatement's)"""
    want, margins = R.restate(decoded)
    if min_margin is not None:
        assert margins.min() >= min_margin, margins.min()
    got = gpe.ops.pattern_place(_cuda({k: decoded[k] for k in INPUTS}))
    torch.cuda.synchronize()
    assert tuple(got) == gpe.ops.PATTERN_PLACE_KEYS
    return _compare(got, want, decoded['num_edges'], decoded['num_verts']), want


# ---- the reference fixture -------------------------------------------------------------------------------------------------------------
def test_fixture_against_restatement_and_the_reference_translation(gpe, fx):
    dc = fx['data_config']
    want_dec = D.restate(fx['preds'], dc['standardize'], False)[0]
    want, margins = R.restate(want_dec)
    assert margins.min() >= 1e-3
    dec = gpe.patterns.DecodedPatterns(gpe.ops.pattern_decode(_cuda(fx['preds']), dc['standardize'], False))
    assert dec.placed is None and dec.place() is dec and tuple(dec.placed) == R.KEYS
    again = dec.placed
    assert dec.place().placed is again                      # placed once
    _compare(dec.placed, want, want_dec['num_edges'], want_dec['num_verts'])
    assert dec.edges3d is dec.placed['edges3d'] and dec.translation.shape == (6, 23, 3)
    for b, g in enumerate(fx['garments']):
        spec = dec.as_spec(b)
        pat = copy.deepcopy(g['pattern'])
        assert list(spec['panels']) == list(pat['panels']) and len(spec['panels']) > 0
        for name, panel in spec['panels'].items():
            ref_t = pat['panels'][name].pop('translation')
            assert np.abs(np.asarray(panel.pop('translation')) - np.asarray(ref_t)).max() <= 1e-9, (b, name)
            assert len(panel.pop('universal_translation')) == 3
        assert spec == pat, b                               # everything else is the decode's, equal as before


# ---- the shape menu on drawn panels ----------------------------------------------------------------------------------------------------
def _draw(rng, B, P, L):
    """what a decode leaves (closed and open loops of 3 .. L edges, empty panels anywhere, curved flags, quaternions of any length),
    every panel redrawn until its top-midpoint margin is >= 1e-3"""
    d = {'num_edges': np.zeros((B, P), np.int32), 'num_verts': np.zeros((B, P), np.int32), 'vertices': np.zeros((B, P, L + 1, 2)),
         'curvature': np.zeros((B, P, L, 2)), 'curved': np.zeros((B, P, L), np.int32),
         'rotations': rng.normal(0, 1, (B, P, 4)) * rng.uniform(0.2, 5, (B, P, 1)), 'translations': rng.normal(0, 40, (B, P, 3))}
    for b in range(B):
        for p in range(P):
            n = int(rng.choice([0] + list(range(3, L + 1)))) if (b, p) != (0, 0) else L
            if n == 0:
                continue
            while True:
                nv = n + int(rng.integers(0, 2))
                verts = rng.uniform(-60, 60, (nv, 2))
                verts[0] = 0.0
                quat = rng.normal(0, 1, 4) * rng.uniform(0.2, 5)
                if R.top_mid(R.quat_matrix(quat)[0], verts)[2] >= 1e-3:
                    break
            d['num_edges'][b, p], d['num_verts'][b, p] = n, nv
            d['vertices'][b, p, :nv], d['rotations'][b, p] = verts, quat
            d['curved'][b, p, :n] = rng.integers(0, 2, n)
            d['curvature'][b, p, :n] = rng.uniform(-0.5, 0.9, (n, 2))          # kept by the decode whether curved or not
    return d


@pytest.mark.parametrize('B,P,L', [(1, 1, 3), (3, 3, 4), (6, 23, 14), (2, 64, 16), (67, 5, 14)])
def test_shape_menu_against_restatement(gpe, B, P, L):
    d = _draw(np.random.default_rng(100 * P + L), B, P, L)
    got, want = _check(gpe, d)
    assert (want['top_mid'] >= 0).sum() == (d['num_edges'] > 0).sum() > 0
    if B * P >= 100:
        assert set(want['top_mid'][d['num_edges'] > 0].tolist()) == {0, 1, 2, 3}


# ---- the edge cases, by hand at unit statistics through the decode ---------------------------------------------------------------------
# a 20 x 10 rectangle from the origin; side midpoints: top (10, 10), bottom (10, 0), right (20, 5), left (0, 5)
RECT = [(20, 0, 0, 0), (0, 10, 0.5, 0.25), (-20, 0, 0, 0), (0, -10, 0, 0)]


def _blank(P, L, B=1):
    rot = torch.zeros(B, P, 4)
    rot[..., 3] = 1.0
    return {'outlines': torch.zeros(B, P, L, 4), 'rotations': rot, 'translations': torch.zeros(B, P, 3),
            'stitch_tags': torch.zeros(B, P, L, 3), 'free_edges_mask': torch.full((B, P, L), 3.0)}


def _panel(preds, p, rows, at=None, b=0):
    for l, r in zip(range(len(rows)) if at is None else at, rows):
        preds['outlines'][b, p, l] = torch.tensor(r, dtype=torch.float32)


def _decode_place(gpe, preds, min_margin=1e-3):
    """decode on the device, place on the device; the restatements of both on the host -> (DecodedPatterns, device's, restatement's)"""
    dec = gpe.patterns.DecodedPatterns(gpe.ops.pattern_decode(_cuda(preds), UNIT))
    want_dec = D.restate(preds, UNIT)[0]
    for k in INPUTS:
        assert np.array_equal(dec.tensors[k].cpu().numpy(), want_dec[k], equal_nan=want_dec[k].dtype == np.float64), k
    want, margins = R.restate(want_dec)
    if min_margin is not None:
        assert margins.min() >= min_margin
    got = _compare(dec.place().placed, want, want_dec['num_edges'], want_dec['num_verts'])
    return dec, got, want


def test_empty_panel_between_real_ones_dropped_row_and_open_loop(gpe):
    preds = _blank(4, 6)
    _panel(preds, 0, RECT, at=[0, 1, 3, 5])                  # rows 2 and 4 stay padding: the edge rows are compact
    _panel(preds, 1, RECT[:2])                               # two kept rows: empty
    _panel(preds, 2, RECT)
    _panel(preds, 3, [(20, 0, 0, 0), (0, 10, 0, 0), (-20, 0, 0, 0), (0, -5, 0.3, 0)])      # ends at (0, 5): open, a fifth vertex
    preds['translations'][0, :, 0] = torch.tensor([1.0, 2.0, 3.0, 4.0])
    dec, got, want = _decode_place(gpe, preds)
    assert dec.num_edges[0].tolist() == [4, 0, 4, 4] and dec.num_verts[0].tolist() == [4, 0, 4, 5]
    assert got['top_mid'][0].tolist() == [0, -1, 0, 0]
    # identity: top (10, 10) goes to the universal translation (x, 0, 0)
    assert got['translation'][0].tolist() == [[-9, -10, 0], [0, 0, 0], [-7, -10, 0], [-6, -10, 0]]
    assert got['vertices3d'][0, 0, :4].tolist() == [[-9, -10, 0], [11, -10, 0], [11, 0, 0], [-9, 0, 0]]
    # panel 0, compact rows: edge 1 is the decoder's row 1 (curved), edge 3 returns to vertex 0
    assert got['edges3d'][0, 0, 1].tolist() == [11, -10, 0, 11, 0, 0, 0.5, 0.25]
    assert got['edges3d'][0, 0, 3].tolist() == [-9, 0, 0, -9, -10, 0, 0, 0]
    # the open loop: its last edge ends at the extra vertex, not at vertex 0
    assert got['vertices3d'][0, 3, 4].tolist() == [-6, -5, 0]
    assert got['edges3d'][0, 3, 3].tolist() == [-6, 0, 0, -6, -5, 0, np.float32(0.3), 0]
    spec = dec.as_spec(0)
    assert list(spec['panels']) == ['panel_0', 'panel_2', 'panel_3']
    assert spec['panels']['panel_2']['translation'] == [-7, -10, 0]
    assert spec['panels']['panel_2']['universal_translation'] == [3, 0, 0]


def test_rotations_choose_each_midpoint_and_any_length_is_normalised(gpe):
    quats = [(0, 0, 0, 1), (1, 0, 0, 0), (0, 0, H, H), (0, 0, -H, H)]      # identity, 180 about x, + 90 about z, - 90 about z
    preds = _blank(8, 4)
    for p in range(8):
        _panel(preds, p, RECT)
        preds['rotations'][0, p] = torch.tensor(quats[p % 4]) * (1.0 if p < 4 else 3.0)
    dec, got, want = _decode_place(gpe, preds)
    assert got['top_mid'][0].tolist() == [0, 1, 2, 3] * 2 and not got['place_flags'].any()
    for k in ('rot_matrix', 'translation', 'vertices3d'):
        assert np.abs(got[k][0, 4:] - got[k][0, :4]).max() <= 1e-12, k
    want_t = np.array([[-10, -10, 0], [-10, 0, 0], [5, -20, 0], [-5, 0, 0]], np.float64)
    assert np.abs(got['translation'][0, :4] - want_t).max() <= 1e-12


def test_exact_ties_go_to_the_first_midpoint(gpe):
    preds = _blank(3, 4)
    _panel(preds, 0, RECT)                                   # lies flat (90 about x): R[1][0] = R[1][1] = 0, four equal heights
    preds['rotations'][0, 0] = torch.tensor([H, 0, 0, H])
    _panel(preds, 1, [(0, 10, 0, 0), (0, 10, 0, 0), (0, -20, 0, 0)])        # a box of zero width, + 90 about z: 3D y = c x
    preds['rotations'][0, 1] = torch.tensor([0, 0, H, H])
    _panel(preds, 2, [(10, 0, 0, 0), (10, 0, 0, 0), (-20, 0, 0, 0)])        # a box of zero height under the identity
    dec, got, want = _decode_place(gpe, preds, min_margin=None)
    assert got['top_mid'][0].tolist() == [0, 0, 0]
    assert got['rot_matrix'][0, 0, 1, :2].tolist() == [0, 0] and got['rot_matrix'][0, 1, 1, 1] == 0


def test_zero_and_non_finite_quaternions_set_the_flag_and_as_spec_raises(gpe):
    preds = _blank(4, 4, B=2)
    for p in range(4):
        _panel(preds, p, RECT)
        _panel(preds, p, RECT, b=1)
    preds['rotations'][0, 1] = 0.0
    preds['rotations'][0, 2] = torch.tensor([float('nan'), 0, 0, 1])
    preds['rotations'][0, 3] = torch.tensor([float('inf'), 0, 0, 1])
    dec, got, want = _decode_place(gpe, preds)
    assert got['place_flags'].tolist() == [[0, 1, 1, 1], [0, 0, 0, 0]]
    assert np.array_equal(got['rot_matrix'][0, 1], np.eye(3)) and got['translation'][0, 1].tolist() == [-10, -10, 0]
    with pytest.raises(ValueError, match='panel 1 .*quaternion'):
        dec.as_spec(0)
    assert 'translation' in dec.as_spec(1)['panels']['panel_3']


def test_two_runs_and_a_cu_reservation_give_the_same_bits(gpe, fx):
    dc = fx['data_config']
    decoded = gpe.ops.pattern_decode(_cuda(fx['preds']), dc['standardize'], False)
    a = gpe.ops.pattern_place(decoded)
    b = gpe.ops.pattern_place(decoded)
    prev = gpe._lib.set_reserved_cus(64)
    try:
        c = gpe.ops.pattern_place(decoded)
    finally:
        gpe._lib.set_reserved_cus(prev)
    torch.cuda.synchronize()
    for k in R.KEYS:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
        assert torch.equal(a[k].view(torch.uint8), c[k].view(torch.uint8)), k


def test_strided_views_equal_contiguous_copies(gpe, fx):
    dc = fx['data_config']
    # the predictions as strided views of one wide tensor, as a model's heads leave them
    B, P, L = fx['preds']['outlines'].shape[:3]
    wide = torch.zeros(B, P, L, 9)
    wide[..., :4], wide[..., 4:7], wide[..., 7] = fx['preds']['outlines'], fx['preds']['stitch_tags'], fx['preds']['free_edges_mask']
    wide = wide.cuda()
    rt = torch.cat([fx['preds']['rotations'], fx['preds']['translations']], -1).cuda()
    views = {'outlines': wide[..., :4], 'stitch_tags': wide[..., 4:7], 'free_edges_mask': wide[..., 7], 'rotations': rt[..., :4],
             'translations': rt[..., 4:]}
    assert not views['outlines'].is_contiguous() and not views['rotations'].is_contiguous()
    a = gpe.patterns.DecodedPatterns(gpe.ops.pattern_decode(views, dc['standardize'], False)).place()
    b = gpe.patterns.DecodedPatterns(gpe.ops.pattern_decode(_cuda(fx['preds']), dc['standardize'], False)).place()
    # ... and the decode's tensors as strided views into place itself
    t = dict(b.tensors)
    pad = torch.zeros(B, P, L + 1, 5, device='cuda', dtype=torch.float64)
    pad[..., 1:3] = t['vertices']
    t['vertices'] = pad[..., 1:3]
    t['num_edges'] = torch.stack([t['num_edges'], t['num_edges']], -1)[..., 1]
    assert not t['vertices'].is_contiguous() and not t['num_edges'].is_contiguous()
    c = gpe.ops.pattern_place(t)
    torch.cuda.synchronize()
    for k in R.KEYS:
        assert torch.equal(a.placed[k].view(torch.uint8), b.placed[k].view(torch.uint8)), k
        assert torch.equal(c[k].view(torch.uint8), b.placed[k].view(torch.uint8)), k


def test_off_menu_shapes_and_widths_raise_before_any_launch(gpe):
    def decoded(B, P, L, Rw=4, T=3):
        z = lambda *s, dt=torch.float64: torch.zeros(*s, device='cuda', dtype=dt)      # noqa: E731
        i32 = torch.int32
        return {'num_edges': z(B, P, dt=i32), 'num_verts': z(B, P, dt=i32), 'vertices': z(B, P, L + 1, 2), 'curvature': z(B, P, L, 2),
                'curved': z(B, P, L, dt=i32), 'rotations': z(B, P, Rw), 'translations': z(B, P, T)}
    with pytest.raises(ValueError, match='1 <= P \\* L'):
        gpe.ops.pattern_place(decoded(1, 25, 41))
    with pytest.raises(ValueError, match='rotation width 4'):
        gpe.ops.pattern_place(decoded(1, 2, 4, Rw=6))
    with pytest.raises(ValueError, match='width 3'):
        gpe.ops.pattern_place(decoded(1, 2, 4, T=2))
    bad = decoded(1, 2, 4)
    bad['vertices'] = bad['vertices'].float()
    with pytest.raises(ValueError, match='vertices'):
        gpe.ops.pattern_place(bad)
    with pytest.raises(RuntimeError, match='no CPU path'):
        gpe.ops.pattern_place({k: v.cpu() for k, v in decoded(1, 2, 4).items()})
    ok = gpe.ops.pattern_place(decoded(2, 64, 16))          # the P * L = 1024 edge, every panel empty
    torch.cuda.synchronize()
    assert (ok['top_mid'] == -1).all() and not ok['edges3d'].any()


# ---- the models ------------------------------------------------------------------------------------------------------------------------
def _models(gpe):
    fx = torch.load(os.path.join(GOLDEN, 'full3d_small.pt'), weights_only=False)
    torch.manual_seed(fx['seed'])
    model = getattr(gpe.nets, fx['model'])(fx['data_config'], copy.deepcopy(fx['nn_config']), copy.deepcopy(fx['loss_config']))
    model.load_state_dict(fx['state_dict'])
    known = torch.load(os.path.join(GOLDEN, 'stitch_pairs_known_answer.pt'), weights_only=False)
    stitch = gpe.nets.StitchOnEdge3DPairs(known['data_config'], dict(known['nn_config']), {})
    stitch.load_state_dict(known['state_dict'])                                            # the shipped classifier weights
    full = torch.load(os.path.join(GOLDEN, 'stitch_pairs_full.pt'), weights_only=False)
    return fx, model.cuda().eval(), stitch.cuda().eval(), {'f_shift': full['f_shift'], 'f_scale': full['f_scale']}


def _bits_equal(a, b):
    assert tuple(a) == tuple(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), k


def test_predict_garment_is_predict_pattern_place_predict_stitches(gpe):
    fx, model, stitch, stats = _models(gpe)
    x, dc = fx['features'].cuda(), fx['data_config']
    torch.manual_seed(5)                                     # the decoders draw their start states on the CPU generator
    d = model.predict_garment(x, dc, stitch, stats)
    torch.manual_seed(5)
    want = model.predict_pattern(x, dc)
    placed = gpe.ops.pattern_place(want.tensors)
    out = stitch.predict_stitches(placed['edges3d'], want.num_edges, stats)
    torch.cuda.synchronize()
    _bits_equal(d.tensors, want.tensors)
    _bits_equal(d.placed, placed)
    _bits_equal(d.pairs, {'pair_stitches': out['stitches'], 'num_pair_stitches': out['num_stitches'], 'pair_scores': out['scores']})
    assert d.pair_stitches is d.pairs['pair_stitches'] and d.pair_scores.shape == (x.shape[0], 23 * 14 // 2)
    # keywords reach predict_stitches
    torch.manual_seed(5)
    rows = model.predict_garment(x, dc, stitch, stats, route='auto', return_logits=False)
    _bits_equal(rows.pairs, d.pairs)
    stitch.train()
    with pytest.raises(RuntimeError, match='eval'):
        model.predict_garment(x, dc, stitch, stats)


def test_classifier_stitches_through_as_spec(gpe, fx):
    """the fixture's garments sewn by the shipped classifier: as_spec(stitches='classifier') names panels and kept-edge indices"""
    _, _, stitch, stats = _models(gpe)
    dc = fx['data_config']
    d = gpe.patterns.DecodedPatterns(gpe.ops.pattern_decode(_cuda(fx['preds']), dc['standardize'], False)).place()
    d.attach_pair_stitches(stitch.predict_stitches(d.edges3d, d.num_edges, stats))
    st, ns, sc = d.pair_stitches.cpu().numpy(), d.num_pair_stitches.cpu().numpy(), d.pair_scores.cpu().numpy()
    ne = d.num_edges.cpu().numpy()
    L = 14
    for b in range(len(d)):
        spec = d.as_spec(b, stitches='classifier')
        tags = d.as_spec(b)
        assert spec['panels'] == tags['panels'] and spec['panel_order'] == tags['panel_order']
        assert all('translation' in p for p in spec['panels'].values())
        assert len(spec['stitches']) == ns[b]
        for k, (s0, s1) in enumerate(spec['stitches']):
            for side, s in enumerate((s0, s1)):
                e = int(st[b, side, k])
                assert s == {'panel': 'panel_%d' % (e // L), 'edge': e % L, 'score': float(sc[b, k])}
                assert s['panel'] in spec['panels'] and s['edge'] < ne[b, e // L]          # an index into the panel's edge list


def _capture(side, fn):
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        out = fn()
    return cg, out


def test_place_inside_a_stream_capture(gpe, fx):
    dc = fx['data_config']
    decoded = gpe.ops.pattern_decode(_cuda(fx['preds']), dc['standardize'], False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = gpe.ops.pattern_place(decoded)
        side.synchronize()
        cg, again = _capture(side, lambda: gpe.ops.pattern_place(decoded))
        for t in again.values():
            t.fill_(-7)
        cg.replay()
    torch.cuda.synchronize()
    _bits_equal(again, eager)


def test_predict_garment_inside_a_stream_capture(gpe):
    """the whole of predict_garment captured, the start states of the decoders fed through graph.HostDrawn as a captured training step
    feeds them: the replay equals the eager call bit for bit"""
    fx, model, stitch, stats = _models(gpe)
    x, dc = fx['features'].cuda(), fx['data_config']
    from gpe_amd import graph
    host = graph.HostDrawn(x.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    gpe.ops.HOST_DRAWN = host
    groups = lambda d: {**d.tensors, **d.placed, **d.pairs}          # noqa: E731
    try:
        with torch.cuda.stream(side):
            for _ in range(2):                               # warm-up: workspaces, packs, the host-drawn tensors get their buffers
                torch.manual_seed(5)
                host.begin_step()
                eager = model.predict_garment(x, dc, stitch, stats)
            eager = {k: v.clone() for k, v in groups(eager).items()}
            side.synchronize()
            host.cursor, host.capturing = 0, True
            cg, d = _capture(side, lambda: model.predict_garment(x, dc, stitch, stats))
            host.capturing = False
            for t in groups(d).values():
                t.fill_(-7)
            torch.manual_seed(5)
            host.begin_step()
            cg.replay()
        torch.cuda.synchronize()
    finally:
        gpe.ops.HOST_DRAWN = None
    _bits_equal(groups(d), eager)

"""-m gpu: a prediction decoded to a sewing pattern on the device (csrc/gpe_pattern_decode.hip through ops.pattern_decode,
ops.tags_to_stitches and model.predict_pattern) against
  (1) the fp64 restatement (tests/pattern_decode_restate.py): every output tensor bit for bit, over the shape menu and the edge
      cases of the decode, each built by hand at unit statistics;
  (2) the reference's own results (tests/golden/pattern_decode_*.pt) through DecodedPatterns.as_spec;
  (3) the quality metrics' stitch precision / recall (the same pairing code, csrc/gpe_stitch_greedy.h) recomputed on the host from
      ops.tags_to_stitches' pairs;
plus the refusals off the menu, the strided views of a model's output against contiguous copies, model.predict_pattern for both
pattern models, and both inside a stream capture (no host read; the replay equals the eager call bit for bit).

The greedy pairing measures distances in fp32 where the restatement has fp64: every drawn input keeps a relative margin >=
quality_restate.MARGIN between a decision and its runner-up (asserted); hand-built ties use exactly representable distances."""
import copy
import glob
import os

import numpy as np
import pytest
import torch

import pattern_decode_restate as R
import quality_restate

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, 'pattern_decode_*.pt')))
UNIT = {'gt_shift': {'outlines': [0, 0, 0, 0], 'rotations': [0, 0, 0, 0], 'translations': [0, 0, 0], 'stitch_tags': [0, 0, 0]},
        'gt_scale': {'outlines': [1, 1, 1, 1], 'rotations': [1, 1, 1, 1], 'translations': [1, 1, 1], 'stitch_tags': [1, 1, 1]}}


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _cuda(d):
    return {k: v.clone().cuda() for k, v in d.items()}


def _same(got, want, key):
    """bit-equal; NaN equals NaN whatever its payload"""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (key, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float64:
        nan = np.isnan(want)
        assert (np.isnan(got) == nan).all(), key
        assert (got.view(np.int64)[~nan] == want.view(np.int64)[~nan]).all(), (key, np.argwhere(got != want)[:5])
    else:
        assert (got == want).all(), (key, np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])


def _check(gpe, preds, stats, explicit=False, stitches=None, num_stitches=None, want=None):
    """ops.pattern_decode on the device against the restatement: every output tensor -> the restatement's dict"""
    if want is None:
        want = R.restate(preds, stats, explicit, stitches=stitches, num_stitches=num_stitches)[0]
    got = gpe.ops.pattern_decode(_cuda(preds), stats, explicit, stitches=None if stitches is None else stitches.cuda(),
                                 num_stitches=None if num_stitches is None else num_stitches.cuda())
    torch.cuda.synchronize()
    assert tuple(got) == gpe.ops.PATTERN_DECODE_KEYS == R.KEYS
    for k in R.KEYS:
        _same(got[k], np.ascontiguousarray(want[k]), k)
    return want


# ---- the shape menu on drawn garments ------------------------------------------------------------------------------------------------
def _stats(rng, D):
    fx = torch.load(os.path.join(GOLDEN, 'quality_lstm_e40.pt'), weights_only=False)
    st = copy.deepcopy(fx['data_config']['standardize'])
    st['gt_shift']['stitch_tags'] = rng.uniform(-2, 2, D).tolist()
    st['gt_scale']['stitch_tags'] = rng.uniform(1.5, 2.5, D).tolist()
    return st


def _draw(rng, B, P, L, D, stats):
    """garments of closed / opened loops with padding rows at the end or in the middle, empty panels anywhere, and stitch tags whose
    pairing is decided by construction: the two edges of pair k lie delta_k apart, delta_k rising by 1e-3 of itself per pair, and the
    pairs sit on distinct points of the integer lattice.  Garment 0 has every edge non-free (P * L non-free edges: the limit)."""
    sh = np.asarray(stats['gt_shift']['outlines'], np.float64)
    sc = np.asarray(stats['gt_scale']['outlines'], np.float64)
    pad = -sh / sc
    ol = np.tile(pad, (B, P, L, 1))
    E = P * L
    tags = rng.uniform(-3, 3, (B, E, D))
    logit = rng.uniform(1, 4, (B, E))
    side = 9 if D == 3 else 3
    for b in range(B):
        for p in range(P):
            n = int(rng.choice([0, 2, L] + list(range(3, L + 1))))
            if n >= 3:
                loop = quality_restate._loop_cm(rng, n)
                kind = rng.integers(0, 4)
                if kind == 1:
                    loop[0, 0] += 10.0                                   # opened
                rows = np.arange(n)
                if kind == 2 and n < L:
                    rows = np.sort(rng.choice(L, n, replace=False))      # padding rows in the middle
                ol[b, p, rows] = (loop - sh) / sc
            elif n == 2:
                ol[b, p, :2] = (quality_restate._loop_cm(rng, 3)[:2] - sh) / sc
        m = E if b == 0 else int(rng.integers(0, min(E, 48) + 1))
        edges = rng.permutation(E)[:m]
        logit[b, edges] = -rng.uniform(1, 4, m)
        if m % 2:                                                       # the dropped edge: the largest logit by a margin
            logit[b, edges[-1]] = -0.5
        cells = rng.permutation(side ** D)[:m // 2]
        for k in range(m // 2):
            c = np.array([(cells[k] // side ** d) % side for d in range(D)], np.float64) - side // 2
            delta = 0.01 * 1.001 ** k
            tags[b, edges[2 * k]] = c
            tags[b, edges[2 * k + 1]] = c
            tags[b, edges[2 * k + 1], k % D] += delta
    f = lambda a: torch.tensor(a, dtype=torch.float32)      # noqa: E731
    return {'outlines': f(ol), 'rotations': f(rng.normal(0, 1, (B, P, 4))), 'translations': f(rng.normal(0, 1, (B, P, 3))),
            'stitch_tags': f(tags.reshape(B, P, L, D)), 'free_edges_mask': f(logit.reshape(B, P, L))}


_DRAWS = {}


def _drawn(P, L, D):
    """one draw of 67 garments per shape and its restatement, shared by the batch sizes (the decode is per garment)"""
    key = (P, L, D)
    if key not in _DRAWS:
        rng = np.random.default_rng(1000 * P + 10 * L + D)
        stats = _stats(rng, D)
        explicit = D == 8
        preds = _draw(rng, 67, P, L, D, stats)
        if explicit:                                        # the lattice lies in the un-standardised tags
            sh, sc = (torch.tensor(stats[k]['stitch_tags'], dtype=torch.float32) for k in ('gt_shift', 'gt_scale'))
            preds['stitch_tags'] = (preds['stitch_tags'] - sh) / sc
        detail = {}
        want = R.restate(preds, stats, explicit, detail=detail)[0]
        _DRAWS[key] = (preds, stats, explicit, want, detail['pairing'])
    return _DRAWS[key]


@pytest.mark.parametrize('D', [3, 8])
@pytest.mark.parametrize('B', [1, 3, 67])
@pytest.mark.parametrize('P,L', [(1, 3), (3, 4), (5, 14), (23, 14), (32, 32)])
def test_shape_menu_against_restatement(gpe, P, L, B, D):
    preds, stats, explicit, want, margin = _drawn(P, L, D)
    assert margin >= quality_restate.MARGIN, margin
    assert want['num_stitches'][0] == P * L // 2            # garment 0: every edge paired
    _check(gpe, {k: v[:B] for k, v in preds.items()}, stats, explicit, want={k: v[:B] for k, v in want.items()})


# ---- the edge cases, by hand at unit statistics ----------------------------------------------------------------------------------------
SQUARE = [(10, 0, 0, 0), (0, 10, 0.5, 0.25), (-10, 0, 0, 0), (0, -10, 0, 0)]


def _blank(P, L, D=3, B=1):
    rot = torch.zeros(B, P, 4)
    rot[..., 3] = 1.0                                        # the identity quaternion
    return {'outlines': torch.zeros(B, P, L, 4), 'rotations': rot, 'translations': torch.zeros(B, P, 3),
            'stitch_tags': torch.zeros(B, P, L, D), 'free_edges_mask': torch.full((B, P, L), 3.0)}


def _panel(preds, p, rows, at=None, b=0):
    at = range(len(rows)) if at is None else at
    for l, r in zip(at, rows):
        preds['outlines'][b, p, l] = torch.tensor(r, dtype=torch.float32)


def _nonfree(preds, edges, tags, logit=-3.0, b=0):
    L = preds['outlines'].shape[2]
    for e, t in zip(edges, tags):
        preds['free_edges_mask'][b, e // L, e % L] = logit
        preds['stitch_tags'][b, e // L, e % L] = torch.tensor(t, dtype=torch.float32)


def _pairs(want, b=0):
    n = int(want['num_stitches'][b])
    return [tuple(int(x) for x in want['stitches'][b, :, k]) for k in range(n)]


def test_every_edge_free_and_exactly_one_non_free(gpe):
    preds = _blank(2, 4)
    _panel(preds, 0, SQUARE)
    want = _check(gpe, preds, UNIT)
    assert want['num_stitches'][0] == 0 and want['first_invalid'][0] == -1 and want['num_panels'][0] == 1
    _nonfree(preds, [1], [(1, 1, 1)])
    assert _check(gpe, preds, UNIT)['num_stitches'][0] == 0


def test_odd_count_drops_the_largest_logit(gpe):
    preds = _blank(2, 4)
    _panel(preds, 0, SQUARE)
    _panel(preds, 1, SQUARE)
    _nonfree(preds, [0, 1, 5], [(0, 0, 0), (0.125, 0, 0), (4, 0, 0)])
    preds['free_edges_mask'][0, 0, 1] = -1.0                 # edge 1 is the closest to "free": it goes, though 0 - 1 is the nearest pair
    assert _pairs(_check(gpe, preds, UNIT)) == [(0, 5)]
    preds['free_edges_mask'][0, 0, 1] = 0.0                  # sigmoid exactly 0.5 rounds to 0: still non-free, still the one dropped
    assert _pairs(_check(gpe, preds, UNIT)) == [(0, 5)]


def test_equal_distances_take_the_smallest_row_and_column(gpe):
    preds = _blank(2, 4)
    _panel(preds, 0, SQUARE)
    _panel(preds, 1, SQUARE)
    # unit square: d(0,1) = d(0,2) = d(1,3) = d(2,3) = 1 exactly; the row-major first minimum is (0, 1), then (2, 3)
    _nonfree(preds, [0, 1, 2, 3], [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)])
    assert _pairs(_check(gpe, preds, UNIT)) == [(0, 1), (2, 3)]
    # eight points on a line with unit spacing across both panels: every step a tie with its neighbours
    _nonfree(preds, range(8), [(float(i), 0, 0) for i in range(8)])
    assert _pairs(_check(gpe, preds, UNIT)) == [(0, 1), (2, 3), (4, 5), (6, 7)]


def test_dropped_row_in_the_middle_and_empty_panel_between_real_ones(gpe):
    preds = _blank(3, 6)
    _panel(preds, 0, SQUARE, at=[0, 1, 3, 5])                # rows 2 and 4 stay padding
    _panel(preds, 1, SQUARE[:2])                             # two kept rows: empty
    _panel(preds, 2, SQUARE)
    want = _check(gpe, preds, UNIT)
    assert want['edge_slot'][0, 0].tolist() == [0, 1, 3, 5, -1, -1]
    assert want['new_panel_id'][0].tolist() == [0, -1, 1] and want['num_panels'][0] == 2
    assert want['num_edges'][0].tolist() == [4, 0, 4] and want['num_verts'][0].tolist() == [4, 0, 4]
    assert want['vertices'][0, 0, :4].tolist() == [[0, 0], [10, 0], [10, 10], [0, 10]]
    assert want['curved'][0, 0].tolist() == [0, 1, 0, 0, 0, 0] and want['curvature'][0, 0, 1].tolist() == [0.5, 0.25]


def test_open_loop_gets_the_extra_vertex(gpe):
    preds = _blank(1, 5)
    _panel(preds, 0, [(10, 0, 0, 0), (0, 10, 0, 0), (-10, 0, 0, 0), (0, -5, 0, 0)])
    want = _check(gpe, preds, UNIT)
    assert want['closed'][0, 0] == 0 and want['num_edges'][0, 0] == 4 and want['num_verts'][0, 0] == 5
    assert want['vertices'][0, 0, 4].tolist() == [0, 5]


def test_values_exactly_at_the_thresholds(gpe):
    up = lambda x: float(np.nextafter(np.float32(x), np.float32(np.inf)))      # noqa: E731
    preds = _blank(4, 5)
    # panel 0: a row of exactly +-1.5 is padding; its neighbour above 1.5 in one value is an edge
    _panel(preds, 0, [(10, 0, 0, 0), (1.5, -1.5, 1.5, -1.5), (0, 10, 0, 0), (-10, -10, 0, 0), (1.5, 1.5, 1.5, up(1.5))])
    # panel 1: the loop ends at exactly (3, -3): closed; panel 2: just past 3 in one coordinate: open
    _panel(preds, 1, [(10, 0, 0, 0), (0, 10, 0, 0), (-7, -13, 0, 0)])
    _panel(preds, 2, [(10, 0, 0, 0), (0, 10, 0, 0), (up(-7), -13, 0, 0)])
    # panel 3: curvature on either side of 0.01 in fp32
    below = float(np.nextafter(np.float32(0.01), np.float32(0)))
    c = float(np.float32(0.01))
    lo, hi = (below, c) if np.float64(np.float32(0.01)) > 0.01 else (c, up(0.01))
    _panel(preds, 3, [(10, 0, lo, -lo), (0, 10, hi, 0), (-10, -10, 0, -hi)])
    want = _check(gpe, preds, UNIT)
    assert want['edge_slot'][0, 0].tolist() == [0, 2, 3, 4, -1]
    assert want['closed'][0, :3].tolist() == [1, 1, 0] and want['num_verts'][0, 1:3].tolist() == [3, 4]
    assert want['curved'][0, 3, :3].tolist() == [0, 1, 1]
    # exactly 0.01 in fp64: the value 1 at a scale of 0.01 is the very double the bound is
    stats = copy.deepcopy(UNIT)
    stats['gt_scale']['outlines'] = [1, 1, 0.01, 0.01]
    preds = _blank(1, 3)
    _panel(preds, 0, [(10, 0, 1, -1), (0, 10, 1, up(1)), (-10, -10, 0, 0)])
    assert _check(gpe, preds, stats)['curved'][0, 0].tolist() == [0, 1, 0]


def test_nan_and_inf_in_outlines_logits_and_tags(gpe):
    nan, inf = float('nan'), float('inf')
    preds = _blank(4, 4)
    _panel(preds, 0, [(10, 0, 0, 0), (nan, 0, 0, 0), (0, 10, 0, 0), (-10, -10, 0, 0)])        # a NaN keeps its row
    _panel(preds, 1, [(10, 0, 0, 0), (0, inf, 0, 0), (-10, -10, nan, 0), (0, 0, 0, -inf)])    # so does an inf
    _panel(preds, 2, SQUARE)
    _panel(preds, 3, SQUARE)
    _nonfree(preds, [8, 9, 10, 11, 12, 13], [(0, 0, 0), (nan, 0, 0), (0.25, 0, 0), (inf, 1, 1), (5, 5, 5), (5, 5.5, 5)])
    preds['free_edges_mask'][0, 0, 0] = nan                  # NaN: free
    preds['free_edges_mask'][0, 0, 1] = inf                  # free
    preds['free_edges_mask'][0, 3, 0] = -inf                 # non-free
    want = _check(gpe, preds, UNIT)
    assert want['num_edges'][0].tolist() == [4, 4, 4, 4] and want['closed'][0].tolist() == [0, 0, 1, 1]
    assert np.isnan(want['vertices'][0, 0, 2]).any() and want['curved'][0, 1, 2:4].tolist() == [1, 1]
    assert _pairs(want) == [(8, 10), (12, 13)]               # the pairing stops with the NaN and inf tags left over


def test_stitches_naming_an_empty_panel_and_a_dropped_slot(gpe):
    preds = _blank(3, 5)
    _panel(preds, 0, SQUARE)                                 # slot 4 is padding
    _panel(preds, 2, SQUARE)
    # found in the order of their distances: (0, 10) fine, (4, 11) names the padding row 4, (6, 12) names the empty panel 1
    _nonfree(preds, [0, 10, 4, 11, 6, 12], [(0, 0, 0), (0.125, 0, 0), (3, 0, 0), (3.25, 0, 0), (6, 0, 0), (6.5, 0, 0)])
    want = _check(gpe, preds, UNIT)
    assert _pairs(want) == [(0, 10), (4, 11), (6, 12)]
    assert want['stitch_flags'][0, :4].tolist() == [0, 2, 3, 0] and want['first_invalid'][0] == 2
    dec = gpe.patterns.DecodedPatterns(gpe.ops.pattern_decode(_cuda(preds), UNIT))
    spec = dec.as_spec(0)
    assert spec['stitches'] == [[{'panel': 'panel_0', 'edge': 0}, {'panel': 'panel_2', 'edge': 0}],
                                [{'panel': 'panel_0', 'edge': 4}, {'panel': 'panel_2', 'edge': 1}]]      # the slot, as the reference
    with pytest.raises(ValueError, match='stitch 2 .*panel 1'):
        dec.as_spec(0, strict=True)


def test_given_stitches_with_padding_and_ids_out_of_range(gpe):
    preds = _blank(3, 5, B=2)
    for b in range(2):
        _panel(preds, 0, SQUARE, b=b)
        _panel(preds, 2, SQUARE, b=b)
    _nonfree(preds, [0, 1], [(0, 0, 0), (1, 0, 0)])          # the tags would pair (0, 1): the given stitches replace that
    st = torch.tensor([[[1, 0, 2, 0, 15, 3], [11, 0, 12, 0, 3, 10]],
                       [[0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]])
    want = _check(gpe, preds, UNIT, stitches=st)
    assert _pairs(want) == [(1, 11), (2, 12), (15, 3), (3, 10)] and want['stitches'].shape == (2, 2, 6)
    assert want['stitch_flags'][0].tolist() == [0, 0, 1, 0, 0, 0] and want['first_invalid'].tolist() == [2, -1]
    assert want['num_stitches'].tolist() == [4, 0]
    want = _check(gpe, preds, UNIT, stitches=st.int(), num_stitches=torch.tensor([3, 6]))
    assert _pairs(want) == [(1, 11), (2, 12)] and want['first_invalid'].tolist() == [-1, -1]
    with pytest.raises(RuntimeError, match='no CPU path'):
        gpe.ops.pattern_decode(_cuda(preds), UNIT, stitches=st)


def test_garment_with_no_valid_panel(gpe):
    preds = _blank(3, 4)
    _panel(preds, 1, SQUARE[:2])
    _nonfree(preds, [4, 5], [(0, 0, 0), (1, 0, 0)])
    want = _check(gpe, preds, UNIT)
    assert want['num_panels'][0] == 0 and (want['new_panel_id'] == -1).all() and (want['num_verts'] == 0).all()
    assert _pairs(want) == [(4, 5)] and want['stitch_flags'][0, 0] == 1 and want['first_invalid'][0] == 0
    spec = gpe.patterns.DecodedPatterns(gpe.ops.pattern_decode(_cuda(preds), UNIT)).as_spec(0)
    assert spec == {'panels': {}, 'panel_order': [], 'stitches': []}


def test_off_menu_shapes_raise_before_any_launch(gpe):
    with pytest.raises(ValueError, match='1025|1 <= P \\* L'):
        gpe.ops.pattern_decode(_cuda(_blank(25, 41)), UNIT)
    with pytest.raises(ValueError, match='tag width'):
        gpe.ops.pattern_decode(_cuda(_blank(2, 4, D=9)), UNIT)
    with pytest.raises(ValueError, match='1 <= P \\* L'):
        gpe.ops.tags_to_stitches(torch.zeros(1, 25, 41, 3, device='cuda'), torch.zeros(1, 25, 41, device='cuda'))
    with pytest.raises(ValueError, match='tag width'):
        gpe.ops.tags_to_stitches(torch.zeros(1, 2, 4, 9, device='cuda'), torch.zeros(1, 2, 4, device='cuda'))
    torch.cuda.synchronize()


# ---- the reference's recorded results --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', FIXTURES, ids=[os.path.basename(f)[15:-3] for f in FIXTURES])
def test_reference_patterns_through_as_spec(gpe, path):
    fx = torch.load(path, weights_only=False)
    dc = fx['data_config']
    _check(gpe, fx['preds'], dc['standardize'], dc['explicit_stitch_tags'], stitches=fx['stitches'])
    dec = gpe.patterns.DecodedPatterns(gpe.ops.pattern_decode(
        _cuda(fx['preds']), dc['standardize'], dc['explicit_stitch_tags'],
        stitches=None if fx['stitches'] is None else fx['stitches'].cuda()))
    for b, (pat, raised) in enumerate(zip(fx['patterns'], fx['raised'])):
        spec = dec.as_spec(b)
        for panel in spec['panels'].values():
            panel.pop('universal_translation')
        assert spec == pat, b
        assert raised == (int(dec.first_invalid[b]) >= 0)


# ---- the shared pairing code: ops.tags_to_stitches against the quality metrics -------------------------------------------------------
QUALITY = sorted(glob.glob(os.path.join(GOLDEN, 'quality_*.pt')))


@pytest.mark.parametrize('path', QUALITY, ids=[os.path.basename(f)[8:-3] for f in QUALITY])
def test_tags_to_stitches_implies_the_quality_metrics(gpe, path):
    fx = torch.load(path, weights_only=False)
    dc = fx['data_config']
    ops = gpe.ops
    preds, gt = _cuda(fx['preds']), _cuda(fx['gt_matched'])
    B, P, L = preds['outlines'].shape[:3]
    explicit = bool(dc['explicit_stitch_tags'])
    stats = dc['standardize']
    tags = preds['stitch_tags']
    if explicit:                                             # the kernel's fp32 product and sum, each rounded
        tags = tags * torch.tensor(stats['gt_scale']['stitch_tags'], device='cuda') + \
            torch.tensor(stats['gt_shift']['stitch_tags'], device='cuda')
    st, ns = ops.tags_to_stitches(tags, preds['free_edges_mask'])
    assert st.dtype == torch.int32 and st.shape == (B, 2, P * L // 2) and ns.shape == (B,)
    st, ns = st.cpu().numpy(), ns.cpu().numpy()
    # the pairs the fixture implies (its inputs keep the decision margin)
    margins = []
    t64 = tags.double().cpu().numpy().reshape(B, P * L, -1)
    lg = fx['preds']['free_edges_mask'].double().numpy().reshape(B, P * L)
    for b in range(B):
        want = R.tags_to_stitches(t64[b], lg[b], margins)
        assert [tuple(st[b, :, k]) for k in range(ns[b])] == want, b
        assert (st[b, :, ns[b]:] == 0).all()
    # precision and recall from those pairs, in the number types of the metric (csrc/gpe_quality.hip)
    qs = ops.quality_stats({'shift': stats['gt_shift']['outlines'], 'scale': stats['gt_scale']['outlines']},
                           tag_stats={'shift': stats['gt_shift']['stitch_tags'], 'scale': stats['gt_scale']['stitch_tags']}
                           if explicit else None)
    flags = ops.QM_STITCH | (ops.QM_TAG_STATS if explicit else 0)
    out, _ = ops.quality_metrics(flags, qs, B, P, L, stitch_tags=preds['stitch_tags'], free_logits=preds['free_edges_mask'],
                                 stitches=gt['stitches'], nums=gt['num_stitches'])
    out = out.cpu().numpy()
    gst, gn = fx['gt_matched']['stitches'].numpy(), fx['gt_matched']['num_stitches'].numpy().reshape(B)
    prec, rec = 0.0, np.float32(0)
    for b in range(B):
        pairs = {frozenset((int(st[b, 0, k]), int(st[b, 1, k]))) for k in range(ns[b])}
        truth = {frozenset((int(gst[b, 0, k]), int(gst[b, 1, k]))) for k in range(max(0, min(int(gn[b]), gst.shape[2])))}
        good = len(pairs & truth)
        prec += good / len(pairs) if pairs else 0.0
        rec = np.float32(rec + (np.float32(good) * (np.float32(1) / np.float32(gn[b])) if pairs and gn[b] else np.float32(0)))
    assert out[9] == np.float32(prec / B) and out[10] == np.float32(rec / np.float32(B)), (out[9:11], prec / B, rec / B)


# ---- the models ----------------------------------------------------------------------------------------------------------------------------
def _model(gpe, name):
    fx = torch.load(os.path.join(GOLDEN, name), weights_only=False)
    torch.manual_seed(fx['seed'])
    model = getattr(gpe.nets, fx['model'])(fx['data_config'], copy.deepcopy(fx['nn_config']), copy.deepcopy(fx['loss_config']))
    model.load_state_dict(fx['state_dict'])
    return fx, model.cuda().eval()


def _equal_dicts(a, b):
    assert tuple(a) == tuple(b)
    for k in a:
        _same(a[k], b[k].cpu().numpy(), k)


@pytest.mark.parametrize('name', ['full3d_small.pt', 'segment3d_small.pt'])
def test_predict_pattern_is_predict_then_decode(gpe, name):
    fx, model = _model(gpe, name)
    x = fx['features'].cuda()
    dc = fx['data_config']
    torch.manual_seed(5)                                     # the decoders draw their start states on the CPU generator
    dec = model.predict_pattern(x, dc)
    torch.manual_seed(5)
    preds = model.predict(x)
    assert not preds['outlines'].is_contiguous() and not preds['free_edges_mask'].is_contiguous()       # strided views
    want = gpe.ops.pattern_decode(preds, dc['standardize'], dc['explicit_stitch_tags'])
    _equal_dicts(dec.tensors, want)
    # contiguous copies of the views: the same bits
    dense = {k: preds[k].contiguous().clone() for k in ('outlines', 'rotations', 'translations', 'stitch_tags', 'free_edges_mask')}
    _equal_dicts(gpe.ops.pattern_decode(dense, dc['standardize'], dc['explicit_stitch_tags']), want)
    # and the restatement on what the model predicted (untrained weights: whatever panels come out; no margin for the stitches)
    got = R.restate({k: v.cpu() for k, v in dense.items()}, dc['standardize'], dc['explicit_stitch_tags'])[0]
    for k in ('num_edges', 'edge_slot', 'num_verts', 'closed', 'new_panel_id', 'num_panels', 'vertices', 'curvature', 'rotations',
              'translations', 'curved'):
        _same(want[k], np.ascontiguousarray(got[k]), k)
    given = torch.tensor([[[1, 0, 30], [20, 0, 400]]] * x.shape[0], device='cuda')
    dec = model.predict_pattern(x, dc, stitches=given)
    assert dec.stitches.shape == (x.shape[0], 2, 3) and dec.num_stitches.tolist() == [2] * x.shape[0]
    assert (dec.stitch_flags[:, 1] & 1).all()                # edge id 400 >= 23 * 14
    assert isinstance(dec.as_spec(0), dict)


def _capture(side, fn):
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        out = fn()
    return cg, out


def test_decode_inside_a_stream_capture(gpe):
    """a host read inside a capture is an error of the runtime; the replay equals the eager call bit for bit"""
    fx = torch.load(FIXTURES[0], weights_only=False)
    dc = fx['data_config']
    preds = _cuda(fx['preds'])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = gpe.ops.pattern_decode(preds, dc['standardize'])
        eager_st = gpe.ops.tags_to_stitches(preds['stitch_tags'], preds['free_edges_mask'])
        side.synchronize()
        cg, (again, st) = _capture(side, lambda: (gpe.ops.pattern_decode(preds, dc['standardize']),
                                                  gpe.ops.tags_to_stitches(preds['stitch_tags'], preds['free_edges_mask'])))
        for t in list(again.values()) + list(st):
            t.fill_(-7)
        cg.replay()
    torch.cuda.synchronize()
    _equal_dicts(again, eager)
    assert torch.equal(st[0], eager_st[0]) and torch.equal(st[1], eager_st[1])
    assert torch.equal(eager['stitches'], eager_st[0]) and torch.equal(eager['num_stitches'], eager_st[1])


def test_predict_pattern_inside_a_stream_capture(gpe):
    """the whole of predict_pattern captured, the start states of the decoders fed through graph.HostDrawn as a captured training step
    feeds them: the replay equals the eager call bit for bit"""
    fx, model = _model(gpe, 'full3d_small.pt')
    x = fx['features'].cuda()
    dc = fx['data_config']
    from gpe_amd import graph
    host = graph.HostDrawn(x.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    gpe.ops.HOST_DRAWN = host
    try:
        with torch.cuda.stream(side):
            for _ in range(2):                               # warm-up: workspaces, packs, the host-drawn tensors get their buffers
                torch.manual_seed(5)
                host.begin_step()
                eager = model.predict_pattern(x, dc)
            eager = {k: v.clone() for k, v in eager.tensors.items()}
            side.synchronize()
            host.cursor, host.capturing = 0, True
            cg, dec = _capture(side, lambda: model.predict_pattern(x, dc))
            host.capturing = False
            for t in dec.tensors.values():
                t.fill_(-7)
            torch.manual_seed(5)
            host.begin_step()
            cg.replay()
        torch.cuda.synchronize()
    finally:
        gpe.ops.HOST_DRAWN = None
    _equal_dicts(dec.tensors, eager)

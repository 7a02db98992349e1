#!/usr/bin/env python3
"""Generates tests/golden/pattern_place_small.pt: what the REFERENCE'S OWN code makes of a batch of predictions between its two
prediction stages — NNSewingPattern.pattern_from_tensors / panel_from_numeric / _edge_dict with real `panel_translations`
(nn/data/pattern_converter.py:118-187, 228-288, 510-515), then _3D_edges_per_panel and all_edge_pairs (:458-499, 517-552), called
unbound and unmodified in the order of Garment3DPatternFullDataset._pred_to_pattern (nn/data/datasets.py:731-767).

The stand-in object supplies what those functions read (`name`, `properties`, `pattern`, `panel_classifier = None`, a no-op
_invalidate_all_values) and the three things the reference takes from its external `pattern` package, written from their
definitions (INTEGRATION.md lists the reference lines that pin each):
    _point_in_3D(p2, R, t)               R . (p2.x, p2.y, 0) + t
    rotation_tools.euler_xyz_to_R(a)     scipy Rotation.from_euler('xyz', a, degrees=True).as_matrix()   (set on the stub module here)
    _panel_universal_transtation(name)   (3D point, 2D point) of the bounding-box side midpoint — top, bottom, right, left — whose
                                         3D image has the largest y, the first of them on a tie (argmax): universal_point below, the
                                         ONE rule that rests on the package's published definition alone
plus panel_order().

Only runnable where the reference checkout exists (like scripts/make_pattern_decode_golden.py, whose sys.path set-up on the read-only
stubs it shares).  The fixture holds data only: configs, inputs, per garment the resulting `pattern` dict, the per-panel edge rows
(fp64), the all_edge_pairs rows (fp32), the rotation matrices, the midpoint chosen and its margin.  Seeded: a re-run writes the
same file.

Inputs: quality_restate.make_batch, B = 6, P = 23, L = 14, with the faults of pattern_decode_restate.plant_fault; redrawn until
  - every decision margin of the decode is >= quality_restate.MARGIN (as for the decode fixtures),
  - every panel's top-midpoint margin (largest 3D y minus the second largest, tests/pattern_place_restate.py) is >= 1e-3, so that
    fp64 on host and device decide alike,
  - each of the four midpoints is chosen at least once,
  - the six garments have at most MAX_PAIR_ROWS edge pairs in all (the fixture's size).

    python scripts/make_pattern_place_golden.py [REFERENCE_DIR]
"""
import copy
import json
import os
import sys

import numpy as np
import torch
from scipy.spatial.transform import Rotation

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('GPE_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(REPO, 'oracle', 'refgen', 'stubs'), os.path.join(REF, 'nn'), REPO, os.path.join(REPO, 'tests')]

from data.datasets import Garment3DPatternFullDataset  # noqa: E402  (the reference's class)
from data.pattern_converter import NNSewingPattern, InvalidPatternDefError  # noqa: E402  (the reference's class)
from pattern import rotation as rotation_stub  # noqa: E402
import quality_restate  # noqa: E402
import pattern_decode_restate as D  # noqa: E402
import pattern_place_restate as R  # noqa: E402

torch.set_num_threads(1)
LSTM = 'models/baseline/lstm_stitch_tags.yaml'
SHIPPED = json.load(open(os.path.join(REPO, 'tests', 'golden', 'shipped_yaml_configs.json')))
PLACE_MARGIN = 1e-3
MAX_PAIR_ROWS = 4000

rotation_stub.euler_xyz_to_R = lambda angles: Rotation.from_euler('xyz', angles, degrees=True).as_matrix()


def universal_point(vertices, rot_matrix, point_in_3d):
    """The universal point of a panel by the `pattern` package's published definition: the four midpoints of the sides of the 2D
    bounding box of the vertices, in the order top (mid_x, max_y), bottom (mid_x, min_y), right (max_x, mid_y), left (min_x, mid_y);
    the one whose 3D image has the largest y, the first on a tie.  -> (number, 3D point, 2D point)"""
    lo, hi = vertices.min(axis=0), vertices.max(axis=0)
    mid = (lo + hi) / 2
    mids = np.array([[mid[0], hi[1]], [mid[0], lo[1]], [hi[0], mid[1]], [lo[0], mid[1]]])
    mids_3d = np.stack([point_in_3d(m) for m in mids])
    k = int(np.argmax(mids_3d[:, 1]))
    return k, mids_3d[k], mids[k]


class StandIn:
    """what the reference's functions read from a pattern, and the functions themselves, unmodified"""
    pattern_from_tensors = NNSewingPattern.pattern_from_tensors
    panel_from_numeric = NNSewingPattern.panel_from_numeric
    _edge_dict = NNSewingPattern._edge_dict
    _3D_edges_per_panel = NNSewingPattern._3D_edges_per_panel
    all_edge_pairs = NNSewingPattern.all_edge_pairs
    _stitches_as_set = NNSewingPattern._stitches_as_set

    def __init__(self, name):
        self.name = name
        self.properties = {}
        self.pattern = {}
        self.panel_classifier = None
        self.chosen = {}

    def _invalidate_all_values(self):
        pass

    def panel_order(self, force_update=False, pad_to_len=None):
        return self.pattern['panel_order']

    def _point_in_3D(self, point, rotation, translation):
        return rotation.dot(np.append(np.asarray(point, np.float64)[:2], 0.0)) + np.asarray(translation, np.float64)

    def _panel_universal_transtation(self, panel_name):
        panel = self.pattern['panels'][panel_name]
        rot_matrix = rotation_stub.euler_xyz_to_R(panel['rotation'])
        translation = panel.get('translation', [0.0, 0.0, 0.0])         # the template's, until panel_from_numeric sets the panel's
        k, point_3d, point_2d = universal_point(np.array(panel['vertices']), rot_matrix,
                                                lambda m: self._point_in_3D(m, rot_matrix, translation))
        self.chosen[panel_name] = k
        return point_3d, point_2d


def reference_garment(pred, data_config, name):
    """Garment3DPatternFullDataset._pred_to_pattern's steps on one garment with the placement, then the classifier's input"""
    prediction = {k: v.clone() for k, v in pred.items()}
    gt_shifts, gt_scales = data_config['standardize']['gt_shift'], data_config['standardize']['gt_scale']
    for key in gt_shifts:
        if key == 'stitch_tags' and not data_config['explicit_stitch_tags']:
            continue
        prediction[key] = prediction[key].cpu().numpy() * gt_scales[key] + gt_shifts[key]
    stitches = Garment3DPatternFullDataset.tags_to_stitches(                                 # ---- the reference, unmodified ----
        prediction['stitch_tags'], prediction['free_edges_mask'])
    obj, raised = StandIn(name), False
    try:
        obj.pattern_from_tensors(prediction['outlines'], panel_rotations=prediction['rotations'],
                                 panel_translations=prediction['translations'], stitches=stitches, padded=True)      # ---- unmodified ----
    except InvalidPatternDefError:
        raised = True
    assert prediction['outlines'].dtype == np.float64 and prediction['translations'].dtype == np.float64
    edge_rows = obj._3D_edges_per_panel()                                                    # ---- the reference, unmodified ----
    pair_rows, mapping, _ = obj.all_edge_pairs()                                             # ---- the reference, unmodified ----
    assert pair_rows.dtype == torch.float32
    order = obj.pattern['panel_order']
    return {'pattern': obj.pattern, 'raised': raised,
            'edge_rows': {n: np.stack(edge_rows[n]).astype(np.float64) for n in order},
            'pair_rows': pair_rows.contiguous(), 'pair_first': mapping[0], 'pair_last': mapping[-1],
            'rot_matrix': {n: rotation_stub.euler_xyz_to_R(obj.pattern['panels'][n]['rotation']) for n in order},
            'top_mid': {n: obj.chosen[n] for n in order}}


def main():
    B, seed = 6, 8101
    kinds = ['ok', 'pad_real', 'open', 'extra', 'ok', 'open']
    faults = ['none', 'mid_drop', 'empty_stitch', 'two_rows', 'dropped_stitch', 'mid_drop']
    data_config = copy.deepcopy(SHIPPED[LSTM]['dataset'])
    data_config['max_pattern_len'] = 23                 # nn/data/datasets.py:377-379 with panel_classes_condenced.json
    data_config['explicit_stitch_tags'] = False
    P, L, S = data_config['max_pattern_len'], data_config['max_panel_len'], data_config['max_num_stitches']
    assert (P, L) == (23, 14)
    stats = data_config['standardize']
    rng = np.random.default_rng(seed)
    for attempt in range(5000):
        preds, _ = quality_restate.make_batch(rng, B, P, L, S, data_config, kinds)
        for b in range(B):
            D.plant_fault(rng, preds, b, faults[b], stats)
        decoded, decode_margin = D.restate(preds, stats, False)
        ne = decoded['num_edges'].astype(np.int64)
        pair_rows = sum(int(ne[b].sum() ** 2 - (ne[b] ** 2).sum()) // 2 for b in range(B))
        if pair_rows > MAX_PAIR_ROWS or decode_margin < quality_restate.MARGIN:
            continue
        placed, margins = R.restate(decoded)
        if margins.min() >= PLACE_MARGIN and set(placed['top_mid'][ne > 0].tolist()) == {0, 1, 2, 3}:
            break
    else:
        raise RuntimeError('no draw with the margins, all four midpoints and <= %d pair rows' % MAX_PAIR_ROWS)
    garments = [reference_garment({k: v[b] for k, v in preds.items()}, data_config, 'garment_%d' % b) for b in range(B)]
    # the margins are asserted on the REFERENCE'S choice too: the restatement's midpoint is the stand-in's, panel by panel
    for b, g in enumerate(garments):
        slots = [p for p in range(P) if ne[b, p] > 0]
        assert [g['top_mid']['panel_%d' % p] for p in slots] == placed['top_mid'][b, slots].tolist()
        assert len(g['pair_rows']) == int(ne[b].sum() ** 2 - (ne[b] ** 2).sum()) // 2
    assert float(margins.min()) >= PLACE_MARGIN
    hit = np.bincount(placed['top_mid'][ne > 0], minlength=4)
    assert (hit > 0).all()
    fx = {'data_config': data_config, 'seed': seed, 'draws': attempt + 1, 'decode_margin': decode_margin,
          'margins': torch.from_numpy(margins), 'preds': preds, 'garments': garments}
    out = os.path.join(REPO, 'tests', 'golden', 'pattern_place_small.pt')
    torch.save(fx, out)
    print('pattern_place_small B=%d draws=%d place margin=%.2e decode margin=%.2e midpoints top/bottom/right/left=%s panels=%s '
          'pair rows=%s raised=%s  %.0f KB'
          % (B, attempt + 1, margins.min(), decode_margin, hit.tolist(), [len(g['pattern']['panel_order']) for g in garments],
             [len(g['pair_rows']) for g in garments], ''.join('x' if g['raised'] else '.' for g in garments),
             os.path.getsize(out) / 1024))


if __name__ == '__main__':
    main()

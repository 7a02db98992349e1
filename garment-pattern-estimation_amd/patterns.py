"""Decoded predictions as sewing-pattern specifications: the host end of ops.pattern_decode (csrc/gpe_pattern_decode.hip) and
ops.pattern_place (csrc/gpe_pattern_place.hip).

The kernels leave a batch of decoded patterns in device tensors; `DecodedPatterns.as_spec(i)` is the one place that reads a garment
back and builds the dict the reference leaves in `pattern.pattern` (NNSewingPattern.pattern_from_tensors / panel_from_numeric,
nn/data/pattern_converter.py:118-187, 228-271), and `to_json` writes it.

The predicted translation is that of the panel's universal point (the bounding-box side midpoint that lies highest in 3D).  It is
always passed through as `universal_translation`.  `DecodedPatterns.place()` turns it into the translation of the panel's origin on
the device (the reference's key `translation`, :281-288) and builds the 3D edges the stitch classifier reads (`edges3d`,
_3D_edges_per_panel :517-552); the definitions it rests on are listed in INTEGRATION.md."""
import json


class DecodedPatterns:
    """the tensors of ops.pattern_decode for a batch (ops.PATTERN_DECODE_KEYS; layouts: include/gpe_hip.h gpe_pattern_decode) and,
    after place(), those of ops.pattern_place (ops.PATTERN_PLACE_KEYS; include/gpe_hip_place.h) in `placed`; after
    model.predict_garment also the edge-pair classifier's `pair_stitches`, `num_pair_stitches`, `pair_scores` in `pairs`.
    Attribute access reaches them by name (`d.vertices`, `d.stitches`, `d.edges3d`, ...); nothing here touches the host but
    as_spec / to_json."""

    def __init__(self, tensors):
        self.tensors = dict(tensors)
        self.placed = None
        self.pairs = None
        self.batch_size, self.max_pattern_len, self.max_panel_len = self.tensors['edge_slot'].shape

    def __getattr__(self, name):
        d = self.__dict__
        for group in (d.get('tensors'), d.get('placed'), d.get('pairs')):
            if group is not None and name in group:
                return group[name]
        raise AttributeError(name)

    def __len__(self):
        return self.batch_size

    def place(self):
        """the panels placed in 3D on the device (ops.pattern_place, one launch, once): `rot_matrix`, `translation`, `top_mid`,
        `vertices3d`, `edges3d`, `place_flags` become attributes and as_spec carries the reference's key 'translation'.  -> self"""
        if self.placed is None:
            from . import ops
            self.placed = ops.pattern_place(self.tensors)
        return self

    def label_stitches(self):
        """the stitches this pattern carries as labels for the edge-pair classifier: -> (stitches int32 [B, 2, S], n_labels int32
        [B]), both on the device, no host read.  n_labels = first_invalid where a stitch names a missing panel (the stitches before
        it, as _pred_to_pattern keeps them, nn/data/datasets.py:756-765), num_stitches otherwise.  The ids are panel * L + row — what
        ops.stitch_pairs_eval takes as gt_stitches, which reads `id % L` as the index in the panel's compact edge list: the
        reference compares the stored edge id with that index in the same way and does not notice a dropped row (stitch_flags bit
        1, include/gpe_hip.h)."""
        import torch
        first, nums = self.tensors['first_invalid'], self.tensors['num_stitches']
        return self.tensors['stitches'], torch.where(first >= 0, first, nums)

    def attach_pair_stitches(self, out):
        """the edge-pair classifier's answer (ops.stitch_pairs' dict) on this batch's edges3d, for as_spec(stitches='classifier')"""
        self.pairs = {'pair_stitches': out['stitches'], 'num_pair_stitches': out['num_stitches'], 'pair_scores': out['scores']}
        return self

    def as_spec(self, i, panel_names=None, strict=False, stitches='tags'):
        """garment i as {'panels': {name: {'vertices', 'edges', 'rotation', 'universal_translation'}}, 'panel_order', 'stitches'}.
        panel_names: one name per panel slot (default 'panel_<slot>', the reference's names without a panel classifier).
        rotation: Euler xyz angles in degrees of the predicted quaternion, formed as the reference forms them.
        strict=False gives what _pred_to_pattern (nn/data/datasets.py:756-765) leaves after it caught InvalidPatternDefError: the
        stitches before the first one that names a missing panel.  strict=True raises ValueError for that stitch instead.
        After place() every panel also has the reference's 'translation' (of the panel's origin); a panel whose quaternion could not
        be normalised (place_flags) raises ValueError, where the reference's scipy call raises.
        stitches='tags' (default) lists the stitches paired from the predicted tags (or given to the decode), as the reference's
        pattern_from_tensors leaves them; 'classifier' lists those of the edge-pair classifier (model.predict_garment) in the shape of
        the reference's _stitch_entry, [{'panel', 'edge', 'score'}, {...}] — there `edge` is the index of the edge in the panel's
        edge list (the classifier reads the compact edge rows), not the decoder's row slot."""
        from scipy.spatial.transform import Rotation
        if stitches not in ('tags', 'classifier'):
            raise ValueError("stitches must be 'tags' or 'classifier' (got %r)" % (stitches,))
        if stitches == 'classifier' and self.pairs is None:
            raise ValueError("stitches='classifier' needs the edge-pair classifier's answer: model.predict_garment attaches it")
        if not 0 <= i < self.batch_size:
            raise IndexError('garment %d of a batch of %d' % (i, self.batch_size))
        t = {k: v[i].cpu().numpy() for k, v in self.tensors.items()}               # the read-back
        placed = None if self.placed is None else {k: self.placed[k][i].cpu().numpy() for k in ('translation', 'place_flags')}
        P, L = self.max_pattern_len, self.max_panel_len
        names = ['panel_' + str(p) for p in range(P)] if panel_names is None else list(panel_names)
        if len(names) != P:
            raise ValueError('%d panel names for %d panel slots' % (len(names), P))
        panels, order = {}, []
        for p in range(P):
            if t['new_panel_id'][p] < 0:
                continue
            n, nv = int(t['num_edges'][p]), int(t['num_verts'][p])
            edges = []
            for k in range(n):
                edge = {'endpoints': [k, k + 1 if k + 1 < nv else 0]}
                if t['curved'][p, k]:
                    edge['curvature'] = t['curvature'][p, k].tolist()
                edges.append(edge)
            if placed is not None and placed['place_flags'][p]:
                raise ValueError('garment %d: the rotation of panel %d (%s) is no quaternion that can be normalised: %s'
                                 % (i, p, names[p], t['rotations'][p].tolist()))
            panels[names[p]] = {'vertices': t['vertices'][p, :nv].tolist(), 'edges': edges,
                                'rotation': Rotation.from_quat(t['rotations'][p]).as_euler('xyz', degrees=True).tolist(),
                                'universal_translation': t['translations'][p].tolist()}
            if placed is not None:
                panels[names[p]]['translation'] = placed['translation'][p].tolist()
            order.append(names[p])
        if stitches == 'classifier':
            st, ns, sc = (self.pairs[k][i].cpu().numpy() for k in ('pair_stitches', 'num_pair_stitches', 'pair_scores'))
            found = [[{'panel': names[int(e) // L], 'edge': int(e) % L, 'score': float(sc[k])} for e in st[:, k]]
                     for k in range(int(ns))]
            return {'panels': panels, 'panel_order': order, 'stitches': found}
        ns, first = int(t['num_stitches']), int(t['first_invalid'])
        if first >= 0:
            if strict:
                a, b = int(t['stitches'][0, first]), int(t['stitches'][1, first])
                bad = [e // L for e in (a, b) if not 0 <= e // L < P or t['new_panel_id'][e // L] < 0]
                raise ValueError('garment %d: stitch %d (edges %d, %d) refers to non-existing panel %d' % (i, first, a, b, bad[0]))
            ns = first
        found = [[{'panel': names[int(e) // L], 'edge': int(e) % L} for e in t['stitches'][:, k]] for k in range(ns)]
        return {'panels': panels, 'panel_order': order, 'stitches': found}

    def to_json(self, i, path, **kwargs):
        """as_spec(i, **kwargs) written to `path` as JSON"""
        with open(path, 'w') as f:
            json.dump(self.as_spec(i, **kwargs), f, indent=2)

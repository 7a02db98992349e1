"""Decoded predictions as sewing-pattern specifications: the host end of ops.pattern_decode (csrc/gpe_pattern_decode.hip).

The kernel leaves a batch of decoded patterns in device tensors; `DecodedPatterns.as_spec(i)` is the one place that reads a garment
back and builds the dict the reference leaves in `pattern.pattern` (NNSewingPattern.pattern_from_tensors / panel_from_numeric,
nn/data/pattern_converter.py:118-187, 228-271), and `to_json` writes it.

Not converted: the predicted translation is that of the panel's top mid-point (the reference's "universal" translation); turning it
into the translation of the panel's origin needs the reference's `pattern` package (_panel_universal_transtation, _point_in_3D).  It is
passed through as `universal_translation`, deliberately not under the reference's key `translation`."""
import json


class DecodedPatterns:
    """the tensors of ops.pattern_decode for a batch (ops.PATTERN_DECODE_KEYS; layouts: include/gpe_hip.h gpe_pattern_decode).
    Attribute access reaches them by name (`d.vertices`, `d.stitches`, ...); nothing here touches the host but as_spec / to_json."""

    def __init__(self, tensors):
        self.tensors = dict(tensors)
        self.batch_size, self.max_pattern_len, self.max_panel_len = self.tensors['edge_slot'].shape

    def __getattr__(self, name):
        try:
            return self.__dict__['tensors'][name]
        except KeyError:
            raise AttributeError(name) from None

    def __len__(self):
        return self.batch_size

    def as_spec(self, i, panel_names=None, strict=False):
        """garment i as {'panels': {name: {'vertices', 'edges', 'rotation', 'universal_translation'}}, 'panel_order', 'stitches'}.
        panel_names: one name per panel slot (default 'panel_<slot>', the reference's names without a panel classifier).
        rotation: Euler xyz angles in degrees of the predicted quaternion, formed as the reference forms them.
        strict=False gives what _pred_to_pattern (nn/data/datasets.py:756-765) leaves after it caught InvalidPatternDefError: the
        stitches before the first one that names a missing panel.  strict=True raises ValueError for that stitch instead."""
        from scipy.spatial.transform import Rotation
        if not 0 <= i < self.batch_size:
            raise IndexError('garment %d of a batch of %d' % (i, self.batch_size))
        t = {k: v[i].cpu().numpy() for k, v in self.tensors.items()}               # the read-back
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
            panels[names[p]] = {'vertices': t['vertices'][p, :nv].tolist(), 'edges': edges,
                                'rotation': Rotation.from_quat(t['rotations'][p]).as_euler('xyz', degrees=True).tolist(),
                                'universal_translation': t['translations'][p].tolist()}
            order.append(names[p])
        ns, first = int(t['num_stitches']), int(t['first_invalid'])
        if first >= 0:
            if strict:
                a, b = int(t['stitches'][0, first]), int(t['stitches'][1, first])
                bad = [e // L for e in (a, b) if not 0 <= e // L < P or t['new_panel_id'][e // L] < 0]
                raise ValueError('garment %d: stitch %d (edges %d, %d) refers to non-existing panel %d' % (i, first, a, b, bad[0]))
            ns = first
        stitches = [[{'panel': names[int(e) // L], 'edge': int(e) % L} for e in t['stitches'][:, k]] for k in range(ns)]
        return {'panels': panels, 'panel_order': order, 'stitches': stitches}

    def to_json(self, i, path, **kwargs):
        """as_spec(i, **kwargs) written to `path` as JSON"""
        with open(path, 'w') as f:
            json.dump(self.as_spec(i, **kwargs), f, indent=2)

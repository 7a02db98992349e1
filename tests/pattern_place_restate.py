"""The panels of a decoded prediction placed in 3D (include/gpe_hip_place.h gpe_pattern_place; the reference's
NNSewingPattern._3D_edges_per_panel and the inverse of its universal translation, nn/data/pattern_converter.py:517-552, 281-288)
restated from the definition in plain fp64 numpy, one garment and one panel at a time — the yardstick of
tests/test_pattern_place_host.py and tests/test_gpu_pattern_place.py, the margin check of scripts/make_pattern_place_golden.py and
the per-garment host loop scripts/pattern_place_bench.py times.

`restate(decoded)` takes the tensors of ops.pattern_decode (arrays or tensors: num_edges, num_verts, vertices, curvature, curved,
rotations, translations) and returns the output tensors of ops.pattern_place as numpy arrays plus the per-panel margin of the one
decision in it: the largest 3D height of a bounding-box side midpoint minus the second largest (inf for an empty panel).  A panel
whose margin is far above fp64 rounding is decided alike by every fp64 evaluation order."""
import numpy as np

KEYS = ('rot_matrix', 'translation', 'top_mid', 'vertices3d', 'edges3d', 'place_flags')
BAD_QUAT = 1


def _np(t):
    if hasattr(t, 'detach'):
        t = t.detach().cpu().numpy()
    return np.asarray(t)


def quat_matrix(q):
    """(x, y, z, w), any non-zero length -> (R [3, 3] of the normalised quaternion as scipy's as_matrix forms it, flag); a zero or
    non-finite norm gives the identity and BAD_QUAT"""
    q = np.asarray(q, np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        nrm = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    if not nrm > 0.0 or np.isinf(nrm):
        return np.eye(3), BAD_QUAT
    x, y, z, w = q / nrm
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    return np.array([[x2 - y2 - z2 + w2, 2.0 * (xy - zw), 2.0 * (xz + yw)],
                     [2.0 * (xy + zw), -x2 + y2 - z2 + w2, 2.0 * (yz - xw)],
                     [2.0 * (xz - yw), 2.0 * (yz + xw), -x2 - y2 + z2 + w2]]), 0


def side_midpoints(verts):
    """the four midpoints of the sides of the 2D bounding box of `verts` [nv, 2], in the order top, bottom, right, left"""
    lo, hi = verts.min(0), verts.max(0)
    cx, cy = (lo[0] + hi[0]) / 2.0, (lo[1] + hi[1]) / 2.0
    return np.array([[cx, hi[1]], [cx, lo[1]], [hi[0], cy], [lo[0], cy]])


def top_mid(R, verts):
    """The universal point of a panel (_panel_universal_transtation of the reference's `pattern` package, by its published
    definition): the bounding-box side midpoint that lies highest in 3D, the first of them on a tie (argmax).  The 3D height of a
    midpoint m is R[1, 0] m.x + R[1, 1] m.y; the translation moves all four alike.  -> (number, the 2D point, margin)"""
    mids = side_midpoints(verts)
    y3 = R[1, 0] * mids[:, 0] + R[1, 1] * mids[:, 1]
    k = int(np.argmax(y3))
    top2 = np.sort(y3)[::-1]
    return k, mids[k], float(top2[0] - top2[1])


def place_panel(verts, curv, curved, quat, universal):
    """one non-empty panel: verts [nv, 2], curv [n, 2], curved [n], quat [4], universal [3] -> dict of its outputs and the margin"""
    n, nv = len(curv), len(verts)
    R, flag = quat_matrix(quat)
    k, mid, margin = top_mid(R, verts)
    t = np.asarray(universal, np.float64) - (R[:, 0] * mid[0] + R[:, 1] * mid[1])
    v3 = (R[:, 0][None, :] * verts[:, 0:1] + R[:, 1][None, :] * verts[:, 1:2]) + t[None, :]
    rows = np.zeros((n, 8), np.float32)
    for e in range(n):
        end = e + 1 if e + 1 < nv else 0
        c = curv[e] if curved[e] else (0.0, 0.0)
        with np.errstate(over='ignore'):
            rows[e] = np.concatenate([v3[e], v3[end], c]).astype(np.float32)
    return dict(R=R, flag=flag, top=k, t=t, v3=v3, rows=rows), margin


def restate(decoded):
    """-> ({name: array} with the names and layouts of ops.pattern_place, margins [B, P])"""
    d = {k: _np(decoded[k]) for k in ('num_edges', 'num_verts', 'vertices', 'curvature', 'curved', 'rotations', 'translations')}
    B, P = d['num_edges'].shape
    L = d['curved'].shape[2]
    o = {'rot_matrix': np.zeros((B, P, 3, 3)), 'translation': np.zeros((B, P, 3)), 'top_mid': np.full((B, P), -1, np.int32),
         'vertices3d': np.zeros((B, P, L + 1, 3)), 'edges3d': np.zeros((B, P, L, 8), np.float32),
         'place_flags': np.zeros((B, P), np.int32)}
    margins = np.full((B, P), np.inf)
    for b in range(B):
        for p in range(P):
            n, nv = int(d['num_edges'][b, p]), int(d['num_verts'][b, p])
            if n <= 0 or nv <= 0:
                continue
            r, margins[b, p] = place_panel(d['vertices'][b, p, :nv], d['curvature'][b, p, :n], d['curved'][b, p, :n],
                                           d['rotations'][b, p], d['translations'][b, p])
            o['rot_matrix'][b, p], o['translation'][b, p], o['top_mid'][b, p] = r['R'], r['t'], r['top']
            o['vertices3d'][b, p, :nv], o['edges3d'][b, p, :n], o['place_flags'][b, p] = r['v3'], r['rows'], r['flag']
    return o, margins


def host_loop(decoded):
    """the restatement without its margins' caller: what scripts/pattern_place_bench.py times as the per-garment host loop"""
    return restate(decoded)[0]

"""Host restatement of csrc/gpe_mesh_sample.hip: the point clouds and segmentation labels of include/gpe_hip.h
(gpe_mesh_points_sample) in numpy — Philox4x32-10 from stitch_sample_restate, the integer face thresholds, every decision
returned, the float32 arithmetic as the kernel does it (every product and sum rounded on its own), the Box-Muller noise in
float64, and the two nearest-neighbour passes.  The yardstick of the bit-exact device tests (tests/test_gpu_mesh_sample.py); its
own distribution is held against the analytic one (area-proportional faces, uniform in the triangle, standard normal noise) in
tests/test_mesh_sample_host.py.

    thresholds(verts, faces)        uint32 [F] of one garment
    draw(...)                       faces, integer barycentrics and float32 points of one slot
    normals(...)                    the float64 standard normals of one slot
    snap(points, verts)             nearest vertex of every point, float32, the lower index winning
    relabel(points, raw)            the stitch-point pass -> labels, how many fell back to 0
    sample_batch(...)               a call of the entry point
    twelve_faces()                  the twelve-face mesh both test files draw from
"""
import numpy as np

from stitch_sample_restate import words, chi2_quantile  # noqa: F401  (chi2_quantile: for the tests)

F32 = np.float32
FACE, NOISE = 8, 9
TOP = 1 << 31
ONE = 1 << 24
K = F32(2.0 ** -24)


def thresholds(verts, faces):
    """T[f] = floor(2^31 C_f / C_total), C the sequential float64 cumulative sum of 0.5 |(B - A) x (C - A)| of the fp32 vertices;
    2^31 from the last face of positive area onwards; zeros when there is none"""
    v = np.asarray(verts, dtype=F32).astype(np.float64)
    out = np.zeros(len(faces), dtype=np.uint32)
    total, cum, last = 0.0, [], -1
    for i, (a, b, c) in enumerate(np.asarray(faces, dtype=np.int64)):
        e1, e2 = v[b] - v[a], v[c] - v[a]
        cx, cy, cz = e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]
        area = 0.5 * np.sqrt(cx * cx + cy * cy + cz * cz)
        if area > 0:
            last = i
        total = total + area
        cum.append(total)
    if last < 0:
        return out
    for i, c in enumerate(cum):
        out[i] = TOP if i >= last else int(np.floor(2.0 ** 31 * (c / total)))
    return out


def draw(verts, faces, T, b, N, seed, drawn):
    """slot b on one garment -> dict face int [N], iu, iv int [N] (after the reflection), bary fp32 [N, 3] = (b0, b1, b2),
    points fp32 [N, 3] = (b0 A + b1 B) + b2 C"""
    verts, faces = np.asarray(verts, dtype=F32), np.asarray(faces, dtype=np.int64)
    w = words(FACE, np.arange(N), b, seed, drawn)
    t = (w[:, 0] >> np.uint32(1)).astype(np.int64)
    face = np.searchsorted(np.asarray(T, dtype=np.int64), t, side='right')          # the first f with T[f] > t
    iu, iv = (w[:, 1] >> np.uint32(8)).astype(np.int64), (w[:, 2] >> np.uint32(8)).astype(np.int64)
    over = iu + iv > ONE
    iu, iv = np.where(over, ONE - iu, iu), np.where(over, ONE - iv, iv)
    b1, b2, b0 = iu.astype(F32) * K, iv.astype(F32) * K, (ONE - iu - iv).astype(F32) * K
    A, B, C = verts[faces[face, 0]], verts[faces[face, 1]], verts[faces[face, 2]]
    p = (b0[:, None] * A + b1[:, None] * B) + b2[:, None] * C
    assert p.dtype == F32
    return {'face': face, 'iu': iu, 'iv': iv, 'bary': np.stack([b0, b1, b2], axis=1), 'points': p}


def normals(b, N, seed, drawn):
    """float64 [N, 3]: Box-Muller on the words of kind 9 — (0, 1) -> x (cosine) and y (sine), (2, 3) -> z (cosine)"""
    w = words(NOISE, np.arange(N), b, seed, drawn) >> np.uint32(8)
    u1a, u2a = (w[:, 0].astype(np.float64) + 1.0) * 2.0 ** -24, w[:, 1].astype(np.float64) * 2.0 ** -24
    u1b, u2b = (w[:, 2].astype(np.float64) + 1.0) * 2.0 ** -24, w[:, 3].astype(np.float64) * 2.0 ** -24
    ra, rb = np.sqrt(-2.0 * np.log(u1a)), np.sqrt(-2.0 * np.log(u1b))
    return np.stack([ra * np.cos(2.0 * np.pi * u2a), ra * np.sin(2.0 * np.pi * u2a), rb * np.cos(2.0 * np.pi * u2b)], axis=1)


def distances(points, others):
    """fp32 [N, M]: d = (dx dx + dy dy) + dz dz, every operation rounded to float32"""
    p, o = np.asarray(points, dtype=F32), np.asarray(others, dtype=F32)
    dx, dy, dz = o[None, :, 0] - p[:, None, 0], o[None, :, 1] - p[:, None, 1], o[None, :, 2] - p[:, None, 2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == F32
    return d


def snap(points, verts):
    """the nearest vertex of every point: the lexicographic minimum of (d, vertex)"""
    return np.argmin(distances(points, verts), axis=1)       # argmin returns the first of equal minima


def relabel(points, raw):
    """a point labelled -1 takes the label of the nearest point whose raw label is >= 0 (the lower point wins a tie); none: 0.
    -> (labels int64 [N], how many fell back)"""
    raw = np.asarray(raw, dtype=np.int64)
    out = raw.copy()
    open_ = np.nonzero(raw < 0)[0]
    keep = np.nonzero(raw >= 0)[0]
    if not len(open_):
        return out, 0
    if not len(keep):
        out[open_] = 0
        return out, len(open_)
    points = np.asarray(points, dtype=F32)
    out[open_] = raw[keep[np.argmin(distances(points[open_], points[keep]), axis=1)]]
    return out, 0


def labels_of(points, verts, vert_labels):
    """both passes on given (noisy, unstandardised) points -> (segmentation int64 [N], fallback count)"""
    return relabel(points, np.asarray(vert_labels, dtype=np.int64)[snap(points, verts)])


def standardized(points, shift, scale):
    if shift is None:
        return points
    return (points - np.asarray(shift, dtype=F32)) / np.asarray(scale, dtype=F32)


def sample_batch(meshes, index, N, seed, drawn, noise_w=0.0, shift=None, scale=None):
    """meshes [(verts, faces, labels)], index [B] -> features fp32 [B, N, 3], segmentation int64 [B, N], status int32 [B] and the
    decisions of every slot (None for a slot with a negative status).  With noise the points are p + w z with z rounded from float64:
    the device's differ in the last bits (tests compare those under a derived bar and the labels on the device's own points)."""
    B = len(index)
    feats, seg, status, decisions = np.zeros((B, N, 3), dtype=F32), np.zeros((B, N), dtype=np.int64), np.zeros(B, dtype=np.int32), []
    cache = {}
    for b, g in enumerate(index):
        if not 0 <= g < len(meshes):
            status[b] = -2
            decisions.append(None)
            continue
        verts, faces, labels = meshes[g]
        if g not in cache:
            cache[g] = thresholds(verts, faces)
        T = cache[g]
        if not len(T) or T[-1] != TOP:
            status[b] = -1
            decisions.append(None)
            continue
        d = draw(verts, faces, T, b, N, seed, drawn)
        p = d['points']
        if noise_w:
            d['clean'], d['z'] = p, normals(b, N, seed, drawn)
            p = p + F32(noise_w) * d['z'].astype(F32)
            d['points'] = p
        seg[b], status[b] = labels_of(p, verts, labels)
        feats[b] = standardized(p, shift, scale)
        decisions.append(d)
    return feats, seg, status, decisions


def twelve_faces():
    """twelve triangles in the plane z = 0.25 x whose areas run from 1 to 50 in shuffled order, one of them degenerate (face 7:
    three collinear vertices)"""
    areas = [9.0, 1.0, 50.0, 17.0, 3.0, 28.0, 41.0, 0.0, 2.0, 35.0, 12.0, 6.0]
    verts, faces = [], []
    for i, a in enumerate(areas):
        x0 = 12.0 * i
        if a:
            tri = [(x0, 0.0), (x0 + 10.0, 0.0), (x0 + 3.0, 2.0 * a / 10.0)]
        else:
            tri = [(x0, 0.0), (x0 + 5.0, 1.0), (x0 + 10.0, 2.0)]
        faces.append([len(verts) + k for k in range(3)])
        verts += [(x, y, 0.25 * x) for x, y in tri]
    verts = np.asarray(verts, dtype=np.float32) / np.float32(64.0)
    return verts, np.asarray(faces, dtype=np.int64), np.arange(len(verts), dtype=np.int64) // 3

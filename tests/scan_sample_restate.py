"""Host restatement of csrc/gpe_scan_sample.hip (include/gpe_hip_scan.h), integer- and float32-exact, in numpy on top of
stitch_sample_restate.words: the yardstick of the bit-exact device tests (tests/test_gpu_scan_sample.py); its own distribution is held
against np.random.permutation(n)[:N] in tests/test_scan_sample_host.py.

The draw rule.  Slot b of a call draws cloud g = index[b].  Point i of that cloud gets the 64-bit key (w0 << 32) | w1 of
words(kind 13, item i, slot b, seed, draw).  The points are ordered by (key, i) ascending; output row r < N is the point of rank r,
rank r mod n when the cloud has n < N points (status N - n, else 0).  n = 0: status -1; index outside the set: status -2; such a slot
is zeros with picked -1.  features = (p - shift) / scale in float32, subtract then divide (p itself without statistics).

The labels.  For every point of every cloud named by a valid slot: the row of the lexicographic minimum of (d, row) over the slot's N
drawn points, d = (dx dx + dy dy) + dz dz, every operation rounded to float32 on its own; the label is the first maximum over P of
that row's weights.  If two slots name the same cloud the higher slot's labels stand.

    keys(n, b, seed, draw)   the uint64 keys of a cloud of n points
    order(n, b, seed, draw)  the points by (key, i)
    sample_batch(...)        a call of gpe_scan_sample
    labels(...)              a call of gpe_scan_labels
"""
import numpy as np

import stitch_sample_restate as S

KIND = 13
F32 = np.float32


def keys(n, b, seed, draw):
    w = S.words(KIND, np.arange(n, dtype=np.int64), b, seed, draw)
    return (w[:, 0].astype(np.uint64) << np.uint64(32)) | w[:, 1].astype(np.uint64)


def order(n, b, seed, draw):
    """the indices of a cloud of n points sorted by (key, i) ascending"""
    return np.lexsort((np.arange(n), keys(n, b, seed, draw)))     # the last key is the primary one


def picked_of(n, N, b, seed, draw):
    """-> (picked int32 [N], status)"""
    if n == 0:
        return np.full(N, -1, dtype=np.int32), -1
    o = order(n, b, seed, draw)
    return o[np.arange(N) % n if n < N else np.arange(N)].astype(np.int32), max(N - n, 0)


def standardize(p, shift, scale):
    p = np.asarray(p, dtype=F32)
    if shift is None:
        return p
    return ((p - np.asarray(shift, dtype=F32)) / np.asarray(scale, dtype=F32)).astype(F32)


def sample_batch(clouds, index, N, seed, draw, shift=None, scale=None):
    """-> features float32 [B, N, 3], picked int32 [B, N], status int32 [B]"""
    B = len(index)
    feats, picked, status = np.zeros((B, N, 3), dtype=F32), np.full((B, N), -1, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b, g in enumerate(index):
        if not 0 <= g < len(clouds):
            status[b] = -2
            continue
        cloud = np.asarray(clouds[g], dtype=F32).reshape(-1, 3)
        picked[b], status[b] = picked_of(len(cloud), N, b, seed, draw)
        if len(cloud):
            feats[b] = standardize(cloud[picked[b]], shift, scale)
    return feats, picked, status


def nearest_rows(points, drawn):
    """points float32 [n, 3], drawn float32 [N, 3] -> the row of the lexicographic minimum of (d, row) for every point; float32
    operations one by one"""
    points, drawn = np.asarray(points, dtype=F32), np.asarray(drawn, dtype=F32)
    d = [(drawn[None, :, a] - points[:, None, a]).astype(F32) for a in range(3)]
    sq = [(x * x).astype(F32) for x in d]
    dist = ((sq[0] + sq[1]).astype(F32) + sq[2]).astype(F32)
    return np.argmin(dist, axis=1)                                 # the first minimum: the lower row


def labels(clouds, index, picked, att, out=None):
    """att float32 [B, N, P] -> int32 [T] over the concatenated clouds; rows nobody writes keep `out` (or -1)"""
    sizes = [len(np.asarray(c).reshape(-1, 3)) for c in clouds]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    res = np.full(off[-1], -1, dtype=np.int32) if out is None else np.array(out, dtype=np.int32)
    for b, g in enumerate(index):                                  # ascending: a higher slot overwrites a lower one
        if not 0 <= g < len(clouds) or sizes[g] == 0:
            continue
        cloud = np.asarray(clouds[g], dtype=F32).reshape(-1, 3)
        rows = nearest_rows(cloud, cloud[picked[b]])
        res[off[g]:off[g + 1]] = np.argmax(np.asarray(att[b], dtype=F32)[rows], axis=1)      # the first maximum
    return res

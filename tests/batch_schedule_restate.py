"""Host restatement of gpe_batch_schedule_draw (csrc/gpe_epoch_feed.hip, contract in include/gpe_hip_feed.h), integer-exact, in numpy
with the Philox4x32-10 of tests/stitch_sample_restate.py.  The yardstick of the bit-exact device tests
(tests/test_gpu_epoch_feed.py); its own distribution is held against counts recorded from the reference's BalancedBatchSampler
(nn/data/utils.py:16-92; scripts/make_batch_schedule_golden.py) in tests/test_epoch_feed_host.py.

    quotas(sizes, B)            the reference's per-type batch lengths, in its own expression
    draw(...)                   one epoch -> table, batch_len and the class of every slot
    tally(...) / statistics     the three statistics the recorded counts hold, and their two-sample chi-square comparison
"""
import numpy as np

import stitch_sample_restate as S

ORDER, FILL, SLOT = 10, 11, 12


def quotas(sizes, B):
    """int((len_c / G) * B) in double (nn/data/utils.py:48)"""
    G = sum(sizes)
    return [int((n / G) * B) for n in sizes]


def rows_of(G, B, drop_last):
    return G // B + (1 if (not drop_last and G % B) else 0)


def words(kind, item, b, seed, epoch):
    """the block of one decision, item and b broadcast against each other: counter (item | kind << 28, b << 8, epoch lo, epoch hi), key
    (seed lo, seed hi) — stitch_sample_restate.words with an array of slots"""
    item, b = np.broadcast_arrays(np.asarray(item, dtype=np.int64), np.asarray(b, dtype=np.int64))
    ctr = np.empty(item.shape + (4,), dtype=np.uint32)
    ctr[..., 0] = (item | (kind << 28)) & 0xFFFFFFFF
    ctr[..., 1] = (b << 8) & 0xFFFFFFFF
    ctr[..., 2] = int(epoch) & 0xFFFFFFFF
    ctr[..., 3] = (int(epoch) >> 32) & 0xFFFFFFFF
    key = np.empty(item.shape + (2,), dtype=np.uint32)
    key[..., 0] = int(seed) & 0xFFFFFFFF
    key[..., 1] = (int(seed) >> 32) & 0xFFFFFFFF
    return S.philox4x32(ctr, key)


def _key64(w):
    return (w[..., 0].astype(np.uint64) << np.uint64(32)) | w[..., 1].astype(np.uint64)


def _ranks(keys):
    """position of every entry in the order ascending by (key, index)"""
    order = np.lexsort((np.arange(len(keys)), keys))
    rank = np.empty(len(keys), dtype=np.int64)
    rank[order] = np.arange(len(keys))
    return rank


def draw(class_lists, quota, B, drop_last, seed, epoch):
    """class_lists: the garment ids of every class, in class order -> dict
      table      int32 [rows, B], a kept remainder padded with -1
      batch_len  int32 [rows]
      classes    int [rows, B]: the class of the garment in every slot (-1 for padding)
      pre        the table before the slot shuffle"""
    sizes = [len(l) for l in class_lists]
    C, G = len(sizes), sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ids = np.concatenate([np.asarray(l, dtype=np.int64).reshape(-1) for l in class_lists]) if G else np.zeros(0, dtype=np.int64)
    nfull, rows = G // B, rows_of(G, B, drop_last)
    # order inside a class: ascending by (key, position)
    keys = _key64(words(ORDER, np.arange(G), 0, seed, epoch))
    queue = []
    for c in range(C):
        r = _ranks(keys[off[c]:off[c + 1]])
        q = np.empty(sizes[c], dtype=np.int64)
        q[r] = ids[off[c]:off[c + 1]]
        queue.append(q)
    taken = [0] * C
    pre = np.full((rows, B), -1, dtype=np.int64)
    cls = np.full((rows, B), -1, dtype=np.int64)
    batch_len = np.zeros(rows, dtype=np.int32)
    for t in range(rows):
        n = 0
        if t == nfull:                                         # the kept remainder: every garment left, in class order
            for c in range(C):
                while taken[c] < sizes[c]:
                    pre[t, n], cls[t, n] = queue[c][taken[c]], c
                    taken[c] += 1
                    n += 1
        else:
            for c in range(C):
                for _ in range(min(int(quota[c]), sizes[c] - taken[c])):
                    pre[t, n], cls[t, n] = queue[c][taken[c]], c
                    taken[c] += 1
                    n += 1
            fill = words(FILL, t, np.arange(B), seed, epoch)[:, 0] if n < B else None   # one block per slot; word 0 decides
            for j in range(n, B):
                alive = [c for c in range(C) if taken[c] < sizes[c]]
                c = alive[int(S.below(fill[j], len(alive)))]
                pre[t, j], cls[t, j] = queue[c][taken[c]], c
                taken[c] += 1
            n = B
        batch_len[t] = n
    table, classes = np.full((rows, B), -1, dtype=np.int64), np.full((rows, B), -1, dtype=np.int64)
    for t in range(rows):
        n = int(batch_len[t])
        skeys = _key64(words(SLOT, t, np.arange(n), seed, epoch))
        r = _ranks(skeys)
        table[t, r], classes[t, r] = pre[t, :n], cls[t, :n]
    return {'table': table.astype(np.int32), 'batch_len': batch_len, 'classes': classes, 'pre': pre.astype(np.int32)}


# ---- the statistics the reference's recorded counts hold -----------------------------------------------------------------------------

def tally(batches, class_of, watched, B, rows):
    """the counts of one epoch (batches: lists of garment ids, full rows only) added to nothing: -> (comp, batch_of, slot_of)
      comp      {(t, class counts of batch t): 1}
      batch_of  [(class index of a watched garment, batch it landed in, or `rows` when it was dropped)]
      slot_of   [(class index, slot inside its batch)] for the watched garments that landed"""
    C = max(class_of.values()) + 1
    comp, batch_of, slot_of = [], [], []
    where = {}
    for t, b in enumerate(batches):
        counts = [0] * C
        for s, g in enumerate(b):
            counts[class_of[g]] += 1
            where[g] = (t, s)
        comp.append((t,) + tuple(counts))
    for i, g in enumerate(watched):
        t, s = where.get(g, (rows, None))
        batch_of.append((i, t))
        if s is not None:
            slot_of.append((i, s))
    return comp, batch_of, slot_of


class Counts:
    """N epochs' counts of the three statistics (what tests/golden/batch_schedule_small.pt holds per setting)"""

    def __init__(self, C, B, rows):
        self.N, self.C, self.B, self.rows = 0, C, B, rows
        self.comp = {}                                           # (t, counts...) -> epochs
        self.batch_of = np.zeros((C, rows + 1), dtype=np.int64)  # [watched garment of class c, batch or dropped]
        self.slot_of = np.zeros((C, B), dtype=np.int64)          # [watched garment of class c, slot]

    def add(self, batches, class_of, watched):
        comp, batch_of, slot_of = tally(batches, class_of, watched, self.B, self.rows)
        for k in comp:
            self.comp[k] = self.comp.get(k, 0) + 1
        for i, t in batch_of:
            self.batch_of[i, t] += 1
        for i, s in slot_of:
            self.slot_of[i, s] += 1
        self.N += 1

    def comp_rows(self):
        """the composition counts as an int64 [n, 1 + C + 1] array: t, the class counts, epochs"""
        return np.asarray([k + (v,) for k, v in sorted(self.comp.items())], dtype=np.int64).reshape(-1, self.C + 2)

    @classmethod
    def from_recorded(cls, rec):
        out = cls(int(rec['C']), int(rec['B']), int(rec['rows']))
        out.N = int(rec['N'])
        out.comp = {tuple(int(v) for v in r[:-1]): int(r[-1]) for r in np.asarray(rec['comp'])}
        out.batch_of, out.slot_of = np.asarray(rec['batch_of']), np.asarray(rec['slot_of'])
        return out


def two_sample(a, b):
    """Two-sample chi-square of two count vectors over the same cells -> (statistic, degrees of freedom).  Cells whose expected count
    under the pooled estimate falls below 5 in either sample are pooled into one cell; with K = sqrt(sum b / sum a) the statistic is
    sum (K a_i - b_i / K)^2 / (a_i + b_i), chi-square with cells - 1 degrees when both samples come from one distribution."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    na, nb = a.sum(), b.sum()
    pooled = (a + b) / (na + nb)
    small = pooled * min(na, nb) < 5
    if small.any():
        a, b = np.concatenate([a[~small], [a[small].sum()]]), np.concatenate([b[~small], [b[small].sum()]])
    on = (a + b) > 0
    a, b = a[on], b[on]
    K = np.sqrt(nb / na)
    return float(((K * a - b / K) ** 2 / (a + b)).sum()), int(len(a) - 1)


def statistics(x, y):
    """the comparisons of two Counts of one setting -> {name: (statistic, degrees of freedom)}: the composition of every batch t, the
    batch of the watched garment of every class, its slot.  One table per batch / per class, each with its own degrees: the tables of
    one epoch depend on each other, so their statistics are not added up."""
    out = {}
    for t in range(x.rows):
        cells = sorted({k for k in x.comp if k[0] == t} | {k for k in y.comp if k[0] == t})
        if cells:
            out['composition of batch %d' % t] = two_sample([x.comp.get(k, 0) for k in cells], [y.comp.get(k, 0) for k in cells])
    for c in range(x.C):
        out['batch of class %d' % c] = two_sample(x.batch_of[c], y.batch_of[c])
        out['slot of class %d' % c] = two_sample(x.slot_of[c], y.slot_of[c])
    return {k: v for k, v in out.items() if v[1] >= 1}

"""Host restatement of csrc/gpe_stitch_sample.hip, integer-exact: Philox4x32-10 and the pair sampler of include/gpe_hip.h
(gpe_stitch_sample), in numpy.  The yardstick of the bit-exact device tests (tests/test_gpu_stitch_sample.py); its own distribution
is held against the analytic model of NNSewingPattern.stitches_as_3D_pairs (nn/data/pattern_converter.py:321-409) and the
reference's recorded counts in tests/test_stitch_sample_host.py.

    sample(...)        one batch slot -> rows, labels, status and the decisions taken
    sample_batch(...)  a call of the entry point
    model(...)         the analytic distribution of the reference's draw for one garment
"""
import numpy as np

U32 = np.uint32
U64 = np.uint64
M0, M1 = U64(0xD2511F53), U64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = U64(0xFFFFFFFF)
FLIP, SWAP, DUP, PAIR, KEY = range(5)
ATTEMPTS = 64
SHUFFLE_PAIRS, SHUFFLE_ORDER = 1, 2


def philox4x32(ctr, key, rounds=10):
    """ctr uint32 [..., 4], key uint32 [..., 2] -> uint32 [..., 4] (Salmon et al., SC'11; Random123's philox4x32)"""
    c = [np.asarray(ctr)[..., i].astype(U64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(U64) for i in range(2)]
    for r in range(rounds):
        p0, p1 = M0 * c[0], M1 * c[2]                      # < 2^64: exact in uint64
        c = [(p1 >> U64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> U64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + U64(W0)) & MASK, (k[1] + U64(W1)) & MASK]
    return np.stack(c, axis=-1).astype(U32)


def words(kind, item, b, seed, draw, attempt=0):
    """the block of one decision: counter (item | kind << 28, attempt | b << 8, draw lo, draw hi), key (seed lo, seed hi)"""
    item, attempt = np.broadcast_arrays(np.asarray(item, dtype=np.int64), np.asarray(attempt, dtype=np.int64))
    ctr = np.empty(item.shape + (4,), dtype=U32)
    ctr[..., 0] = (item | (kind << 28)) & 0xFFFFFFFF
    ctr[..., 1] = (attempt | (int(b) << 8)) & 0xFFFFFFFF
    ctr[..., 2] = int(draw) & 0xFFFFFFFF
    ctr[..., 3] = (int(draw) >> 32) & 0xFFFFFFFF
    key = np.empty(item.shape + (2,), dtype=U32)
    key[..., 0] = int(seed) & 0xFFFFFFFF
    key[..., 1] = (int(seed) >> 32) & 0xFFFFFFFF
    return philox4x32(ctr, key)


def below(word, n):
    """an integer in [0, n): (uint64(word) * n) >> 32"""
    return ((np.asarray(word).astype(U64) * np.asarray(n).astype(U64)) >> U64(32)).astype(np.int64)


def counts_of(num_edges, L):
    return np.clip(np.asarray(num_edges, dtype=np.int64), 0, L)


def valid_stitches(num_edges, L, gt, gt_num):
    """gt int [2, S], gt_num -> [(e_a, e_b)] of the entries below the count whose ids lie in 0 .. E - 1 and name present edges"""
    cnt = counts_of(num_edges, L)
    E = len(cnt) * L
    gt = np.asarray(gt, dtype=np.int64).reshape(2, -1)
    out = []
    for s in range(int(np.clip(gt_num, 0, gt.shape[1]))):
        a, b = int(gt[0, s]), int(gt[1, s])
        if 0 <= a < E and 0 <= b < E and a % L < cnt[a // L] and b % L < cnt[b // L]:
            out.append((a, b))
    return out


def flipped(edge):
    """an edge [start xyz | end xyz | cx cy] reversed, in the edge's own dtype"""
    e = np.asarray(edge)
    one = e.dtype.type(1)
    out = e.copy()
    out[0:3], out[3:6] = e[3:6], e[0:3]
    out[6] = one - e[6] if e[6] != 0 else e.dtype.type(0)
    out[7] = -e[7]
    return out


def sample(edges, num_edges, gt, gt_num, b, n_stitched, n_non, flags, shift, scale, seed, draw):
    """one batch slot on garment (edges [P, L, Fe] fp32, num_edges [P], gt [2, S], gt_num)
    -> dict rows fp32 [R, 2 Fe], labels bool [R], status int and the decisions: flips {edge: bit}, swaps [S_v], choices [dups],
    pairs [(e_a, e_b) or None per non-stitched row], attempts [per non-stitched row], perm [R] (position of pre-shuffle row r),
    desc [(e_a, e_b) or None per pre-shuffle row]"""
    edges = np.asarray(edges, dtype=np.float32)
    P, L, Fe = edges.shape
    E, R = P * L, n_stitched + n_non
    cnt = counts_of(num_edges, L)
    present = [p for p in range(P) if cnt[p] > 0]
    shift, scale = np.asarray(shift, dtype=np.float32), np.asarray(scale, dtype=np.float32)
    out = {'rows': np.zeros((R, 2 * Fe), dtype=np.float32), 'labels': np.zeros(R, dtype=bool), 'status': 0, 'flips': {}, 'swaps': [],
           'choices': [], 'pairs': [], 'attempts': [], 'perm': np.arange(R), 'desc': [None] * R}
    st = valid_stitches(num_edges, L, gt, gt_num)
    Sv = len(st)
    if Sv > n_stitched:
        out['status'] = -1
        return out
    ids = np.asarray([p * L + l for p in present for l in range(cnt[p])], dtype=np.int64)
    if flags & SHUFFLE_PAIRS and len(ids):
        bits = words(FLIP, ids, b, seed, draw)[:, 0] >> U32(31)
        out['flips'] = {int(e): int(f) for e, f in zip(ids, bits)}
    else:
        out['flips'] = {int(e): 0 for e in ids}
    desc = []
    if Sv:
        sw = (words(SWAP, np.arange(Sv), b, seed, draw)[:, 0] >> U32(31)).astype(int) if flags & SHUFFLE_PAIRS else np.zeros(Sv, dtype=int)
        out['swaps'] = sw.tolist()
        desc = [(bb, a) if s else (a, bb) for (a, bb), s in zip(st, sw)]
        if n_stitched > Sv:
            ch = below(words(DUP, np.arange(Sv, n_stitched), b, seed, draw)[:, 0], Sv)
            out['choices'] = ch.tolist()
            desc += [desc[c] for c in ch]
    n_pos = len(desc)
    n_neg = R - n_pos
    stitched = set(st) | {(bb, a) for a, bb in st}
    pairs, attempts = [None] * n_neg, [ATTEMPTS] * n_neg
    pending = np.arange(n_neg)
    if present:
        pan, pc = np.asarray(present), cnt[np.asarray(present)]
        for a in range(ATTEMPTS):
            if not len(pending):
                break
            w = words(PAIR, pending, b, seed, draw, attempt=a)
            ia, ib = below(w[:, 0], len(pan)), below(w[:, 2], len(pan))
            ea = pan[ia] * L + below(w[:, 1], pc[ia])
            eb = pan[ib] * L + below(w[:, 3], pc[ib])
            keep = []
            for j, x, y in zip(pending, ea, eb):
                if x != y and (int(x), int(y)) not in stitched:
                    pairs[j], attempts[j] = (int(x), int(y)), a
                else:
                    keep.append(j)
            pending = np.asarray(keep, dtype=np.int64)
    out['pairs'], out['attempts'] = pairs, attempts           # attempts: rejected ones in front of the accepted one; 64 = gave up
    out['status'] = sum(1 for q in pairs if q is None)
    desc += pairs
    out['desc'] = desc
    if flags & SHUFFLE_ORDER:
        keys = words(KEY, np.arange(R), b, seed, draw)[:, 0]
        order = np.lexsort((np.arange(R), keys))              # by (key, row)
        perm = np.empty(R, dtype=np.int64)
        perm[order] = np.arange(R)
        out['perm'] = perm
    flat = edges.reshape(E, Fe)
    for r, d in enumerate(desc):
        pos = out['perm'][r]
        out['labels'][pos] = r < n_pos
        if d is None:
            continue
        halves = [flipped(flat[e]) if out['flips'][e] else flat[e] for e in d]
        out['rows'][pos] = (np.concatenate(halves) - shift) / scale
    return out


def sample_batch(edges3d, num_edges, gt_stitches, gt_num_stitches, index, n_stitched, n_non, flags, shift, scale, seed, draw):
    """a call of gpe_stitch_sample -> rows fp32 [B, R, 2 Fe], labels bool [B, R], status int32 [B], [decisions per slot]"""
    G = len(edges3d)
    Fe, R = np.asarray(edges3d[0]).shape[-1], n_stitched + n_non
    rows = np.zeros((len(index), R, 2 * Fe), dtype=np.float32)
    labels, status, dec = np.zeros((len(index), R), dtype=bool), np.zeros(len(index), dtype=np.int32), []
    for b, g in enumerate(index):
        if not 0 <= g < G:
            status[b] = -2
            dec.append(None)
            continue
        d = sample(edges3d[g], num_edges[g], gt_stitches[g], gt_num_stitches[g], b, n_stitched, n_non, flags, shift, scale, seed, draw)
        rows[b], labels[b], status[b] = d['rows'], d['labels'], d['status']
        dec.append(d)
    return rows, labels, status, dec


# ---- the analytic model of the reference's draw ---------------------------------------------------------------------------------

def model(num_edges, L, stitches):
    """-> {(e_a, e_b): probability} of an accepted non-stitched ordered pair: panels uniform among the present ones, edges uniform
    inside, conditioned on not being a self pair or a stitch in either orientation: proportional to 1 / (n_p n_q)"""
    cnt = counts_of(num_edges, L)
    ids = [(p * L + l, int(cnt[p])) for p in range(len(cnt)) for l in range(cnt[p])]
    bad = set(stitches) | {(b, a) for a, b in stitches}
    w = {(a, b): 1.0 / (na * nb) for a, na in ids for b, nb in ids if a != b and (a, b) not in bad}
    z = sum(w.values())
    return {k: v / z for k, v in w.items()}


def chi2_quantile(df, p):
    """Wilson-Hilferty: the p quantile of chi-square with df degrees of freedom"""
    z = _norm_quantile(p)
    return df * (1.0 - 2.0 / (9.0 * df) + z * np.sqrt(2.0 / (9.0 * df))) ** 3


def _norm_quantile(p):
    """Acklam's rational approximation of the standard normal quantile (|relative error| < 1.2e-9), central and upper branch"""
    a = [-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02, -3.066479806614716e+01,
         2.506628277459239e+00]
    b = [-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01, -1.328068155288572e+01]
    c = [-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00, 4.374664141464968e+00,
         2.938163982698783e+00]
    d = [7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00]
    if p < 0.5:
        return -_norm_quantile(1.0 - p)
    if p <= 0.97575:
        q = p - 0.5
        r = q * q
        return (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q / \
               (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0)
    q = np.sqrt(-2.0 * np.log(1.0 - p))
    return -(((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0)


def chi2_statistics(rec, num_edges, L, stitches, n_stitched, n_non):
    """the five statistics of recorded counts `rec` against the analytic model -> {name: (statistic, degrees of freedom)}
      flips   per edge seen in a call, Bernoulli 1/2: sum (flips - seen / 2)^2 / (seen / 4), one degree per edge
      swaps   per stitch and call, Bernoulli 1/2
      choices (n_stitched - S_v) N draws, uniform on the S_v stitches
      pairs   n_non N independent draws from model()
      perm    N uniform permutations of R rows summed: the Pearson statistic of the R x R count matrix, times (R - 1) / R, is
              chi-square with (R - 1)^2 degrees (the covariance of a centred permutation matrix is 1 / (R - 1) times the projection on
              the matrices with zero row and column sums, whose dimension that is)"""
    N = int(rec['N'])
    Sv, R = len(stitches), n_stitched + n_non
    seen, fl = np.asarray(rec['flip_seen'], dtype=float), np.asarray(rec['flip_count'], dtype=float)
    on = seen > 0
    out = {'flips': (float((((fl - seen / 2) ** 2)[on] / (seen[on] / 4)).sum()), int(on.sum()))}
    sw = np.asarray(rec['swap_count'], dtype=float)
    out['swaps'] = (float(((sw - N / 2) ** 2 / (N / 4)).sum()), Sv)
    ch = np.asarray(rec['choice_hist'], dtype=float)
    exp = (n_stitched - Sv) * N / Sv
    out['choices'] = (float(((ch - exp) ** 2 / exp).sum()), Sv - 1)
    m = model(num_edges, L, stitches)
    got = {(int(a), int(b)): int(c) for a, b, c in np.asarray(rec['pair_counts']).reshape(-1, 3)}
    assert set(got) <= set(m), 'a non-stitched pair outside the model: %s' % sorted(set(got) - set(m))[:3]
    out['pairs'] = (float(sum((got.get(k, 0) - n_non * N * q) ** 2 / (n_non * N * q) for k, q in m.items())), len(m) - 1)
    pm = np.asarray(rec['perm_counts'], dtype=float)
    out['perm'] = (float(((pm - N / R) ** 2 / (N / R)).sum() * (R - 1) / R), (R - 1) ** 2)
    return out


def tally(decisions, E, stitches, n_stitched, n_non):
    """the counts scripts/make_stitch_sample_golden.py records of the reference, from the restatement's decisions"""
    Sv, R = len(stitches), n_stitched + n_non
    rec = {'N': len(decisions), 'flip_seen': np.zeros(E, dtype=np.int64), 'flip_count': np.zeros(E, dtype=np.int64),
           'swap_count': np.zeros(Sv, dtype=np.int64), 'choice_hist': np.zeros(Sv, dtype=np.int64),
           'perm_counts': np.zeros((R, R), dtype=np.int64), 'flip_inconsistent': 0}
    pairs = {}
    for d in decisions:
        used = {e for q in d['desc'] if q is not None for e in q}
        for e in used:
            rec['flip_seen'][e] += 1
            rec['flip_count'][e] += d['flips'][e]
        rec['swap_count'] += np.asarray(d['swaps'], dtype=np.int64)
        for c in d['choices']:
            rec['choice_hist'][c] += 1
        for q in d['pairs']:
            pairs[q] = pairs.get(q, 0) + 1
        rec['perm_counts'][np.arange(R), d['perm']] += 1
    rec['pair_counts'] = np.asarray([(a, b, c) for (a, b), c in sorted(pairs.items())], dtype=np.int64)
    return rec


# ---- what both test files share: the six garments as one resident set, and reading rows back ---------------------------------------

TAGS = ('small', 'gaps', 'none', 'one', 'claimed', 'full')


def resident_set(golden_dir, tags=TAGS, S=None):
    """the stitch_pairs_<tag>.pt garments padded to one [G, P, L, 8] set (slots past the counts hold 1e3: they must be ignored),
    ground truth from `plants`, each in its own orientation, padded to S entries with an id that must not be read
    -> dict edges fp32 [G, P, L, 8], num_edges int64 [G, P], gt int64 [G, 2, S], gt_num int64 [G], shift, scale (lists), tags"""
    import os
    import torch
    fxs = [torch.load(os.path.join(golden_dir, 'stitch_pairs_%s.pt' % t), weights_only=False) for t in tags]
    P, L = max(f['edges'].shape[0] for f in fxs), max(f['edges'].shape[1] for f in fxs)
    S = max(len(f['plants']) for f in fxs) + 3 if S is None else S
    G = len(fxs)
    edges = np.full((G, P, L, 8), 1e3, dtype=np.float32)
    ne, gt, num = np.zeros((G, P), dtype=np.int64), np.full((G, 2, S), 10 ** 6, dtype=np.int64), np.zeros(G, dtype=np.int64)
    for g, f in enumerate(fxs):
        n = f['num_edges'].numpy()
        ne[g, :len(n)] = n
        for p in range(len(n)):
            edges[g, p, :n[p]] = f['edges'].numpy()[p, :n[p]]
        for s, (a, b) in enumerate(f['plants']):
            gt[g, 0, s], gt[g, 1, s] = a[0] * L + a[1], b[0] * L + b[1]
        num[g] = len(f['plants'])
    return {'edges': edges, 'num_edges': ne, 'gt': gt, 'gt_num': num, 'shift': [float(v) for v in fxs[0]['f_shift']],
            'scale': [float(v) for v in fxs[0]['f_scale']], 'tags': list(tags)}


def decode(rows, edges, num_edges, shift, scale):
    """rows fp32 [R, 16] of one garment (edges [P, L, 8]) -> per row ((e_a, flipped), (e_b, flipped)), or None for a row of zeros, by
    exact value match of each half against every present edge as stored and reversed, standardised in fp32; a half that matches
    nothing, or two candidates, is an error"""
    edges = np.asarray(edges, dtype=np.float32)
    P, L, Fe = edges.shape
    cnt = counts_of(num_edges, L)
    shift, scale = np.asarray(shift, dtype=np.float32), np.asarray(scale, dtype=np.float32)
    look = [{}, {}]
    for p in range(P):
        for l in range(cnt[p]):
            for flip, v in ((0, edges[p, l]), (1, flipped(edges[p, l]))):
                for h in (0, 1):
                    key = ((v - shift[h * Fe:(h + 1) * Fe]) / scale[h * Fe:(h + 1) * Fe]).tobytes()
                    assert key not in look[h], 'two edges give the same row half'
                    look[h][key] = (p * L + l, flip)
    out = []
    for r in np.asarray(rows, dtype=np.float32):
        out.append(None if not r.any() else (look[0][r[:Fe].tobytes()], look[1][r[Fe:].tobytes()]))
    return out


def check_slot(rows, labels, status, edges, num_edges, gt, gt_num, n_stitched, n_non, flags, shift, scale):
    """the invariants of one batch slot's output that need no random number: label count, every valid stitch present, no negative row
    a stitch or a self pair, one flip bit per edge, duplicates copies of stitch rows, give-ups zero rows counted by status"""
    P, L, _ = np.asarray(edges).shape
    st = valid_stitches(num_edges, L, gt, gt_num)
    R = n_stitched + n_non
    rows, labels = np.asarray(rows), np.asarray(labels).astype(bool)
    assert rows.shape[0] == R and labels.shape == (R,)
    if len(st) > n_stitched:
        assert status == -1 and not rows.any() and not labels.any()
        return
    assert status >= 0
    assert labels.sum() == (n_stitched if st else 0)
    dec = decode(rows, edges, num_edges, shift, scale)
    assert sum(1 for d in dec if d is None) == status and not any(labels[i] for i, d in enumerate(dec) if d is None)
    both = set(st) | {(b, a) for a, b in st}
    flip = {}
    for d in dec:
        for e, f in d or ():
            assert flip.setdefault(e, f) == f, 'edge %d is flipped in one row and not in another' % e
            assert flags & SHUFFLE_PAIRS or f == 0
    pos = [(d[0][0], d[1][0]) for i, d in enumerate(dec) if labels[i]]
    neg = [(d[0][0], d[1][0]) for i, d in enumerate(dec) if not labels[i] and d is not None]
    assert all(q in both for q in pos) and all(q not in both and q[0] != q[1] for q in neg)
    for a, b in set(st):
        fwd, rev = pos.count((a, b)), pos.count((b, a))
        assert fwd + rev >= 1, 'stitch %s is missing' % ((a, b),)
        if a != b and (b, a) not in st:
            assert fwd == 0 or rev == 0, 'copies of stitch %s differ in orientation' % ((a, b),)
            assert flags & SHUFFLE_PAIRS or rev == 0
    if not flags & SHUFFLE_ORDER:
        assert labels[:n_stitched if st else 0].all()
        assert pos[:len(st)] == st or flags & SHUFFLE_PAIRS

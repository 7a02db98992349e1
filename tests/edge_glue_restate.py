"""Test infrastructure: the EdgeConv glue kernels (csrc/gpe_edge_glue.hip, gpe_bn.hip, gpe_rowgemm.hip) restated one by one.

For every kernel: a case builder (`build_<kernel>`: the exact host buffers of one call, at their padded pitches, NaN where the
kernel must not read, a sentinel where it must not write), a plain fp64 reference written from the formula in include/gpe_hip.h
(`_ref_<kernel>`, on top of the `f_*` functions that tests/test_edge_glue_host.py composes into a whole layer), a checker
(`check_<kernel>(case, got, variant=None)`: element by element, bars in units of u = 2^-24 times a per-element magnitude of the
reference, AssertionError with the offending index) and an emulation (`emulate_<kernel>`: what a correct kernel returns — the fp64
reference rounded once, or the fp32 sequential restatement where the order of fp32 operations is part of the contract).

`variant=` makes the REFERENCE wrong in one plausible way (VARIANTS): the list of mistakes the case lists (CASES) must tell
apart — tests/test_edge_glue_host.py asserts that every variant is rejected by at least one case.

No GPU and no gpe_amd here: NumPy only.  `abi_args(case, dev)` lays out the C-ABI argument list of the call from a
{name: device tensor} map, so that tests/test_gpu_edge_glue.py is one loop."""
import types

import numpy as np

U = 2.0 ** -24
SENTINEL = -777.25
WORD_FILL = 0x7F000000          # a large bit pattern: an amax word the call does not reset keeps it (atomicMax on the bits)
NBLK = 512                      # GS_BLOCKS / PS_BLOCKS: partial blocks of the gather statistics and of the point sums
LD = np.longdouble


def round_up(x, m):
    return (x + m - 1) // m * m


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def f64(x):
    return np.asarray(x, dtype=np.float64)


def bits(x):
    return f32(x).view(np.uint32)


def word(v):
    """the uint32 [1] amax word holding the fp32 value v"""
    return np.array([v], np.float32).view(np.uint32).copy()


def word_value(w):
    return float(np.asarray(w, np.uint32).view(np.float32)[0])


class Case(types.SimpleNamespace):
    """kernel, id, p (scalars), inp {name: array the kernel reads}, out0 {name: array it writes, pre-filled}"""


def _case(kernel, p, inp, out0):
    name = '-'.join('%s%s' % (k, '%g' % v if isinstance(v, float) else v) for k, v in p.items() if k not in ('seed', 'eps', 'momentum', 'ldo'))
    return Case(kernel=kernel, id=name, p=p, inp=inp, out0=out0)


def padded(t, ld, fill):
    buf = np.full((t.shape[0], ld), fill, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf


# ----------------------------------------------------------------------------------------------------------------------
# comparison helpers: every failure names the kernel, the case, the output and the first offending index
# ----------------------------------------------------------------------------------------------------------------------
def _fail(case, what, idx, got, ref, extra=''):
    raise AssertionError('%s[%s] %s at %s: got %r, reference %r %s' % (case.kernel, case.id, what, tuple(int(i) for i in idx), got, ref, extra))


def _within(case, what, got, ref, bar):
    """|got - ref| <= bar element by element (a NaN fails) -> the worst |diff| / bar (0 where both are 0)"""
    got, ref = f64(got), f64(ref)
    bar = np.broadcast_to(f64(bar), ref.shape)
    assert got.shape == ref.shape, (case.kernel, case.id, what, got.shape, ref.shape)
    diff = np.abs(got - ref)
    bad = ~(diff <= bar)
    if bad.any():
        idx = np.argwhere(bad)[0]
        t = tuple(idx)
        _fail(case, what, idx, got[t], ref[t], '|diff| %.3e > bar %.3e (%.2f bars)' % (diff[t], bar[t], diff[t] / bar[t] if bar[t] > 0 else np.inf))
    pos = bar > 0
    return float((diff[pos] / bar[pos]).max()) if pos.any() else 0.0


def _same_bits(case, what, got, ref, mask=None):
    """bit-for-bit equality of two fp32 (or integer) arrays, where `mask`"""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape, (case.kernel, case.id, what, got.shape, ref.shape)
    if got.dtype == np.float32:
        a, b = got.view(np.uint32), f32(ref).view(np.uint32)
    elif got.dtype == np.float64:
        a, b = got.view(np.uint64), np.ascontiguousarray(ref, np.float64).view(np.uint64)
    else:
        a, b = got, ref.astype(got.dtype)
    bad = a != b
    if mask is not None:
        bad &= mask
    if bad.any():
        idx = np.argwhere(bad)[0]
        t = tuple(idx)
        _fail(case, what, idx, got[t], ref[t], '(bits differ)')


def _untouched(case, what, got, orig):
    """`got` still holds what the buffer was pre-filled with (NaN-safe: compared as bits)"""
    _same_bits(case, what + ' (must not be written)', got, orig)


def _seq_sum32(terms, init=None):
    """fp32 sum over the LAST axis in ascending order, starting from +0 (or init): the sequential restatement"""
    terms = f32(terms)
    s = np.zeros(terms.shape[:-1], np.float32) if init is None else f32(init).copy()
    for j in range(terms.shape[-1]):
        s = (s + terms[..., j]).astype(np.float32)
    return s


# ----------------------------------------------------------------------------------------------------------------------
# graphs
# ----------------------------------------------------------------------------------------------------------------------
def make_graph(rng, B, N, k):
    """[B][N][k] cloud-local neighbours: random, with self loops (slot 0 of every other point), duplicate neighbours (slots 0 and 1 of
    every third point) and one hub (point 0 is the last neighbour of the upper half of each cloud)"""
    idx = rng.integers(0, N, size=(B, N, k))
    idx[:, ::2, 0] = np.arange(N)[::2]
    if k > 1:
        idx[:, ::3, 1] = idx[:, ::3, 0]
    idx[:, N // 2:, k - 1] = 0
    return idx.astype(np.int32)


def graph_with_degrees(rng, B, N, k, hub):
    """in-degrees: point 0 `hub`, point 1 none, points 2..5 1, 3, 4, 5; the rest random over points 6..N-1"""
    fixed = [0] * hub + [2] + [3] * 3 + [4] * 4 + [5] * 5
    assert N > 6 and len(fixed) <= N * k
    out = np.empty((B, N * k), np.int64)
    for b in range(B):
        tgt = np.array(fixed + list(rng.integers(6, N, size=N * k - len(fixed))))
        out[b] = rng.permutation(tgt)
    return out.reshape(B, N, k).astype(np.int32)


def to_global(idx):
    B, N, _ = idx.shape
    return (idx + (np.arange(B) * N)[:, None, None]).astype(np.int32)


def reverse_graph(idx, variant=None):
    """rev_off [B][N+1] = exclusive scan of the in-degrees (rev_off[N] = N k), rev_edge [B][N k] = the cloud-local edge ids i k + s of
    every bucket in ascending order: a stable argsort of the targets"""
    B, N, k = idx.shape
    flat = idx.reshape(B, N * k)
    edge = np.argsort(flat, axis=1, kind='stable').astype(np.int32)
    off = np.zeros((B, N + 1), np.int32)
    for b in range(B):
        off[b, 1:] = np.cumsum(np.bincount(flat[b], minlength=N))
    if variant == 'bucket_unsorted':
        for b in range(B):
            for j in range(N):
                edge[b, off[b, j]:off[b, j + 1]] = edge[b, off[b, j]:off[b, j + 1]][::-1]
    elif variant == 'global_edge_ids':
        edge = (edge + (np.arange(B) * N * k)[:, None]).astype(np.int32)
    return off, edge


def _pull(rows, off, edge, B, N, k, init, global_ids=False, descending=False, dtype=np.float32):
    """out[b N + j] = init + sum of rows[b N k + e] over the bucket of (b, j), one edge after the other in bucket order"""
    out = np.array(init, dtype=dtype)
    deg = (off[:, 1:] - off[:, :-1]).reshape(-1)
    base = off[:, :-1].reshape(-1).astype(np.int64)
    cloud = np.repeat(np.arange(B), N)
    for r in range(int(deg.max()) if deg.size else 0):
        pts = np.nonzero(deg > r)[0]
        pos = base[pts] + (deg[pts] - 1 - r if descending else r)
        e = edge[cloud[pts], pos].astype(np.int64) + (0 if global_ids else cloud[pts] * N * k)
        out[pts] = (out[pts] + rows[e].astype(dtype)).astype(dtype)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the operations in fp64 (np.longdouble where a difference of large sums is formed): what the host test composes into a layer
# ----------------------------------------------------------------------------------------------------------------------
def f_gather_stats(P, Q, jg, variant=None, N=None):
    """sum and sum of squares of a1 = relu(P_i + Q_j) over all edges, per channel"""
    P, Q = f64(P), f64(Q)
    jg = np.asarray(jg, np.int64)
    if variant == 'local_jg':
        jg = jg % N
    if variant == 'clamped_slot':
        k = jg.shape[1]
        jg = np.concatenate([jg] + [jg[:, -1:]] * (round_up(k, 8) - k), axis=1)
    a = P[:, None, :] + Q[jg]
    if variant != 'no_relu':
        a = np.maximum(a, 0.0)
    return a.sum((0, 1)), (a * a).sum((0, 1))


def f_bn_finalize(S, Qs, count, gamma, beta, eps, variant=None):
    """-> mean, biased var (clamped at 0), rstd, s = gamma rstd, t = beta - mean s, all fp64 (eps as given: the kernels take a float)"""
    mean = np.asarray(S, LD) / LD(count)
    var = np.asarray(Qs, LD) / LD(count) - mean * mean
    if variant != 'var_not_clamped':
        var = np.maximum(var, 0)
    rstd = 1 / np.sqrt(var + LD(eps))
    s = np.asarray(gamma, LD) * rstd
    return f64(mean), f64(var), f64(rstd), f64(s), f64(np.asarray(beta, LD) - mean * s)


def f_bn_from_running(rm, rv, gamma, beta, eps, variant=None):
    e = 0.0 if variant == 'eps_dropped' else eps
    rstd = 1 / np.sqrt(f64(rv) + e)
    s = f64(gamma) * rstd
    t = f64(beta) + f64(rm) * s if variant == 't_plus' else f64(beta) - f64(rm) * s
    return f64(rm), rstd, s, t


def f_select(mx, mn, s, variant=None):
    """the sign-aware selection of BatchNorm after max: max where s >= 0 (+0 and -0.0 included), min elsewhere"""
    s = f64(s)
    pos = s > 0 if variant == 'sel_s_gt0' else s >= 0
    if variant == 'always_mx':
        pos = np.ones_like(pos)
    return np.where(pos, f64(mx), f64(mn))


def f_finish(mx, mn, s, t, variant=None):
    return f64(s) * f_select(mx, mn, s, variant) + f64(t)


def f_point_sums(g, mx, mn, mean, rstd, s, variant=None):
    """sum_i g, sum_i g xhat_sel with xhat = (sel - mean) rstd, per channel -> s1, s2, sum |g|, sum |g xhat|"""
    g = f64(g)
    xhat = f_select(mx, mn, s, variant) - f64(mean)
    if variant != 'xhat_no_rstd':
        xhat = xhat * f64(rstd)
    if variant == 'tail_rows_dropped':
        keep = g.shape[0] // (8 * NBLK) * (8 * NBLK)
        g, xhat = g[:keep], xhat[:keep]
    return g.sum(0), (g * xhat).sum(0), np.abs(g).sum(0), np.abs(g * xhat).sum(0)


def f_bn_bwd_coef(s1, s2, mean, rstd, s, count, variant=None):
    """coef = {s, c1 = s mean(dy), k2 = s rstd mean(dy xhat), mean}; dgamma = sum dy xhat, dbeta = sum dy"""
    n = count - 1 if variant == 'count_minus_1' else count
    k2 = f64(s) * f64(s2) / n
    if variant != 'k2_no_rstd':
        k2 = k2 * f64(rstd)
    return np.stack([f64(s), f64(s) * f64(s1) / n, k2, f64(mean)]), f64(s2), f64(s1)


def f_dz3(a, g, coef, k, gscale=1.0, amx=None, amn=None, variant=None):
    """dz3 = (a > 0) ? [slot == argsel] s g gscale - c1 - (a - mean) k2 : 0 over a [BN k][F]; amx None = every slot carries the gradient
    -> value, magnitude sum of its three terms (0 where the ReLU is closed)"""
    F = a.shape[1]
    a = f64(a).reshape(-1, k, F)
    s, c1, k2, mean = f64(coef)
    sg = s * f64(g) * (1.0 if variant == 'gscale_dropped' else float(np.float32(gscale)))
    if amx is None:
        hit = np.broadcast_to(sg[:, None, :], a.shape)
    else:
        pos = s > 0 if variant == 'sel_s_gt0' else s >= 0
        sel = np.where(pos, np.asarray(amx, np.int64), np.asarray(amn, np.int64))
        hit = np.where(sel[:, None, :] == np.arange(k)[None, :, None], sg[:, None, :], 0.0)
    tail = (a - mean) * k2
    val = hit - c1 - tail
    live = a >= 0 if variant == 'relu_ge0' else a > 0
    mag = np.abs(hit) + np.abs(c1) + np.abs(tail)
    return np.where(live, val, 0.0).reshape(-1, F), np.where(live, mag, 0.0).reshape(-1, F)


def f_bn_bwd_from_G(G, db, w, mean, rstd, s, t, variant=None):
    """sums[0][c] = sum_f w[f][c] db[f]; sums[1][c] = rstd_c sum_f w[f][c] G[f][c]; dW[f][c] = G[f][c] s_c + db[f] beta_c with
    beta = t + mean s -> sums [2][C], their magnitude sums [2][C], dW [Cn][C]"""
    G, db, w = f64(G), f64(db), f64(w)
    if variant == 'last_row_dropped':
        Gs, dbs, ws = G[:-1], db[:-1], w[:-1]
    else:
        Gs, dbs, ws = G, db, w
    r = 1.0 if variant == 'rstd_dropped' else f64(rstd)
    sums = np.stack([(ws * dbs[:, None]).sum(0), r * (ws * Gs).sum(0)])
    mags = np.stack([np.abs(ws * dbs[:, None]).sum(0), np.abs(r) * np.abs(ws * Gs).sum(0)])
    beta = f64(t) if variant == 'dw_uses_t' else f64(t) + f64(mean) * f64(s)
    return sums, mags, G * f64(s) + db[:, None] * beta


def f_pull(rows, idx):
    """out[b N + j] = sum of rows[e] over the edges e whose neighbour is point j of cloud b, in fp64"""
    out = np.zeros((idx.shape[0] * idx.shape[1], rows.shape[1]))
    np.add.at(out, to_global(idx).reshape(-1), f64(rows))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# shared inputs
# ----------------------------------------------------------------------------------------------------------------------
def make_stats(rng, C):
    """[4][C] fp32 {mean, rstd, s, t}: the scale cycles through +, -, +0.0, -0.0 (t = -0.0 under a zero scale, so that the sign of
    a zero result tells which operand was selected)"""
    role = np.arange(C) % 4
    s = rng.uniform(0.3, 2.0, C) * np.where(role == 1, -1.0, 1.0)
    s = np.where(role == 2, 0.0, np.where(role == 3, -0.0, s))
    t = np.where(role >= 2, -0.0, rng.standard_normal(C))
    return f32(np.stack([rng.standard_normal(C), rng.uniform(0.5, 2.0, C), s, t]))


def make_coef(rng, C):
    """[4][C] fp32 {s, c1, k2, mean}; under a zero scale c1 = k2 = +0, as gpe_bn_bwd_coef gives them"""
    st = make_stats(rng, C)
    zero = (st[2] == 0)
    c1 = np.where(zero, 0.0, rng.standard_normal(C) * 0.3)
    k2 = np.where(zero, 0.0, rng.standard_normal(C) * 0.2)
    return f32(np.stack([st[2], c1, k2, st[0]]))


def make_gammas(rng, C):
    role = np.arange(C) % 5
    g = rng.uniform(0.3, 2.0, C) * np.where(role == 2, -1.0, 1.0)
    return f32(np.where(role == 3, 0.0, np.where(role == 4, -0.0, g)))


# ======================================================================================================================
# gpe_edge_gather_stats
# ======================================================================================================================
def build_edge_gather_stats(B, N, k, H, seed=0):
    rng = np.random.default_rng(seed)
    BN = B * N
    P, Q = rng.standard_normal((BN, H)), rng.standard_normal((BN, H))
    P[:, 1] = -np.abs(P[:, 1]) - 0.1                       # channel 1: P + Q < 0 on every edge -> sum and sum of squares exactly 0
    Q[:, 1] = -np.abs(Q[:, 1])
    pq = padded(f32(np.concatenate([P, Q], 1)), 2 * H + 4, np.nan)
    jg = to_global(make_graph(rng, B, N, k)).reshape(BN, k)
    return _case('gpe_edge_gather_stats', dict(B=B, N=N, k=k, H=H, seed=seed), dict(pq=pq, jg=jg),
                 dict(part=np.full((NBLK, 2, H), SENTINEL, np.float64)))


def _ref_edge_gather_stats(case, variant=None):
    H = case.p['H']
    pq = case.inp['pq']
    return f_gather_stats(pq[:, :H], pq[:, H:2 * H], case.inp['jg'], variant, case.p['N'])


def check_edge_gather_stats(case, got, variant=None):
    S, Q = _ref_edge_gather_stats(case, variant)
    part = f64(got['part'])
    bar = (case.p['k'] + 2) * U
    return dict(sum=_within(case, 'sum', part[:, 0].sum(0), S, bar * np.abs(S)),
                sumsq=_within(case, 'sum of squares', part[:, 1].sum(0), Q, bar * np.abs(Q)))


def emulate_edge_gather_stats(case, seq=False):
    S, Q = _ref_edge_gather_stats(case)
    part = np.zeros_like(case.out0['part'])
    part[NBLK - 1, 0], part[NBLK - 1, 1] = S, Q
    return dict(part=part)


# ======================================================================================================================
# gpe_bn_finalize / gpe_bn_from_running
# ======================================================================================================================
def build_bn_finalize(nblk, C, count=1000.0, running=True, seed=0):
    """partials of channels with |mean| <= 10 std; channel 1 (mod 5) is constant at 7.5 with a sum of squares 1e-8 below count v^2 —
    what fp32 per-point sums can leave behind — so that the biased variance is negative before the clamp"""
    rng = np.random.default_rng(seed)
    std = rng.uniform(0.3, 1.5, C)
    mean = rng.uniform(-2.0, 2.0, C)
    if count == 1.0:
        std = np.zeros(C)
    S, Qs = count * mean, count * (std * std + mean * mean)
    const = (np.arange(C) % 5 == 1)
    S = np.where(const, count * 7.5, S)
    Qs = np.where(const, count * 7.5 * 7.5 * (1 - 1e-8), Qs)
    wts = rng.uniform(0.2, 1.0, (nblk, 1))
    wts /= wts.sum()
    part = np.stack([wts * S, wts * Qs], 1)                         # [nblk][2][C]
    inp = dict(part=part, gamma=make_gammas(rng, C), beta=f32(rng.standard_normal(C)))
    out0 = dict(stats=np.full((4, C), SENTINEL, np.float32))
    if running:
        out0.update(rm=f32(rng.standard_normal(C)), rv=f32(rng.uniform(0.5, 2.0, C)), nbt=np.array([41], np.int64))
    p = dict(nblk=nblk, C=C, count=count, running=int(running), eps=1e-5, momentum=0.1, seed=seed)
    c = _case('gpe_bn_finalize', p, inp, out0)
    c.mean, c.std = np.where(const, 7.5, mean), np.where(const, 0.0, std)
    return c


def _ref_bn_finalize(case, variant=None):
    p, part = case.p, np.asarray(case.inp['part'], LD)
    if variant == 'last_block_dropped':
        part = part[:max(1, p['nblk'] - 1)]
    S, Qs = part[:, 0].sum(0), part[:, 1].sum(0)
    mean, var, rstd, s, t = f_bn_finalize(S, Qs, p['count'], case.inp['gamma'], case.inp['beta'], float(np.float32(p['eps'])), variant)
    r = dict(mean=mean, rstd=rstd, s=s, t=t, tmag=np.abs(f64(case.inp['beta'])) + np.abs(mean * s))
    if p['running']:
        m = float(np.float32(p['momentum']))
        n = p['count']
        unb = var * n / (n - 1) if n > 1 and variant != 'biased_running_var' else var
        r['rm'] = ((1 - m) * f64(case.out0['rm']), m * mean)
        r['rv'] = ((1 - m) * f64(case.out0['rv']), m * unb)
        r['nbt'] = case.out0['nbt'] + (0 if variant == 'nbt_not_incremented' else 1)
    return r


def check_bn_finalize(case, got, variant=None):
    r, st = _ref_bn_finalize(case, variant), got['stats']
    w = dict(mean=_within(case, 'mean', st[0], r['mean'], 2 * U * np.abs(r['mean'])),
             rstd=_within(case, 'rstd', st[1], r['rstd'], 2 * U * np.abs(r['rstd'])),
             s=_within(case, 's', st[2], r['s'], 2 * U * np.abs(r['s'])),
             t=_within(case, 't', st[3], r['t'], 2 * U * r['tmag']))
    if case.p['running']:
        for name in ('rm', 'rv'):
            old, new = r[name]
            w[name] = _within(case, 'running ' + name, got[name], old + new, 2 * U * (np.abs(old) + np.abs(new)))
        _same_bits(case, 'num_batches_tracked', got['nbt'], r['nbt'])
    return w


def emulate_bn_finalize(case, seq=False):
    r = _ref_bn_finalize(case)
    got = dict(stats=f32(np.stack([r['mean'], r['rstd'], r['s'], r['t']])))
    if case.p['running']:
        got.update(rm=f32(r['rm'][0] + r['rm'][1]), rv=f32(r['rv'][0] + r['rv'][1]), nbt=r['nbt'])
    return got


def build_bn_from_running(C, seed=0):
    rng = np.random.default_rng(seed)
    inp = dict(rm=f32(rng.standard_normal(C)), rv=f32(rng.uniform(0.01, 2.0, C)), gamma=make_gammas(rng, C),
               beta=f32(rng.standard_normal(C)))
    return _case('gpe_bn_from_running', dict(C=C, eps=1e-5, seed=seed), inp, dict(stats=np.full((4, C), SENTINEL, np.float32)))


def _ref_bn_from_running(case, variant=None):
    i = case.inp
    mean, rstd, s, t = f_bn_from_running(i['rm'], i['rv'], i['gamma'], i['beta'], float(np.float32(case.p['eps'])), variant)
    return dict(mean=mean, rstd=rstd, s=s, t=t, tmag=np.abs(f64(i['beta'])) + np.abs(mean * s))


def check_bn_from_running(case, got, variant=None):
    r, st = _ref_bn_from_running(case, variant), got['stats']
    return dict(mean=_within(case, 'mean', st[0], r['mean'], 2 * U * np.abs(r['mean'])),
                rstd=_within(case, 'rstd', st[1], r['rstd'], 2 * U * np.abs(r['rstd'])),
                s=_within(case, 's', st[2], r['s'], 2 * U * np.abs(r['s'])),
                t=_within(case, 't', st[3], r['t'], 2 * U * r['tmag']))


def emulate_bn_from_running(case, seq=False):
    r = _ref_bn_from_running(case)
    return dict(stats=f32(np.stack([r['mean'], r['rstd'], r['s'], r['t']])))


# ======================================================================================================================
# gpe_edge_finish / gpe_bn_apply
# ======================================================================================================================
def build_edge_finish(rows, C, seed=0):
    rng = np.random.default_rng(seed)
    alloc = max(rows, 1)                                    # (rows = 0 still needs non-NULL pointers)
    mx = np.abs(rng.standard_normal((alloc, C))) + 0.1      # mx > 0 > mn: under a zero scale the sign of the zero tells them apart
    mn = -np.abs(rng.standard_normal((alloc, C))) - 0.1
    inp = dict(mx=padded(f32(mx), C + 3, np.nan), mn=padded(f32(mn), C + 3, np.nan), stats=make_stats(rng, C))
    return _case('gpe_edge_finish', dict(rows=rows, C=C, seed=seed), inp, dict(y=np.full((alloc, C + 2), SENTINEL, np.float32)))


def _check_affine(case, got, y, mag):
    rows, C = case.p['rows'], case.p['C']
    if rows == 0:
        _untouched(case, 'y', got['y'], case.out0['y'])
        return dict(y=0.0)
    bar = 2 * U * mag
    w = _within(case, 'y', got['y'][:rows, :C], y, bar)
    _same_bits(case, 'y where the bar is 0 (sign of zero included)', got['y'][:rows, :C], f32(y), mask=(bar == 0))
    _untouched(case, 'y pad', got['y'][:, C:], case.out0['y'][:, C:])
    return dict(y=w)


def _ref_edge_finish(case, variant=None):
    C, i = case.p['C'], case.inp
    s, t = f64(i['stats'][2]), f64(i['stats'][3])
    v = f_select(i['mx'][:, :C], i['mn'][:, :C], s, variant)
    return s * v + t, np.abs(s * v) + np.abs(t)


def check_edge_finish(case, got, variant=None):
    return _check_affine(case, got, *_ref_edge_finish(case, variant))


def _emulate_affine(case, y):
    out = case.out0['y'].copy()
    if case.p['rows']:
        out[:, :case.p['C']] = f32(y)
    return dict(y=out)


def emulate_edge_finish(case, seq=False):
    return _emulate_affine(case, _ref_edge_finish(case)[0])


def build_bn_apply(rows, C, seed=0):
    rng = np.random.default_rng(seed)
    alloc = max(rows, 1)
    a = np.maximum(rng.standard_normal((alloc, C)), 0.0)
    inp = dict(a=padded(f32(a), C + 3, np.nan), stats=make_stats(rng, C))
    return _case('gpe_bn_apply', dict(rows=rows, C=C, seed=seed), inp, dict(y=np.full((alloc, C + 2), SENTINEL, np.float32)))


def _ref_bn_apply(case, variant=None):
    C, i = case.p['C'], case.inp
    s = f64(i['stats'][1 if variant == 'uses_rstd_row' else 2])
    t = 0.0 * f64(i['stats'][3]) if variant == 't_dropped' else f64(i['stats'][3])
    sa = s * f64(i['a'][:, :C])
    return sa + t, np.abs(sa) + np.abs(t)


def check_bn_apply(case, got, variant=None):
    return _check_affine(case, got, *_ref_bn_apply(case, variant))


def emulate_bn_apply(case, seq=False):
    return _emulate_affine(case, _ref_bn_apply(case)[0])


# ======================================================================================================================
# gpe_edge_sum_k: fp32, slots ascending from +0
# ======================================================================================================================
def build_edge_sum_k(npts, k, F, seed=0):
    rng = np.random.default_rng(seed)
    a = f32(rng.standard_normal((npts * k, F)))
    return _case('gpe_edge_sum_k', dict(npts=npts, k=k, F=F, seed=seed), dict(a=padded(a, F + 3, np.nan)),
                 dict(out=np.full((npts, F + 2), SENTINEL, np.float32)))


def _ref_edge_sum_k(case, variant=None):
    p = case.p
    a = case.inp['a'][:, :p['F']].reshape(p['npts'], p['k'], p['F']).transpose(0, 2, 1)      # [npts][F][k]
    if variant == 'last_slot_dropped':
        a = a[..., :max(1, p['k'] - 1)]
    if variant == 'slots_descending':
        a = a[..., ::-1]
    seq = _seq_sum32(a)
    if variant == 'no_grid_stride':
        seq[8192:] = SENTINEL                                                                 # 2048 workgroups x 4 waves, one pass
    return seq, f64(a).sum(-1), np.abs(f64(a)).sum(-1)


def _check_seq(case, what, got, seq, ref64, mag, deg):
    """bit-exact against the fp32 sequential restatement, which is itself within deg u sum|terms| of the fp64 value"""
    _within(case, what + ': the restatement against fp64', seq, ref64, deg * U * mag)
    _same_bits(case, what, got, seq)
    return float(np.max(np.abs(f64(got) - ref64) / np.maximum(deg * U * mag, 1e-300))) if ref64.size else 0.0


def check_edge_sum_k(case, got, variant=None):
    seq, ref64, mag = _ref_edge_sum_k(case, variant)
    F = case.p['F']
    if variant is not None:                                  # (a wrong restatement need not be close to fp64: only the bits are compared)
        _same_bits(case, 'out', got['out'][:, :F], seq)
        return {}
    w = _check_seq(case, 'out', got['out'][:, :F], seq, ref64, mag, case.p['k'])
    _untouched(case, 'out pad', got['out'][:, F:], case.out0['out'][:, F:])
    return dict(out_vs_fp64=w)


def emulate_edge_sum_k(case, seq=False):
    out = case.out0['out'].copy()
    s, r, _ = _ref_edge_sum_k(case)
    out[:, :case.p['F']] = s if seq else f32(r)
    return dict(out=out)


# ======================================================================================================================
# gpe_edge_inputs_fwd / gpe_edge_inputs_bwd
# ======================================================================================================================
def build_edge_inputs_fwd(B, N, k, C, seed=0):
    rng = np.random.default_rng(seed)
    npts = B * N
    x = f32(rng.standard_normal((npts, C)))
    jg = to_global(make_graph(rng, B, N, k)).reshape(npts * k)
    ldo = round_up(2 * C, 4) + 4
    return _case('gpe_edge_inputs_fwd', dict(B=B, N=N, k=k, C=C, ldo=ldo, seed=seed), dict(x=padded(x, C + 1, np.nan), jg=jg),
                 dict(out=np.full((npts * k, ldo), SENTINEL, np.float32)))


def _ref_edge_inputs_fwd(case, variant=None):
    p = case.p
    x = case.inp['x'][:, :p['C']]
    xi = np.repeat(x, p['k'], axis=0)
    xj = x[case.inp['jg']]
    d32 = (xi - xj) if variant == 'xi_minus_xj' else (xj - xi)                                # fp32: one subtraction
    d64 = f64(xi) - f64(xj) if variant == 'xi_minus_xj' else f64(xj) - f64(xi)
    return np.concatenate([xi, d32.astype(np.float32)], 1), np.concatenate([f64(xi), d64], 1), np.concatenate([np.abs(f64(xi)), np.abs(f64(xi)) + np.abs(f64(xj))], 1)


def check_edge_inputs_fwd(case, got, variant=None):
    seq, ref64, mag = _ref_edge_inputs_fwd(case, variant)
    C = case.p['C']
    w = _check_seq(case, 'out', got['out'][:, :2 * C], seq, ref64, mag, 1)
    if variant == 'pad_untouched':
        _untouched(case, 'out pad', got['out'][:, 2 * C:], case.out0['out'][:, 2 * C:])
    else:
        _same_bits(case, 'out pad (all of it is written 0)', got['out'][:, 2 * C:], np.zeros_like(got['out'][:, 2 * C:]))
    return dict(out_vs_fp64=w)


def emulate_edge_inputs_fwd(case, seq=False):
    out = np.zeros_like(case.out0['out'])
    s, r, _ = _ref_edge_inputs_fwd(case)
    out[:, :2 * case.p['C']] = s if seq else f32(r)
    return dict(out=out)


def build_edge_inputs_bwd(B, N, k, C, seed=0):
    rng = np.random.default_rng(seed)
    idx = make_graph(rng, B, N, k)
    off, edge = reverse_graph(idx)                          # built here, not by gpe_knn_reverse
    g = f32(rng.standard_normal((B * N * k, 2 * C)))
    c = _case('gpe_edge_inputs_bwd', dict(B=B, N=N, k=k, C=C, seed=seed),
              dict(g=padded(g, round_up(2 * C, 4) + 4, np.nan), rev_off=off, rev_edge=edge),
              dict(gx=np.full((B * N, C + 2), SENTINEL, np.float32)))
    c.idx = idx
    return c


def _ref_edge_inputs_bwd(case, variant=None):
    p = case.p
    B, N, k, C = p['B'], p['N'], p['k'], p['C']
    g1, g2 = case.inp['g'][:, :C], case.inp['g'][:, C:2 * C]
    own = g1.copy() if variant == 'g2_not_subtracted' else (g1 - g2).astype(np.float32)
    own = own.reshape(B * N, k, C).transpose(0, 2, 1)
    off, edge = case.inp['rev_off'], case.inp['rev_edge']
    gl = variant == 'global_edge_ids'
    if variant == 'pull_first':
        seq = _seq_sum32(own, init=_pull(g2, off, edge, B, N, k, np.zeros((B * N, C), np.float32)))
    else:
        seq = _pull(g2, off, edge, B, N, k, _seq_sum32(own), global_ids=gl)
    ref64 = (f64(g1) - f64(g2)).reshape(B * N, k, C).sum(1) + f_pull(g2, case.idx)
    mag = (np.abs(f64(g1)) + np.abs(f64(g2))).reshape(B * N, k, C).sum(1) + f_pull(np.abs(g2), case.idx)
    deg = (k + (off[:, 1:] - off[:, :-1]).reshape(-1))[:, None]
    return seq, ref64, mag, deg


def check_edge_inputs_bwd(case, got, variant=None):
    seq, ref64, mag, deg = _ref_edge_inputs_bwd(case, variant)
    C = case.p['C']
    if variant is not None:                                  # (a wrong restatement need not be close to fp64: only the bits are compared)
        _same_bits(case, 'gx', got['gx'][:, :C], seq)
        return {}
    w = _check_seq(case, 'gx', got['gx'][:, :C], seq, ref64, mag, deg)
    _untouched(case, 'gx pad', got['gx'][:, C:], case.out0['gx'][:, C:])
    return dict(gx_vs_fp64=w)


def emulate_edge_inputs_bwd(case, seq=False):
    out = case.out0['gx'].copy()
    s, r = _ref_edge_inputs_bwd(case)[:2]
    out[:, :case.p['C']] = s if seq else f32(r)
    return dict(gx=out)


# ======================================================================================================================
# gpe_knn_reverse
# ======================================================================================================================
def build_knn_reverse(B, N, k, hub=0, seed=0):
    rng = np.random.default_rng(seed)
    if hub:
        idx = rng.integers(10, N, size=(B, N, k)).astype(np.int32)          # points 1 .. 9 isolated
        flat = idx.reshape(B, -1)
        flat[:, rng.permutation(N * k)[:hub]] = 0                           # point 0: in-degree `hub`
    else:
        idx = rng.integers(0, N, size=(B, N, k)).astype(np.int32)
    return _case('gpe_knn_reverse', dict(B=B, N=N, k=k, hub=hub, seed=seed), dict(idx=idx),
                 dict(rev_off=np.full((B, N + 1), -1, np.int32), rev_edge=np.full((B, N * k), -1, np.int32)))


def knn_reverse_uses_lds(N, k):
    """the launcher's rule: counters and offsets (2 N + 1 ints) plus the N k edge ids within 150 KB -> edges sorted in LDS"""
    return (2 * N + 1 + N * k) * 4 <= 150 * 1024


def check_knn_reverse(case, got, variant=None):
    off, edge = reverse_graph(case.inp['idx'], variant)
    if variant == 'rev_off_N_missing':
        off[:, -1] = -1
    _same_bits(case, 'rev_off', got['rev_off'], off)
    _same_bits(case, 'rev_edge', got['rev_edge'], edge)
    return {}


def emulate_knn_reverse(case, seq=False):
    off, edge = reverse_graph(case.inp['idx'])
    return dict(rev_off=off, rev_edge=edge)


# ======================================================================================================================
# gpe_edge_pull_dq: fp32, incoming edges in ascending edge id from +0, into the right half of a [BN][2H] buffer
# ======================================================================================================================
def build_edge_pull_dq(B, N, k, H, hub=300, seed=0):
    rng = np.random.default_rng(seed)
    idx = graph_with_degrees(rng, B, N, k, hub)
    off, edge = reverse_graph(idx)
    dz = f32(rng.standard_normal((B * N * k, H)))
    c = _case('gpe_edge_pull_dq', dict(B=B, N=N, k=k, H=H, seed=seed), dict(dz=padded(dz, H + 4, np.nan), rev_off=off, rev_edge=edge),
              dict(dpq=np.full((B * N, 2 * H), SENTINEL, np.float32)))
    c.idx = idx
    return c


def _ref_edge_pull_dq(case, variant=None):
    p = case.p
    B, N, k, H = p['B'], p['N'], p['k'], p['H']
    dz = case.inp['dz'][:, :H]
    off, edge = case.inp['rev_off'], case.inp['rev_edge']
    seq = _pull(dz, off, edge, B, N, k, np.zeros((B * N, H), np.float32), global_ids=(variant == 'global_edge_ids'),
                descending=(variant == 'descending_order'))
    deg = (off[:, 1:] - off[:, :-1]).reshape(-1)[:, None]
    return seq, f_pull(dz, case.idx), f_pull(np.abs(dz), case.idx), deg


def check_edge_pull_dq(case, got, variant=None):
    seq, ref64, mag, deg = _ref_edge_pull_dq(case, variant)
    H = case.p['H']
    left, right = got['dpq'][:, :H], got['dpq'][:, H:]
    if variant == 'left_half_overwritten':
        _same_bits(case, 'dPQ left half', left, seq)
        return {}
    if variant is not None:
        _same_bits(case, 'dQ', right, seq)
        return {}
    w = _check_seq(case, 'dQ', right, seq, ref64, mag, deg)
    _untouched(case, 'dPQ left half', left, case.out0['dpq'][:, :H])
    return dict(dq_vs_fp64=w)


def emulate_edge_pull_dq(case, seq=False):
    out = case.out0['dpq'].copy()
    s, r = _ref_edge_pull_dq(case)[:2]
    out[:, case.p['H']:] = s if seq else f32(r)
    return dict(dpq=out)


# ======================================================================================================================
# gpe_edge_bwd_point_sums
# ======================================================================================================================
def build_edge_bwd_point_sums(rows, C, with_word=True, seed=0):
    rng = np.random.default_rng(seed)
    mx = np.abs(rng.standard_normal((rows, C))) + 0.1
    mn = mx - np.abs(rng.standard_normal((rows, C))) - 0.1
    g = f32(rng.standard_normal((rows, C)))
    inp = dict(g=padded(g, C + 1, np.nan), mx=padded(f32(mx), C + 3, np.nan), mn=padded(f32(mn), C + 3, np.nan),
               stats=make_stats(rng, C))
    out0 = dict(part=np.full((NBLK, 2, C), SENTINEL, np.float64))
    if with_word:
        out0['word'] = np.array([WORD_FILL], np.uint32)
    return _case('gpe_edge_bwd_point_sums', dict(rows=rows, C=C, word=int(with_word), seed=seed), inp, out0)


def _ref_edge_bwd_point_sums(case, variant=None):
    C, i = case.p['C'], case.inp
    st = i['stats']
    s1, s2, m1, m2 = f_point_sums(i['g'][:, :C], i['mx'][:, :C], i['mn'][:, :C], st[0], st[1], st[2], variant)
    return s1, s2, m1, m2, float(np.abs(f64(st[2]) * f64(i['g'][:, :C])).max())


def check_edge_bwd_point_sums(case, got, variant=None):
    s1, s2, m1, m2, amax = _ref_edge_bwd_point_sums(case, variant)
    part = f64(got['part'])
    w = dict(s1=_within(case, 'sum g', part[:, 0].sum(0), s1, 1e-13 * m1),
             s2=_within(case, 'sum g xhat', part[:, 1].sum(0), s2, 4 * U * m2))
    if case.p['word']:
        if variant == 'word_not_reset':
            amax = max(amax, word_value(np.array([WORD_FILL], np.uint32)))
        v = word_value(got['word'])
        if not (amax <= v <= amax * (1 + 8 * U)):
            _fail(case, 'amax_sg word', (0,), v, amax, '(must lie in [true, true (1 + 8u)])')
        w['word'] = (v / amax - 1) / (8 * U) if amax > 0 else 0.0
    return w


def emulate_edge_bwd_point_sums(case, seq=False):
    s1, s2, _, _, amax = _ref_edge_bwd_point_sums(case)
    part = np.zeros_like(case.out0['part'])
    part[NBLK - 1, 0], part[NBLK - 1, 1] = s1, s2
    got = dict(part=part)
    if case.p['word']:
        v = np.float32(amax)
        got['word'] = word(v if float(v) >= amax else np.nextafter(v, np.float32(np.inf)))
    return got


# ======================================================================================================================
# gpe_bn_bwd_coef
# ======================================================================================================================
def build_bn_bwd_coef(nblk, C, with_grads=True, count=3000.0, seed=0):
    rng = np.random.default_rng(seed)
    part = rng.standard_normal((nblk, 2, C)) + 0.25
    out0 = dict(coef=np.full((4, C), SENTINEL, np.float32))
    if with_grads:
        out0.update(dgamma=np.full(C, SENTINEL, np.float32), dbeta=np.full(C, SENTINEL, np.float32))
    return _case('gpe_bn_bwd_coef', dict(nblk=nblk, C=C, grads=int(with_grads), count=count, seed=seed),
                 dict(part=part, stats=make_stats(rng, C)), out0)


def _ref_bn_bwd_coef(case, variant=None):
    part, st = np.asarray(case.inp['part'], LD), case.inp['stats']
    if variant == 'last_block_dropped':
        part = part[:max(1, case.p['nblk'] - 1)]
    return f_bn_bwd_coef(f64(part[:, 0].sum(0)), f64(part[:, 1].sum(0)), st[0], st[1], st[2], case.p['count'], variant)


def check_bn_bwd_coef(case, got, variant=None):
    coef, dg, db = _ref_bn_bwd_coef(case, variant)
    w = dict(coef=_within(case, 'coef', got['coef'], coef, 2 * U * np.abs(coef)))
    if case.p['grads']:
        w['dgamma'] = _within(case, 'dgamma', got['dgamma'], dg, 2 * U * np.abs(dg))
        w['dbeta'] = _within(case, 'dbeta', got['dbeta'], db, 2 * U * np.abs(db))
    return w


def emulate_bn_bwd_coef(case, seq=False):
    coef, dg, db = _ref_bn_bwd_coef(case)
    got = dict(coef=f32(coef))
    if case.p['grads']:
        got.update(dgamma=f32(dg), dbeta=f32(db))
    return got


# ======================================================================================================================
# gpe_edge_dz3 / gpe_edge_dz3_all (in place over a3)
# ======================================================================================================================
def _build_dz3(kernel, B, N, k, F, gscale, with_word, seed):
    rng = np.random.default_rng(seed)
    BN, E = B * N, B * N * k
    ru = round_up(F, 4)
    a = np.maximum(rng.standard_normal((E, F)), 0.0)       # about half of it exact +0.0
    flat = a.reshape(-1)
    flat[::7] = 0.0
    flat[3::41] = -0.0                                      # a3 <= 0 in every spelling: +0.0, -0.0, negative
    flat[5::53] = -1.5
    if F >= 3:
        a[:, 2] = 0.0                                       # a dead channel
    a3 = np.full((E, ru + 4), SENTINEL, np.float32)
    a3[:, :ru] = np.nan                                     # columns F .. round_up(F, 4) - 1: loaded with the quad, written 0
    a3[:, :F] = f32(a)
    g = f32(rng.standard_normal((BN, F)))
    inp = dict(g=padded(g, F + 1, np.nan), coef=make_coef(rng, F))
    if kernel == 'gpe_edge_dz3':
        e = np.arange(BN)[:, None] * F + np.arange(F)[None, :]
        amx = e % k                                         # every slot, k - 1 included
        amn = (amx + 1 + (e // 3) % max(k - 1, 1)) % k      # != amx whenever k > 1
        inp.update(amx=padded(amx.astype(np.uint8), ru + 4, 255), amn=padded(amn.astype(np.uint8), ru + 4, 255))
    out0 = dict(a3=a3)
    if with_word:
        out0['word'] = np.array([WORD_FILL], np.uint32)
    p = dict(B=B, N=N, k=k, F=F, gscale=float(np.float32(gscale)), word=int(with_word), seed=seed)
    return _case(kernel, p, inp, out0)


def build_edge_dz3(B, N, k, F, with_word=True, seed=0):
    return _build_dz3('gpe_edge_dz3', B, N, k, F, 1.0, with_word, seed)


def build_edge_dz3_all(B, N, k, F, gscale=1.0, with_word=True, seed=0):
    return _build_dz3('gpe_edge_dz3_all', B, N, k, F, gscale, with_word, seed)


def _ref_dz3(case, variant=None):
    p, i = case.p, case.inp
    F = p['F']
    sel = (i['amx'][:, :F], i['amn'][:, :F]) if 'amx' in i else (None, None)
    return f_dz3(case.out0['a3'][:, :F], i['g'][:, :F], i['coef'], p['k'], p['gscale'], sel[0], sel[1], variant)


def check_edge_dz3(case, got, variant=None):
    val, mag = _ref_dz3(case, variant)
    F = case.p['F']
    ru = round_up(F, 4)
    out = got['a3']
    bar = 8 * U * mag
    w = dict(dz3=_within(case, 'dz3', out[:, :F], val, bar))
    # a closed ReLU gives exactly +0; where all three terms are 0 (a zero scale) the sign of the zero is the selected slot's
    _same_bits(case, 'dz3 where the bar is 0 (sign of zero included)', out[:, :F], f32(val), mask=(bar == 0))
    if variant == 'quad_pad_untouched':
        _untouched(case, 'columns F .. round_up(F, 4)', out[:, F:ru], case.out0['a3'][:, F:ru])
    else:
        _same_bits(case, 'columns F .. round_up(F, 4) (written 0)', out[:, F:ru], np.zeros_like(out[:, F:ru]))
    _untouched(case, 'columns from round_up(F, 4)', out[:, ru:], case.out0['a3'][:, ru:])
    if case.p['word']:
        exp = int(np.abs(out[:, :ru]).view(np.uint32).max())
        if variant == 'word_not_reset':
            exp = max(exp, WORD_FILL)
        if int(got['word'][0]) != exp:
            _fail(case, 'amax_out word', (0,), hex(int(got['word'][0])), hex(exp), '(bits of the largest |value| written)')
    return w


check_edge_dz3_all = check_edge_dz3


def emulate_edge_dz3(case, seq=False):
    F = case.p['F']
    out = case.out0['a3'].copy()
    out[:, :round_up(F, 4)] = 0.0
    out[:, :F] = f32(_ref_dz3(case)[0])
    got = dict(a3=out)
    if case.p['word']:
        got['word'] = np.array([np.abs(out[:, :round_up(F, 4)]).view(np.uint32).max()], np.uint32)
    return got


emulate_edge_dz3_all = emulate_edge_dz3


# ======================================================================================================================
# gpe_edge_dz3_bound
# ======================================================================================================================
def build_edge_dz3_bound(F, seed=0):
    """the words and coefficients of a small dz3 case (1 x 8 points x 4 slots), so that the bound and max |dz3| both apply"""
    d = build_edge_dz3(1, 8, 4, F, True, seed)
    s = f64(d.inp['coef'][0])
    sg = np.float32(np.abs(s * f64(d.inp['g'][:, :F])).max())
    sg = np.nextafter(sg, np.float32(np.inf))              # (what gpe_edge_bwd_point_sums hands over: not below the true maximum)
    a3 = np.float32(np.nanmax(d.out0['a3'][:, :F]))
    c = _case('gpe_edge_dz3_bound', dict(F=F, seed=seed), dict(amax_sg=word(sg), coef=d.inp['coef'], amax_a3=word(a3)),
              dict(word=np.array([0xFFFFFFFF], np.uint32)))
    c.dz3_max = float(np.abs(_ref_dz3(d)[0]).max())
    return c


def _ref_edge_dz3_bound(case, variant=None):
    _, c1, k2, mean = f64(case.inp['coef'])
    sg, a3 = word_value(case.inp['amax_sg']), word_value(case.inp['amax_a3'])
    a3 = a3 * (1.0 if variant == 'a3_margin_dropped' else 1.001)
    m = 0.0 if variant == 'mean_dropped' else np.abs(mean)
    tail = (np.abs(c1) + (a3 + m) * np.abs(k2)).max()
    return ((0.0 if variant == 'sg_dropped' else sg) + tail) * 1.000001


def check_edge_dz3_bound(case, got, variant=None):
    ref = _ref_edge_dz3_bound(case, variant)
    w = int(got['word'][0])
    if w >> 31:
        _fail(case, 'bound word', (0,), hex(w), None, '(sign bit set)')
    v = word_value(got['word'])
    r = _within(case, 'bound', np.array([v]), np.array([ref]), 4 * U * abs(ref))
    if not v >= case.dz3_max:
        _fail(case, 'bound', (0,), v, case.dz3_max, '(below max |dz3| of the eager reference)')
    return dict(bound=r)


def emulate_edge_dz3_bound(case, seq=False):
    return dict(word=word(np.float32(_ref_edge_dz3_bound(case))))


# ======================================================================================================================
# gpe_bn_bwd_from_G
# ======================================================================================================================
def build_bn_bwd_from_G(Cn, C, with_dw=True, seed=0):
    rng = np.random.default_rng(seed)
    inp = dict(G=padded(f32(rng.standard_normal((Cn, C))), C + 3, np.nan), db=f32(rng.standard_normal(Cn)),
               w=padded(f32(rng.standard_normal((Cn, C))), C + 1, np.nan), stats=make_stats(rng, C))
    out0 = dict(sums=np.full((2, C), SENTINEL, np.float64))
    if with_dw:
        out0['dw'] = np.full((Cn, C + 2), SENTINEL, np.float32)
    return _case('gpe_bn_bwd_from_G', dict(Cn=Cn, C=C, dw=int(with_dw), seed=seed), inp, out0)


def _ref_bn_bwd_from_G(case, variant=None):
    C, i = case.p['C'], case.inp
    st = i['stats']
    return f_bn_bwd_from_G(i['G'][:, :C], i['db'], i['w'][:, :C], st[0], st[1], st[2], st[3], variant)


def check_bn_bwd_from_G(case, got, variant=None):
    sums, mags, dw = _ref_bn_bwd_from_G(case, variant)
    C = case.p['C']
    w = dict(sums=_within(case, 'sums', got['sums'], sums, 1e-13 * mags))
    if case.p['dw']:
        w['dw'] = _within(case, 'dW', got['dw'][:, :C], dw, 2 * U * np.abs(dw))
        _untouched(case, 'dW pad', got['dw'][:, C:], case.out0['dw'][:, C:])
    return w


def emulate_bn_bwd_from_G(case, seq=False):
    sums, _, dw = _ref_bn_bwd_from_G(case)
    got = dict(sums=sums)
    if case.p['dw']:
        got['dw'] = case.out0['dw'].copy()
        got['dw'][:, :case.p['C']] = f32(dw)
    return got


# ======================================================================================================================
# the case lists of tests/test_gpu_edge_glue.py: the smallest shapes that reach each branch (see that file), and the variants
# ======================================================================================================================
KERNELS = ['edge_gather_stats', 'bn_finalize', 'bn_from_running', 'edge_finish', 'edge_sum_k', 'bn_apply', 'edge_inputs_fwd',
           'edge_bwd_point_sums', 'bn_bwd_coef', 'edge_dz3', 'edge_dz3_all', 'edge_dz3_bound', 'bn_bwd_from_G', 'knn_reverse',
           'edge_pull_dq', 'edge_inputs_bwd']
SEQ_KERNELS = ['edge_sum_k', 'edge_pull_dq', 'edge_inputs_fwd', 'edge_inputs_bwd']       # fp32 order is part of the contract

CASES = {
    # (B, N, k, H): B unpinned / pinned / uneven per XCD; k around the 8 rows in flight; H one quad .. every lane
    'edge_gather_stats': [(1, 33, 1, 4), (7, 20, 7, 64), (8, 24, 8, 200), (9, 17, 9, 256), (16, 12, 16, 64), (8, 40, 17, 200),
                          (1, 40, 64, 256), (9, 23, 64, 4)],
    # (nblk, C, count, running): nblk around the 64 row slots and the 4 x 64 chains; C around the 16 channels per workgroup
    'bn_finalize': [(1, 200, 1000.0, True), (63, 1, 1000.0, True), (64, 15, 1000.0, False), (65, 16, 1000.0, True),
                    (192, 17, 1000.0, True), (193, 257, 1000.0, False), (255, 16, 1000.0, True), (256, 15, 1000.0, True),
                    (257, 17, 1000.0, True), (512, 200, 1000.0, True), (513, 1, 1000.0, True), (64, 17, 1.0, True)],
    'bn_from_running': [(1,), (63,), (64,), (65,), (200,)],
    # (rows, C)
    'edge_finish': [(0, 150), (1, 257), (255, 1), (256, 150), (257, 257)],
    'bn_apply': [(0, 150), (1, 257), (255, 1), (256, 150), (257, 257)],
    # (npts, k, F)
    'edge_sum_k': [(1, 1, 1), (5, 5, 63), (5, 16, 64), (1, 5, 65), (5, 16, 150), (8200, 2, 3)],
    # (B, N, k, C)
    'edge_inputs_fwd': [(1, 30, 1, 1), (7, 20, 4, 3), (8, 16, 9, 5), (9, 11, 4, 1), (16, 10, 9, 3)],
    'edge_inputs_bwd': [(1, 30, 1, 1), (7, 20, 4, 3), (8, 16, 9, 5), (9, 11, 4, 1), (16, 10, 9, 3)],
    # (rows, C, word): rows around the 512 blocks and their 8 rows in flight; C around the 256 columns of a workgroup
    'edge_bwd_point_sums': [(1, 257, True), (511, 1, False), (512, 255, True), (513, 256, False), (4095, 1, True),
                            (4096, 257, False), (4097, 255, True), (4611, 256, True)],
    # (nblk, C, dgamma / dbeta given)
    'bn_bwd_coef': [(1, 200, True), (15, 1, False), (16, 63, True), (17, 64, False), (512, 65, True)],
    # (B, N, k, F, word): F around the quad and the 256 columns of a workgroup; k around the 8 rows in flight; the last: the stride loop
    'edge_dz3': [(1, 1, 1, 1, True), (1, 3, 7, 3, False), (1, 4, 8, 4, True), (1, 5, 9, 5, False), (7, 10, 16, 150, True),
                 (1, 5, 20, 200, True), (1, 4, 7, 255, False), (1, 3, 9, 256, True), (1, 5, 8, 257, True), (7, 10, 20, 260, False),
                 (1, 16390, 1, 5, True)],
    # (B, N, k, F, gscale = 1 / k?, word)
    'edge_dz3_all': [(1, 1, 1, 1, False, True), (1, 3, 7, 3, True, False), (1, 4, 8, 4, False, True), (1, 5, 9, 5, True, False),
                     (7, 10, 16, 150, True, True), (1, 5, 20, 200, False, True), (1, 4, 7, 255, True, False),
                     (1, 3, 9, 256, True, True), (1, 5, 8, 257, False, True), (7, 10, 20, 260, True, False),
                     (1, 16390, 1, 5, False, True)],
    'edge_dz3_bound': [(1,), (255,), (256,), (257,)],
    # (Cn, C, dw given): Cn around the 16 f-lanes and their two chains; C around the 64 columns of a workgroup
    'bn_bwd_from_G': [(1, 200, True), (15, 1, True), (16, 63, False), (17, 64, True), (31, 65, True), (32, 200, False),
                      (33, 1, True), (150, 63, True), (200, 200, True)],
    # (B, N, k, hub): (2 N + 1 + N k) ints within 150 KB -> sorted in LDS, else in global memory (knn_reverse_uses_lds)
    'knn_reverse': [(1, 1, 1, 0), (3, 2, 1, 0), (2, 1023, 3, 0), (2, 1024, 3, 0), (2, 1025, 3, 0), (1, 2048, 16, 0),
                    (1, 2048, 20, 0), (1, 1025, 40, 0), (2, 1024, 5, 4000)],
    # (B, N, k, H): in-degrees 0, 1, 3, 4, 5 and a hub of 300 in every cloud
    'edge_pull_dq': [(1, 40, 16, 4), (7, 40, 16, 64), (8, 40, 16, 200), (9, 40, 16, 256), (16, 33, 16, 64)],
}

VARIANTS = {
    'edge_gather_stats': ['no_relu', 'local_jg', 'clamped_slot'],
    'bn_finalize': ['biased_running_var', 'var_not_clamped', 'last_block_dropped', 'nbt_not_incremented'],
    'bn_from_running': ['eps_dropped', 't_plus'],
    'edge_finish': ['sel_s_gt0', 'always_mx'],
    'bn_apply': ['t_dropped', 'uses_rstd_row'],
    'edge_sum_k': ['slots_descending', 'last_slot_dropped', 'no_grid_stride'],
    'edge_inputs_fwd': ['xi_minus_xj', 'pad_untouched'],
    'edge_inputs_bwd': ['global_edge_ids', 'pull_first', 'g2_not_subtracted'],
    'edge_bwd_point_sums': ['sel_s_gt0', 'word_not_reset', 'xhat_no_rstd', 'tail_rows_dropped'],
    'bn_bwd_coef': ['count_minus_1', 'last_block_dropped', 'k2_no_rstd'],
    'edge_dz3': ['sel_s_gt0', 'relu_ge0', 'word_not_reset', 'quad_pad_untouched'],
    'edge_dz3_all': ['gscale_dropped', 'relu_ge0', 'word_not_reset', 'quad_pad_untouched'],
    'edge_dz3_bound': ['mean_dropped', 'a3_margin_dropped', 'sg_dropped'],
    'bn_bwd_from_G': ['rstd_dropped', 'dw_uses_t', 'last_row_dropped'],
    'knn_reverse': ['bucket_unsorted', 'rev_off_N_missing', 'global_edge_ids'],
    'edge_pull_dq': ['global_edge_ids', 'left_half_overwritten', 'descending_order'],
}


def case_params():
    """[(kernel, args)] of every case, for pytest.mark.parametrize"""
    return [(k, a) for k in KERNELS for a in CASES[k]]


_BUILT = {}


def build(kernel, args):
    """the case of CASES[kernel] with these arguments (built once: its inputs are shared and left unchanged)"""
    key = (kernel, tuple(args))
    if key not in _BUILT:
        seed = 1000 * KERNELS.index(kernel) + CASES[kernel].index(tuple(args))
        if kernel == 'edge_dz3_all':
            B, N, k, F, inv, wd = args
            c = build_edge_dz3_all(B, N, k, F, 1.0 / k if inv else 1.0, wd, seed)
        else:
            c = globals()['build_' + kernel](*args, seed=seed)
        _BUILT[key] = c
    return _BUILT[key]


def check(case, got, variant=None):
    return globals()['check_' + case.kernel[4:]](case, got, variant)


def emulate(case, seq=False):
    return globals()['emulate_' + case.kernel[4:]](case, seq)


def abi_args(case, d):
    """the argument list of the call (include/gpe_hip.h), without the stream; d = {name: device tensor}, absent = NULL"""
    p, K = case.p, case.kernel
    g = d.get
    if K == 'gpe_edge_gather_stats':
        return [d['pq'], 2 * p['H'] + 4, p['H'], d['jg'], p['B'], p['N'], p['k'], d['part']]
    if K == 'gpe_bn_finalize':
        return [d['part'], p['nblk'], p['C'], float(p['count']), d['gamma'], d['beta'], p['eps'], p['momentum'], g('rm'), g('rv'),
                g('nbt'), d['stats']]
    if K == 'gpe_bn_from_running':
        return [d['rm'], d['rv'], p['C'], d['gamma'], d['beta'], p['eps'], d['stats']]
    if K == 'gpe_edge_finish':
        return [d['mx'], d['mn'], p['C'] + 3, d['stats'], p['rows'], p['C'], d['y'], p['C'] + 2]
    if K == 'gpe_bn_apply':
        return [d['a'], p['C'] + 3, d['stats'], p['rows'], p['C'], d['y'], p['C'] + 2]
    if K == 'gpe_edge_sum_k':
        return [d['a'], p['F'] + 3, p['npts'], p['k'], p['F'], d['out'], p['F'] + 2]
    if K == 'gpe_edge_inputs_fwd':
        return [d['x'], p['C'] + 1, p['C'], d['jg'], p['B'] * p['N'], p['k'], d['out'], p['ldo']]
    if K == 'gpe_edge_inputs_bwd':
        return [d['g'], round_up(2 * p['C'], 4) + 4, p['C'], d['rev_off'], d['rev_edge'], p['B'], p['N'], p['k'], d['gx'], p['C'] + 2]
    if K == 'gpe_edge_bwd_point_sums':
        return [d['g'], p['C'] + 1, d['mx'], d['mn'], p['C'] + 3, d['stats'], p['rows'], p['C'], d['part'], g('word')]
    if K == 'gpe_bn_bwd_coef':
        return [d['part'], p['nblk'], d['stats'], p['C'], float(p['count']), d['coef'], g('dgamma'), g('dbeta')]
    if K == 'gpe_edge_dz3':
        ld = round_up(p['F'], 4) + 4
        return [d['a3'], ld, d['g'], p['F'] + 1, d['amx'], d['amn'], ld, d['coef'], p['B'], p['N'], p['k'], p['F'], g('word')]
    if K == 'gpe_edge_dz3_all':
        return [d['a3'], round_up(p['F'], 4) + 4, d['g'], p['F'] + 1, p['gscale'], d['coef'], p['B'], p['N'], p['k'], p['F'], g('word')]
    if K == 'gpe_edge_dz3_bound':
        return [d['amax_sg'], d['coef'], p['F'], d['amax_a3'], d['word']]
    if K == 'gpe_bn_bwd_from_G':
        return [d['G'], p['C'] + 3, d['db'], d['w'], p['C'] + 1, p['Cn'], p['C'], d['stats'], d['sums'], g('dw'), p['C'] + 2]
    if K == 'gpe_knn_reverse':
        return [d['idx'], p['B'], p['N'], p['k'], d['rev_off'], d['rev_edge']]
    if K == 'gpe_edge_pull_dq':
        return [d['dz'], p['H'] + 4, d['rev_off'], d['rev_edge'], p['B'], p['N'], p['k'], p['H'], d['dpq'][:, p['H']:], 2 * p['H']]
    raise KeyError(K)

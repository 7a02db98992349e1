"""Test infrastructure: the dense Linear kernels (csrc/gpe_rowgemm.hip, gpe_smallgemm.hip, gpe_gemm_x6.hip) and the weight packer
(csrc/gpe_pack.hip) restated rung by rung, in the shape of tests/edge_glue_restate.py.

gpe_linear is a ladder (include/gpe_hip.h gpe_linear_path names the rungs): the bf16-pipe kernel (100, f16x3 mode only), the K <= 8
streaming-store kernel (200), the single-stage kernel with 16- or 64-column blocks (301, 304) and the streaming kernel with 16 NT
columns per block (404 .. 416).  gpe_linear_splitk is a fifth entry into the single-stage kernel, one K slab of 256 per workgroup.

A case is one call: `build` lays out its host buffers at padded pitches — every column of A, of the addend and of the source weight
that the kernel must not read holds NaN (the A rows from column K on, the quad [K, round4(K)) of the bf16-pipe kernel included: it
loads the quad whole and must mask it), the packed-weight buffer is NaN before gpe_pack_weight fills it, and ALL of y outside the
valid elements holds a sentinel that must come back untouched (pad columns, rows >= M, the unused slot of two-level rows).
`check(case, got, variant=None)` compares element by element against fp64, `emulate(case)` is what a correct kernel returns (an
fp32 restatement in one plausible order; for rung 100 it carries the three-term bf16 split), `abi_args(case, d)` is the C-ABI
argument list.  `variant=` makes the REFERENCE wrong in one plausible way; tests/test_linear_host.py asserts that every bar
accepts `emulate` and that every variant is rejected by at least one case.

THE BARS, in units of u = 2^-24 times mag = sum_k |a_k w_k| + |bias| + |addend| (per element), derived from the arithmetic:

  exact kernels   A term of the sum passes through at most one rounding of its product, K - 1 fp32 additions of the accumulation
                  (the first lands in a zero accumulator, exactly) and the two epilogue additions (bias, addend), in whatever order
                  the kernel takes them: n = 1 + (K - 1) + 2 = K + 2 roundings, each at most u relative to a partial sum that mag
                  bounds.  bar = gamma(K + 2) mag, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability, lemma 3.1).  ReLU is
                  1-Lipschitz and exact.  The fused multiply-adds of the K <= 8 kernel round less often.
  gpe_linear_splitk   partial z is the bare product over its slab of ks <= 256: n = 1 + (ks - 1) = ks, against the slab's own mag.
  rung 100        x = h + m + l in bf16, each term the round-to-nearest of what the previous ones left: 8 + 8 + 8 = 24 significand
                  bits, so the split is exact, with |m| <= 2^-8 |x| and |l| <= 2^-16 |x|.  A product of two bf16 values has 16
                  significand bits: the six partial products per k are exact in fp32.  What the kernel drops per product is
                  m l + l m + l l <= (2 x 2^-24 + 2^-32) |a w| (the terms include/gpe_hip.h names): 2 u mag, rounded up.  What it
                  adds: 6 K exact partial products in fp32 in any order, then bias and addend: at most (6 K - 1) + 2 roundings, each
                  relative to a partial sum bounded by sum |partial products| <= (1 + 2^-8 + 2^-16)^2 mag <= (1 + 2^-6) mag.
                  n = 6 K + 1 + 2 = 6 K + 3, bar = gamma(6 K + 3) (1 + 2^-6) mag.
  gpe_pack_weight bit for bit: one fp32 multiplication by col_scale at most, zeros elsewhere.

Nothing here is tuned: a random two-term split (x = h + m) stays inside the rung-100 bar, because the bar allows 6 K roundings where
the hardware needs far fewer; the case 16384x256x32-lowbits therefore has operands 1 + 2^-9 (1 + j / 128) + 2^-17 - 2^-23, whose
third term l = 2^-17 - 2^-23 is as large as a third term gets and has one sign: dropping it loses 2 x 2^-17 x 0.98 of every product,
1.26 bars at K = 32.

NumPy only: no GPU and no gpe_amd."""
import collections
import types

import numpy as np

U = 2.0 ** -24
SENTINEL = -777.25
BM, KSLAB = 64, 256

# gpe_linear_path's codes
X6, SMALLK, SINGLE1, SINGLE4 = 100, 200, 301, 304
STREAM = {4: 404, 7: 407, 10: 410, 13: 413, 16: 416}
ALL_CODES = (X6, SMALLK, SINGLE1, SINGLE4) + tuple(STREAM.values())
# columns a workgroup owns on each rung: where a bias index without its block offset goes wrong
BLOCK_COLS = {X6: 128, SMALLK: 256, SINGLE1: 16, SINGLE4: 64, 404: 64, 407: 112, 410: 160, 413: 208, 416: 256}

A_INNER, AD_INNER, Y_INNER = 5, 3, 7       # two-level rows: r lives at (r / inner) * (inner + 1) * ld + (r % inner) * ld; one slot unused


def cdiv(a, b):
    return (a + b - 1) // b


def round_up(x, m):
    return (x + m - 1) // m * m


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def f64(x):
    return np.asarray(x, dtype=np.float64)


def bits(x):
    return f32(x).view(np.uint32)


def gamma(n):
    return n * U / (1.0 - n * U)


def bar_factor(K, x6):
    """the bar of one output element in units of its mag (derivation: the module's docstring)"""
    return gamma(6 * K + 3) * (1 + 2.0 ** -6) if x6 else gamma(K + 2)


def pack_kpad(K):
    """K extent of a packed weight: whole 16-k chunks, (96, 160) -> 160 and (160, 208) -> 208"""
    k16 = round_up(K, 16)
    return 160 if 96 < k16 < 160 else 208 if 160 < k16 < 208 else k16


def packed_size(N, K):
    return round_up(N, 16) * pack_kpad(K)


class Case(types.SimpleNamespace):
    """kernel, group, id, p (scalars), inp {name: array the call reads}, out0 {name: array it writes, pre-filled}"""


# ----------------------------------------------------------------------------------------------------------------------
# comparison helpers: a failure names the kernel, the case, the output and the first offending index
# ----------------------------------------------------------------------------------------------------------------------
def _fail(case, what, idx, got, ref, extra=''):
    raise AssertionError('%s[%s] %s at %s: got %r, reference %r %s' % (case.kernel, case.id, what, tuple(int(i) for i in idx), got, ref, extra))


def _within(case, what, got, ref, bar):
    """|got - ref| <= bar element by element (a NaN fails) -> the worst |diff| / bar"""
    got, ref, bar = f64(got), f64(ref), f64(bar)
    assert got.shape == ref.shape == bar.shape, (case.kernel, case.id, what, got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    diff = np.abs(got - ref)
    bad = ~(diff <= bar)
    if bad.any():
        idx = np.argwhere(bad)[0]
        t = tuple(idx)
        _fail(case, what, idx, got[t], ref[t], '|diff| %.3e > bar %.3e (%.2f bars)' % (diff[t], bar[t], diff[t] / bar[t] if bar[t] > 0 else np.inf))
    pos = bar > 0
    return float((diff[pos] / bar[pos]).max()) if pos.any() else 0.0


def _same_bits(case, what, got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, (case.kernel, case.id, what, got.shape, ref.shape)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    if bad.any():
        idx = np.argwhere(bad)[0]
        t = tuple(idx)
        _fail(case, what, idx, got[t], ref[t], '(bits differ)')


# ----------------------------------------------------------------------------------------------------------------------
# buffers
# ----------------------------------------------------------------------------------------------------------------------
def _rows(kind, M, cols, inner2, extra_rows=0):
    """one operand's rows -> dict(off, so, si, inner, size, start [M]): 'plain' 16-byte aligned rows at pitch round4(cols) + 4,
    'pitch1' a pitch that is no multiple of 4, 'base1' a base one float past alignment, 'two' two-level rows with an unused slot"""
    ld = round_up(cols, 4) + 4 + (1 if kind == 'pitch1' else 0)
    off = 1 if kind == 'base1' else 0
    r = np.arange(M, dtype=np.int64)
    if kind == 'two':
        so, si, inner = (inner2 + 1) * ld, ld, inner2
        nrows = cdiv(max(M, 1), inner2) * (inner2 + 1)
        start = (r // inner2) * so + (r % inner2) * si
    else:
        assert kind in ('plain', 'pitch1', 'base1'), kind
        so, si, inner, nrows = ld, 0, 0, M + extra_rows
        start = r * so
    return dict(off=off, so=so, si=si, inner=inner, size=off + nrows * ld + 8, start=start + off)


def _split_bf16(x):
    """the planes h, m, l of SplitBf16x3 (csrc/gpe_edgegemm_split_kernel.h): round to nearest even, thrice"""
    def rn(v):
        b = f32(v).view(np.uint32)
        return ((b + (((b >> 16) & 1) + 0x7FFF)) & np.uint32(0xFFFF0000)).view(np.float32)
    x = f32(x)
    h = rn(x)
    r = (x - h).astype(np.float32)
    m = rn(r)
    s = (r - m).astype(np.float32)
    return h, m, rn(s)


# ----------------------------------------------------------------------------------------------------------------------
# gpe_linear
# ----------------------------------------------------------------------------------------------------------------------
Lin = collections.namedtuple('Lin', 'M N K path path4 bias addend act a ad y kind scale')


def L(M, N, K, path, path4=None, bias=1, addend=0, act=0, a='plain', ad='plain', y='plain', kind='randn', scale=1.0):
    """one gpe_linear call.  path / path4: the gpe_linear_path code the case is written for in math mode 0 / 4"""
    return Lin(M, N, K, path, path if path4 is None else path4, bias, addend, act, a, ad, y, kind, scale)


def _lin_id(s):
    out = '%dx%dx%d' % (s.M, s.N, s.K)
    out += '-' + ''.join(c for c, on in zip('bar', (s.bias, s.addend, s.act)) if on) if (s.bias or s.addend or s.act) else ''
    for tag, v in (('A', s.a), ('AD', s.ad), ('Y', s.y)):
        if v != 'plain':
            out += '-%s%s' % (tag, v)
    if s.kind != 'randn':
        out += '-' + s.kind
    if s.scale != 1.0:
        out += '-x%g' % s.scale
    return out


def build_linear(s, seed, x6=False):
    rng = np.random.default_rng(seed)
    M, N, K = s.M, s.N, s.K
    ra = _rows(s.a, M, K, A_INNER)
    rad = _rows(s.ad, M, N, AD_INNER)
    ry = _rows(s.y, M, N, Y_INNER, extra_rows=2)
    if s.kind == 'lowbits':
        def low(shape):
            return f32(1.0 + 2.0 ** -9 * (1 + rng.integers(0, 128, size=shape) / 128.0) + 2.0 ** -17 - 2.0 ** -23)
        A, W = low((M, K)), low((N, K))
    else:
        A = f32(rng.standard_normal((M, K)) * s.scale)
        W = f32(rng.standard_normal((N, K)) / np.sqrt(K))
    a = np.full(ra['size'], np.nan, np.float32)
    a[ra['start'][:, None] + np.arange(K)] = A
    ldw = K + 3
    w = np.full((N, ldw), np.nan, np.float32)
    w[:, :K] = W
    inp = {'a': a, 'w': w}
    if s.bias:
        inp['bias'] = np.full(N + 4, np.nan, np.float32)
        inp['bias'][:N] = rng.standard_normal(N)
    if s.addend:
        ad = np.full(rad['size'], np.nan, np.float32)
        ad[rad['start'][:, None] + np.arange(N)] = rng.standard_normal((M, N)) * s.scale
        inp['addend'] = ad
    out0 = {'wp': np.full(packed_size(N, K) + 8, np.nan, np.float32), 'y': np.full(ry['size'], SENTINEL, np.float32)}
    c = Case(kernel='gpe_linear', id=_lin_id(s), spec=s, p=dict(M=M, N=N, K=K, act=s.act, ldw=ldw), inp=inp, out0=out0,
             ra=ra, rad=rad, ry=ry, x6=x6, y_idx=ry['start'][:, None] + np.arange(N))
    c.native_path = s.path4 if c.x6 else s.path
    return c


def _lin_operands(case):
    """fp32 A [M][K], W [N][K], bias [N] or None, addend [M][N] or None, as the call's buffers hold them"""
    if not hasattr(case, '_ops'):
        p = case.p
        A = case.inp['a'][case.ra['start'][:, None] + np.arange(p['K'])]
        W = case.inp['w'][:, :p['K']]
        b = case.inp['bias'][:p['N']] if 'bias' in case.inp else None
        ad = case.inp['addend'][case.rad['start'][:, None] + np.arange(p['N'])] if 'addend' in case.inp else None
        case._ops = (f32(A), f32(W), b, ad)
    return case._ops


# variants that leave a case's reference as it is are skipped by the host test (no case can reject them there)
def variant_applies(case, variant):
    s = case.spec
    if case.kernel == 'gpe_pack_weight':
        p = case.p
        return {'pad_nonzero': True, 'scale_by_n': p['cs'] and p['K'] > 1, 'kpad_round16': pack_kpad(p['K']) != round_up(p['K'], 16),
                'not_transposed': bool(p['transpose']) and p['N'] > 1 and p['K'] > 1}[variant]
    if case.kernel == 'gpe_linear_splitk':
        return {'partial_zero': s.K > KSLAB, 'drop_last_k': True, 'last_row_dup': s.M > 1, 'past_N': True}[variant]
    return {'drop_last_k': True, 'drop_slab2': s.K > KSLAB, 'bias_no_block_offset': bool(s.bias) and s.N > BLOCK_COLS[case.native_path],
            'addend_inner0': bool(s.addend) and s.ad == 'two' and s.M > AD_INNER, 'relu_before_addend': bool(s.act and s.addend),
            'no_relu': bool(s.act), 'last_row_dup': s.M % BM != 0 and s.M > 1, 'last_quad_shift': s.N % 4 != 0 and s.N > 1,
            'past_N': s.M > 0, 'x6_two_term': case.x6}[variant]


def _ref_linear(case, variant=None, path=None):
    """-> y [M][N] and mag [M][N] in fp64 (np.longdouble would change nothing: the fp64 error of the sum is 2^-29 of the bar)"""
    s = case.spec
    if variant is None:
        if not hasattr(case, '_ref'):
            case._ref = _ref_linear(case, '')
        return case._ref
    A, W, b, ad = _lin_operands(case)
    if variant == 'x6_two_term':
        A, W = [f64(h) + f64(m) for h, m, _ in (_split_bf16(A), _split_bf16(W))]
    A, W = f64(A), f64(W)
    if variant == 'drop_last_k':
        A = A.copy()
        A[:, -1] = 0.0
    if variant == 'drop_slab2':
        A = A.copy()
        A[:, KSLAB:2 * KSLAB] = 0.0
    y = A @ W.T
    mag = np.abs(A) @ np.abs(W).T
    if b is not None:
        bb = f64(b)
        if variant == 'bias_no_block_offset':
            bb = bb[np.arange(s.N) % BLOCK_COLS[case.native_path if path is None else path]]
        y = y + bb
        mag = mag + np.abs(f64(b))
    relu_done = False
    if ad is not None:
        add = f64(ad)
        if variant == 'addend_inner0':
            rows = (case.rad['off'] + np.arange(s.M, dtype=np.int64) * case.rad['so']) % (case.inp['addend'].size - s.N)
            add = f64(case.inp['addend'][rows[:, None] + np.arange(s.N)])
        if variant == 'relu_before_addend' and s.act:
            y = np.maximum(y, 0.0)
            relu_done = True
        y = y + add
        mag = mag + np.abs(f64(ad))
    if s.act and not relu_done and variant != 'no_relu':
        y = np.maximum(y, 0.0)
    if variant == 'last_row_dup':
        y[-1] = y[-2]
    if variant == 'last_quad_shift':
        q0 = (s.N - 1) // 4 * 4
        y[:, q0:] = np.roll(y, 1, axis=1)[:, q0:]
    return y, mag


def check_linear(case, got, variant=None, x6=None, path=None):
    """x6: hold the result against the bf16-pipe bar (default: the case's native rung); path: the code of the run that is checked"""
    s = case.spec
    x6 = case.x6 if x6 is None else x6
    ref, mag = _ref_linear(case, variant, path)
    y = got['y']
    assert y.shape == case.out0['y'].shape and y.dtype == np.float32
    worst = _within(case, 'y', y[case.y_idx], ref, bar_factor(s.K, x6) * mag)
    keep = np.ones(y.size, bool)
    keep[case.y_idx] = False
    if variant == 'past_N':                                  # the wrong reference has one element behind the last row's N columns written
        q = int(case.y_idx[-1, -1]) + 1
        if bits(y[q:q + 1])[0] == bits([SENTINEL])[0]:
            _fail(case, 'y past N', (q,), y[q], 'a written value')
        keep[q] = False
    _same_bits(case, 'y outside the valid elements (must not be written)', y[keep], case.out0['y'][keep])
    return {'y': worst}


def _emulate_product(A, W, x6):
    """fp32 accumulator of A W^T in one plausible order: exact kernels one rounding per MFMA (4 k values: the 4-term dot in fp64,
    added to the fp32 accumulator); rung 100 per 32-wide K step the six plane products l H, h L, m M, m H, h M, h H (small terms
    first, SplitBf16x3), each an fp32 product of exact terms with fp32 sums, added to the fp32 accumulator"""
    M, K = A.shape
    acc = np.zeros((M, W.shape[0]), np.float32)
    if x6:
        Ap, Wp = _split_bf16(A), _split_bf16(W)
        for k0 in range(0, K, 32):
            for pa, pw in ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)):
                acc = (acc + Ap[pa][:, k0:k0 + 32] @ Wp[pw][:, k0:k0 + 32].T).astype(np.float32)
    else:
        for k0 in range(0, K, 4):
            acc = (acc + f64(A[:, k0:k0 + 4]) @ f64(W[:, k0:k0 + 4]).T).astype(np.float32)
    return acc


def emulate_linear(case, x6=None):
    s = case.spec
    if not hasattr(case, '_emu'):
        case._emu = {}
    x6 = case.x6 if x6 is None else x6
    if x6 not in case._emu:
        A, W, b, ad = _lin_operands(case)
        v = _emulate_product(A, W, x6)
        if b is not None:
            v = (v + b).astype(np.float32)
        if ad is not None:
            v = (v + ad).astype(np.float32)
        if s.act:
            v = np.maximum(v, np.float32(0))
        y = case.out0['y'].copy()
        y[case.y_idx] = v
        case._emu[x6] = {'y': y}
    return case._emu[x6]


# ----------------------------------------------------------------------------------------------------------------------
# gpe_linear_splitk: y[z][M][N] = A[:, 256 z : 256 (z + 1)] W[:, same]^T
# ----------------------------------------------------------------------------------------------------------------------
Spl = collections.namedtuple('Spl', 'M N K a')


def build_linear_splitk(s, seed):
    rng = np.random.default_rng(seed)
    M, N, K = s.M, s.N, s.K
    ra = _rows(s.a, M, K, A_INNER)
    nz = cdiv(K, KSLAB)
    a = np.full(ra['size'], np.nan, np.float32)
    a[ra['start'][:, None] + np.arange(K)] = rng.standard_normal((M, K))
    w = np.full((N, K + 3), np.nan, np.float32)
    w[:, :K] = rng.standard_normal((N, K)) / np.sqrt(K)
    out0 = {'wp': np.full(packed_size(N, K) + 8, np.nan, np.float32), 'y': np.full(nz * M * N + 2 * N + 8, SENTINEL, np.float32)}
    return Case(kernel='gpe_linear_splitk', id='%dx%dx%d%s' % (M, N, K, '' if s.a == 'plain' else '-A' + s.a), spec=s,
                p=dict(M=M, N=N, K=K, ldw=K + 3, nz=nz), inp={'a': a, 'w': w}, out0=out0, ra=ra, x6=False, native_path=SINGLE4)


def _ref_linear_splitk(case, variant=None):
    p = case.p
    A = f64(case.inp['a'][case.ra['start'][:, None] + np.arange(p['K'])])
    W = f64(case.inp['w'][:, :p['K']])
    if variant == 'drop_last_k':
        A = A.copy()
        A[:, -1] = 0.0
    y = np.zeros((p['nz'], p['M'], p['N']))
    mag = np.zeros_like(y)
    for z in range(p['nz']):
        sl = slice(z * KSLAB, (z + 1) * KSLAB)
        y[z] = A[:, sl] @ W[:, sl].T
        mag[z] = np.abs(A[:, sl]) @ np.abs(W[:, sl]).T
    if variant == 'partial_zero':
        y[1] = 0.0
    if variant == 'last_row_dup':
        y[:, -1] = y[:, -2]
    return y, mag


def check_linear_splitk(case, got, variant=None, **_):
    p = case.p
    ref, mag = _ref_linear_splitk(case, variant)
    y = got['y']
    assert y.shape == case.out0['y'].shape and y.dtype == np.float32
    n = ref.size
    ks = np.array([min(KSLAB, p['K'] - z * KSLAB) for z in range(p['nz'])], np.float64)
    worst = _within(case, 'y', y[:n].reshape(ref.shape), ref, gamma(ks)[:, None, None] * mag)
    tail = np.arange(n, y.size)
    if variant == 'past_N':
        if bits(y[n:n + 1])[0] == bits([SENTINEL])[0]:
            _fail(case, 'y past the last partial', (n,), y[n], 'a written value')
        tail = tail[1:]
    _same_bits(case, 'y behind the partials (must not be written)', y[tail], case.out0['y'][tail])
    return {'y': worst}


def emulate_linear_splitk(case, **_):
    if not hasattr(case, '_emu'):
        p = case.p
        A = f32(case.inp['a'][case.ra['start'][:, None] + np.arange(p['K'])])
        W = f32(case.inp['w'][:, :p['K']])
        y = case.out0['y'].copy()
        for z in range(p['nz']):
            sl = slice(z * KSLAB, (z + 1) * KSLAB)
            y[z * p['M'] * p['N']:(z + 1) * p['M'] * p['N']] = _emulate_product(A[:, sl], W[:, sl], False).reshape(-1)
        case._emu = {'y': y}
    return case._emu


# ----------------------------------------------------------------------------------------------------------------------
# gpe_pack_weight: packed[((k / 4) * Npad + n) * 4 + k % 4] = w(n, k) * col_scale[k], zeros for k in [K, kpad) and n in [N, Npad)
# ----------------------------------------------------------------------------------------------------------------------
Pack = collections.namedtuple('Pack', 'N K transpose ldpad cs')


def build_pack_weight(s, seed):
    rng = np.random.default_rng(seed)
    N, K = s.N, s.K
    rows, cols = (K, N) if s.transpose else (N, K)
    ldw = cols + (3 if s.ldpad else 0)
    w = np.full((rows, ldw), np.nan, np.float32)
    w[:, :cols] = rng.standard_normal((rows, cols))
    inp = {'w': w}
    if s.cs:
        inp['col_scale'] = np.full(K + 4, np.nan, np.float32)
        inp['col_scale'][:K] = rng.standard_normal(K)
    out0 = {'wp': np.full(packed_size(N, K) + 8, np.nan, np.float32)}
    return Case(kernel='gpe_pack_weight', id='N%d-K%d%s%s%s' % (N, K, '-T' if s.transpose else '', '-ld' if s.ldpad else '', '-cs' if s.cs else ''),
                spec=s, p=dict(N=N, K=K, transpose=s.transpose, ldw=ldw, cs=s.cs), inp=inp, out0=out0, x6=False, native_path=None)


def ref_packed(w, N, K, transpose=0, col_scale=None, variant=None):
    """the whole gpe_packed_size image of the [N][K] matrix held in w (w[n][k], or w[k][n] when transposed), fp32"""
    w = f32(w)
    if transpose and variant == 'not_transposed':            # the [K][ldw] source read as if it were [N][ldw]
        W = w.reshape(-1)[(np.arange(N)[:, None] * w.shape[1] + np.arange(K)) % w.size]
    else:
        W = w[:K, :N].T if transpose else w[:N, :K]
    if col_scale is not None:
        cs = f32(col_scale)
        W = (W * (cs[np.arange(N) % K][:, None] if variant == 'scale_by_n' else cs[None, :K])).astype(np.float32)
    Npad = round_up(N, 16)
    kpad = round_up(K, 16) if variant == 'kpad_round16' else pack_kpad(K)
    full = np.full((kpad, Npad), np.nan if variant == 'pad_nonzero' else 0.0, np.float32)
    full[:K, :N] = W.T
    return np.ascontiguousarray(full.reshape(kpad // 4, 4, Npad).transpose(0, 2, 1)).reshape(-1)


def _ref_pack_weight(case, variant=None):
    p = case.p
    img = ref_packed(case.inp['w'], p['N'], p['K'], p['transpose'], case.inp.get('col_scale'), variant)
    out = case.out0['wp'].copy()
    out[:img.size] = img
    return out


def check_pack_weight(case, got, variant=None, **_):
    _same_bits(case, 'wp (the whole image and the floats behind it)', got['wp'], _ref_pack_weight(case, variant))
    return {}


def emulate_pack_weight(case, **_):
    return {'wp': _ref_pack_weight(case)}


# ----------------------------------------------------------------------------------------------------------------------
# the cases: the smallest shapes that reach each branch (thresholds: csrc/gpe_rowgemm.hip rg_linear_path, gpe_smallgemm.hip
# gpe_smallgemm_linear_nt, gpe_gemm_x6.hip gpe_gemm_x6_linear_ok).  A case stands in the group of the rung it is checked on by `check` and `emulate`: its math-mode-4 rung for the group 'x6', its
# math-mode-0 rung elsewhere (tests/test_gpu_linear.py runs every case in both modes).
# The streaming kernel's grid is gridDim.x = num_tiles: "fewer workgroups than tiles" is not reachable through gpe_linear, so no
# case pretends to cover its tile loop's second trip.
# ----------------------------------------------------------------------------------------------------------------------
def _epilogues(M, N, K, path, path4=None):
    """bias / addend / ReLU in all eight combinations, then two-level rows for A, the addend and y, each on its own"""
    out = [L(M, N, K, path, path4, bias=b, addend=a, act=r) for b in (0, 1) for a in (0, 1) for r in (0, 1)]
    out += [L(M, N, K, path, path4, addend=1, act=1, a='two'), L(M, N, K, path, path4, addend=1, act=1, ad='two'),
            L(M, N, K, path, path4, addend=1, act=1, y='two')]
    return out


S4 = STREAM[4]
CASES = {
    'single1': (
        [L(M, 17, 17, SINGLE1) for M in (1, 63, 64, 65)]
        + [L(65, N, 16, SINGLE1) for N in (1, 15, 16, 17, 250)]
        + [L(65, 17, K, SINGLE1) for K in (1, 3, 4, 15, 255, 256, 257, 520)]             # (K = 16, 17 stand above)
        # K % 4 == 0: the plain rows above take the vector staging path, a misaligned base or pitch the guarded one
        + [L(65, 17, 4, SINGLE1, a='base1'), L(65, 17, 16, SINGLE1, a='pitch1'), L(65, 17, 256, SINGLE1, a='base1'),
           L(65, 17, 520, SINGLE1, a='pitch1'), L(65, 16, 8, SINGLE1)]
        + _epilogues(65, 35, 20, SINGLE1)
        # neighbours of single-stage <4> (127 and 126 block columns) and of the N <= 16 rule
        + [L(8128, 64, 9, SINGLE1), L(4032, 128, 12, SINGLE1), L(1985, 16, 9, SINGLE1), L(1985, 17, 9, SINGLE1)]
        # what falls off the K <= 8 rung: M = 4095, K = 9, a y pitch that is no multiple of 4, a misaligned addend
        + [L(4095, 4, 3, SINGLE1), L(4096, 4, 9, SINGLE1), L(4096, 4, 3, SINGLE1, y='pitch1'), L(4096, 4, 3, SINGLE1, addend=1, ad='pitch1')]
        # what falls off the bf16-pipe rung by N = 47
        + [L(2048, 47, 1300, SINGLE1)]),
    'single4': (
        [L(1985, N, 9, SINGLE4) for N in (193, 250, 256)]                                # 32 tiles, the last of one row
        + [L(1985, 193, K, SINGLE4) for K in (255, 256, 257, 520)]
        + [L(4096, 65, 9, SINGLE4)]                                                      # 64 tiles x 2 = 128 block columns
        + _epilogues(1985, 193, 12, SINGLE4)
        + [L(4096, 150, 3, SINGLE4)]                                                     # N % 4: off the K <= 8 rung
        # off the bf16-pipe rung: M = 2047, just under the FLOP gate, A rows that are not 16-byte loadable
        + [L(2047, 400, 153, SINGLE4), L(2048, 400, 152, SINGLE4), L(2048, 400, 153, SINGLE4, a='pitch1'),
           L(2048, 400, 153, SINGLE4, a='base1')]),
    'stream': (
        [L(8129, 64, 9, S4), L(8129, 65, 9, S4), L(8129, 208, 9, STREAM[10])]           # 128 tiles: the first streaming shapes
        + [L(16321, N, 9, STREAM[nt]) for N, nt in ((33, 4), (64, 4), (65, 7), (112, 7), (113, 10), (160, 10), (161, 13), (208, 13),
                                                     (209, 16), (256, 16))]              # 256 tiles, the last of one row
        + [L(4096, 400, 9, STREAM[7]), L(8192, 400, 9, STREAM[13]), L(1601, 1000, 9, S4)]
        + [L(8129, 64, K, S4, X6) for K in (255, 256, 257, 520)]                            # (in f16x3 mode these eight are on the bf16 pipe's menu)
        + [L(8192, 400, K, STREAM[13], X6) for K in (255, 256, 257, 520)]
        + _epilogues(8129, 70, 12, S4)
        + [L(4096, 252, 3, S4, y='pitch1')]                                              # off the K <= 8 rung by its y pitch
        + [L(16384, 256, 31, STREAM[16])]),                                              # off the bf16-pipe rung by K = 31
    'smallk': (
        [L(4096, 4, K, SMALLK) for K in (1, 3, 8)]
        + [L(4096 * 32 + 5, 4, 3, SMALLK)]                                               # 4097 row groups on 4096 blocks: the stride loop
        + [L(4096, N, 3, SMALLK) for N in (252, 256, 260)]
        + _epilogues(4100, 12, 5, SMALLK)),
    'x6': (
        [L(2048, 48, 1300, SINGLE1, X6), L(16384, 256, 32, STREAM[16], X6)]              # (2048 x 400 x 153: the epilogue cases)
        # M % 128, N % 128, N % 4, K % 32, K % 4 all nonzero: scalar stores, a scalar addend, NaN behind K inside the last quad
        + [L(2050, 130, 470, SINGLE1, X6, addend=1, act=1)]
        + _epilogues(2048, 400, 153, SINGLE4, X6)
        + [L(2048, 400, 153, SINGLE4, X6, bias=0, scale=sc) for sc in (1e-25, 1e20)]       # (scale 1: the first epilogue case)
        + [L(16384, 256, 32, STREAM[16], X6, bias=0, kind='lowbits')]),
    'splitk': (
        [Spl(M, 64, 257, 'plain') for M in (1, 64, 65)]
        + [Spl(65, N, 256, 'plain') for N in (63, 64, 65)]
        + [Spl(65, 65, 1000, 'plain'), Spl(65, 63, 1000, 'pitch1'), Spl(64, 65, 256, 'base1')]),
    'pack': [Pack(N, K, t, ld, cs) for N in (1, 16, 17) for K in (1, 16, 17, 96, 97, 159, 160, 161, 207, 208, 209)
             for t in (0, 1) for ld in (0, 1) for cs in (0, 1)],
}
GROUPS = list(CASES)
LINEAR_GROUPS = ['x6', 'smallk', 'single1', 'single4', 'stream']
KERNEL_OF = {'splitk': 'linear_splitk', 'pack': 'pack_weight'}

VARIANTS = {
    'linear': ['drop_last_k', 'drop_slab2', 'bias_no_block_offset', 'addend_inner0', 'relu_before_addend', 'no_relu', 'last_row_dup',
               'last_quad_shift', 'past_N', 'x6_two_term'],
    'linear_splitk': ['partial_zero', 'drop_last_k', 'last_row_dup', 'past_N'],
    'pack_weight': ['pad_nonzero', 'scale_by_n', 'kpad_round16', 'not_transposed'],
}

# both sides of every edge of the ladder: (group, case) x 2, the codes they answer in math mode 0 / 4 are in the cases
EDGES = {
    'x6 M 2047/2048': (L(2047, 400, 153, SINGLE4), L(2048, 400, 153, SINGLE4, X6)),
    'x6 N 47/48': (L(2048, 47, 1300, SINGLE1), L(2048, 48, 1300, SINGLE1, X6)),
    'x6 K 31/32': (L(16384, 256, 31, STREAM[16]), L(16384, 256, 32, STREAM[16], X6)),
    'x6 FLOP gate': (L(2048, 400, 152, SINGLE4), L(2048, 400, 153, SINGLE4, X6)),
    'x6 A rows 16-byte loadable': (L(2048, 400, 153, SINGLE4, a='pitch1'), L(2048, 400, 153, SINGLE4, X6)),
    'small-K K 8/9': (L(4096, 4, 8, SMALLK), L(4096, 4, 9, SINGLE1)),
    'small-K M 4095/4096': (L(4095, 4, 3, SINGLE1), L(4096, 4, 3, SMALLK)),
    'small-K N % 4': (L(4096, 150, 3, SINGLE4), L(4096, 252, 3, SMALLK)),
    'small-K y pitch': (L(4096, 252, 3, S4, y='pitch1'), L(4096, 252, 3, SMALLK)),
    'small-K grid of 4096': (L(4096, 4, 3, SMALLK), L(4096 * 32 + 5, 4, 3, SMALLK)),
    'single-stage N 16/17': (L(1985, 16, 9, SINGLE1), L(1985, 17, 9, SINGLE1)),
    'single-stage 127/128 block columns': (L(8128, 64, 9, SINGLE1), L(4096, 65, 9, SINGLE4)),
    'streaming 127/128 tiles': (L(8128, 64, 9, SINGLE1), L(8129, 64, 9, S4)),
    'N 64/65': (L(16321, 64, 9, S4), L(16321, 65, 9, STREAM[7])),
    'N 112/113': (L(16321, 112, 9, STREAM[7]), L(16321, 113, 9, STREAM[10])),
    'N 160/161': (L(16321, 160, 9, STREAM[10]), L(16321, 161, 9, STREAM[13])),
    'N 208/209': (L(16321, 208, 9, STREAM[13]), L(16321, 209, 9, STREAM[16])),
    'N 256/257 (400)': (L(16321, 256, 9, STREAM[16]), L(8192, 400, 9, STREAM[13])),
    'N 400 at 64/128 tiles': (L(4096, 400, 9, STREAM[7]), L(8192, 400, 9, STREAM[13])),
    'K slab 256/257 single1': (L(65, 17, 256, SINGLE1), L(65, 17, 257, SINGLE1)),
    'K slab 256/257 single4': (L(1985, 193, 256, SINGLE4), L(1985, 193, 257, SINGLE4)),
    'K slab 256/257 narrow': (L(8129, 64, 256, S4, X6), L(8129, 64, 257, S4, X6)),
    'K slab 256/257 wide': (L(8192, 400, 256, STREAM[13], X6), L(8192, 400, 257, STREAM[13], X6)),
}


def group_of(spec):
    for g in GROUPS:
        if spec in CASES[g]:
            return g
    raise KeyError(spec)


def case_params():
    """[(group, spec)] of every case, for pytest.mark.parametrize"""
    return [(g, s) for g in GROUPS for s in CASES[g]]


def case_id(v):
    if isinstance(v, str):
        return v
    if isinstance(v, Lin):
        return _lin_id(v)
    return '-'.join(str(x) for x in v)


_BUILT = {}


def build(group, spec):
    """the case (built once: its inputs are shared and left unchanged)"""
    key = (group, spec)
    if key not in _BUILT:
        seed = 1000 * GROUPS.index(group) + CASES[group].index(spec)
        if group in LINEAR_GROUPS:
            c = build_linear(spec, seed, x6=group == 'x6')
        else:
            c = globals()['build_' + KERNEL_OF[group]](spec, seed)
        c.group = group
        _BUILT[key] = c
    return _BUILT[key]


def check(case, got, variant=None, **kw):
    return globals()['check_' + case.kernel[4:]](case, got, variant, **kw)


def emulate(case, **kw):
    return globals()['emulate_' + case.kernel[4:]](case, **kw)


def pack_args(case, d):
    """the gpe_pack_weight call that fills a Linear case's wp from its source weight [N][K + 3]"""
    p = case.p
    return [d['w'], p['ldw'], p['N'], p['K'], 0, None, d['wp']]


def abi_args(case, d):
    """the argument list of the call (include/gpe_hip.h), without the stream; d = {name: device tensor, or anything whose slice
    [off:] is the pointer}, absent = NULL"""
    p = case.p
    if case.kernel == 'gpe_pack_weight':
        return [d['w'], p['ldw'], p['N'], p['K'], p['transpose'], d.get('col_scale'), d['wp']]
    if case.kernel == 'gpe_linear_splitk':
        return [d['a'][case.ra['off']:], case.ra['so'], d['wp'], d['y'], p['M'], p['N'], p['K']]
    ra, rad, ry = case.ra, case.rad, case.ry
    ad = d.get('addend')
    return [d['a'][ra['off']:], ra['so'], ra['si'], ra['inner'], d['wp'], d.get('bias'),
            None if ad is None else ad[rad['off']:], rad['so'], rad['si'], rad['inner'],
            d['y'][ry['off']:], ry['so'], ry['si'], ry['inner'], p['M'], p['N'], p['K'], p['act']]

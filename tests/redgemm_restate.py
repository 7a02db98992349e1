"""Test infrastructure: the reduce-GEMM kernels (csrc/gpe_redgemm.hip, and the bf16-pipe TN kernel of csrc/gpe_gemm_x6.hip) restated
rung by rung, in the shape of tests/linear_restate.py.

gpe_redgemm and gpe_edge_redgemm are one ladder of eight rungs (include/gpe_hip.h gpe_redgemm_path names them):
1 thin, 2 bf16-pipe TN, 3 deep, 4 lazy dz3, 5 b3 f16x3, 6 b3 bf16x3, 7 producer/consumer, 8 big-block.  This module has

  the plan      `plan` / `path_query`: gpe_redgemm_plan and the export's refusals and amax-word settlement, written from the table
                of DESIGN.md 5.33; tests/test_redgemm_host.py holds it against gpe_redgemm_path on every case and on a seeded sweep.
  the cases     `Rd` specs, one call each, grouped by the rung they were written for (CASES); `build(spec, kind)` lays the call
                out in host buffers for the data kinds 'int' and 'rand' (below).
  the checks    `check(case, got, variant=None)` compares G, colsum and the floats behind `part` with fp64, element by element;
                `emulate(case)` is what a correct kernel returns (an fp32 restatement of the rung's partial split in one
                plausible order); `variant=` makes the REFERENCE wrong in one plausible way.

BUFFERS.  U and V sit at padded pitches in buffers of NaN: the pad columns up to and past round4(cols), 64 rows behind `rows`, the
unused slot of two-level rows, the columns of the [P|Q] table past 2 Ng.  G has pitch Ng + 5 and two rows behind Mg, colsum four
floats behind Mg: all of that holds a sentinel that must come back untouched, and the valid elements hold finite old values (used
under `accumulate`, overwritten otherwise).  `part` is gpe_redgemm_ws(Mg, Ng) floats of NaN — a workgroup that has no tile must
still write its partial, or the finish sums NaN — followed by 4096 sentinel floats.

TWO KINDS OF DATA per case.
  int    U, V, [P|Q], the shift and the old G are integers in [-4, 4] and rows <= 2^19: every partial sum is an integer below
         2^24 (|u| <= 4, |v - s| <= 8: 32 rows <= 2^24), so every summation order, in fp32 or fp64, gives the same bits.  On the split
         rungs too: such a value is its own high term (bf16 has 8 significand bits, fp16 11; the f16x3 scale is a power of two),
         the low terms are zero.  Checked for EQUALITY.  This is what catches a dropped, doubled or misplaced row, a wrong gather
         index, a skipped shift, a pad column in a column sum.
  rand   randn, V offset by +3 where a shift is used (shift = the column means: the cancellation the shift exists for).

THE BARS for random data, per element, u = 2^-24, mag = sum_r |u_r| |v_r - s| (+ |G_old| under accumulate), gamma(n) = n u / (1 - n u)
(Higham, Accuracy and Stability, lemma 3.1).  v_r is the fp32 row the kernel is given: for a gathered V that is relu(P_i + Q_j)
formed in fp32, as the forward pass stored it.
  exact rungs (1, 3, 7, 8)   a term passes through one rounding of v - s, one of its product, the n_p - 1 additions of the longest
         fp32 accumulator chain of the rung (n_p rows: restated from the plan, `chain_rows`), the fp32 write of the fp64 finish
         and the accumulate: bar = gamma(n_p + 3) mag.  (Thin: the chain of one wave, plus the fp32 write of the workgroup's partial.)
  rung 2 (TN)   the project's bf16-pipe bar (tests/linear_restate.py) with rows in the place of K: gamma(6 rows + 3) (1 + 2^-6) mag.
  rung 6 (b3 bf16x3)   the kernel's header comment: u = uh + ul, v = vh + vl, u v ~= ul vh + uh vl + uh vh, three terms.  Both splits
         round to nearest even: |x - xh| <= 2^-9 |x|, xl = rn(x - xh) leaves |e_x| <= 2^-18 |x|, |xl| <= 2^-9 (1 + 2^-9) |x|.  Dropped per
         product: ul vl + e_u v + u e_v <= 3 x 2^-18 (1 + 2^-8) |u v|.  The three plane products are exact in fp32 (8 x 8 bits) and
         summed in fp32, 3 n_p terms of total magnitude <= (1 + 2^-8)^2 mag:
         bar = (3 x 2^-18 (1 + 2^-8) + gamma(3 n_p + 3) (1 + 2^-7)) mag.
  rung 5 (b3 f16x3)    operands scaled by a power of two s with s A in [2^14, 2^15), A the amax word (V: the word + max |shift|);
         fp16 has 11 significand bits and an absolute floor of 2^-25 (half a subnormal step): |x s - h| <= 2^-11 |x s| + 2^-25,
         |e_x| <= 2^-22 |x| + 2^-25 / s <= 2^-22 |x| + 2^-39 A, |xl| <= 2^-11 |x| + 2^-39 A.  Dropped per product, as above:
         <= 3 x 2^-22 (1 + 2^-10) |u v| + 2^-39 (1 + 2^-10) (A_u |v| + A_v |u|) + 2^-78 A_u A_v; the plane products are exact (11 x 11
         bits), summed in fp32:  bar = (12 u (1 + 2^-10) + gamma(3 n_p + 3) (1 + 2^-9)) mag
                                       + 2^-39 (1 + 2^-10) (A_u sum |v - s| + A_v sum |u|) + rows 2^-78 A_u A_v.
  colsum        every kernel adds at most 8 values in fp32 before it goes to fp64 (thin: the wave's whole chain): gamma(8 + 2) sum |u|,
         thin gamma(n_p + 2) sum |u|.
Two of the wrong variants are rejected by construction and show only that the checker looks there: `read_past_rows` makes the
reference NaN (any finite result fails it), `colsum_incl_Mg` expects a written colsum[Mg] where the emulation leaves the sentinel.
The TN bar is the one the project uses for its bf16 pipe; at thousands of rows it is too wide to see a lost low split term
(2^-16 of mag against 6 rows u): on rung 2 only the integer data and the structure checks bind.
Nothing here is taken from a kernel's output; profiles/redgemm_tests.md has the figures an MI355X and the emulation reach.

NumPy only: no GPU and no gpe_amd."""
import collections
import functools
import types
import zlib

import numpy as np

U = 2.0 ** -24
SENTINEL = -777.25
PART_TAIL = 4096
TAIL_ROWS = 64
INNER = 7                                   # two-level rows: 7 rows per outer slot of 8, one slot unused

THIN, TN, DEEP, LAZY, B3F16, B3BF16, PC, BIG = 1, 2, 3, 4, 5, 6, 7, 8
RUNG_NAMES = {THIN: 'thin', TN: 'tn', DEEP: 'deep', LAZY: 'lazy', B3F16: 'b3f16', B3BF16: 'b3bf16', PC: 'pc', BIG: 'big'}
PLAN_FIELDS = ('gx', 'gy', 'gz', 'nblk', 'MgPad', 'NgPad', 'MH', 'NH', 'MT', 'vec', 'vvec', 'ql', 'num_tiles', 'rows_per_split',
               'pin_tpc', 'floats', 'cs')
EINVAL = -22


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


# ----------------------------------------------------------------------------------------------------------------------
# the plan.  An operand is (base address, outer stride, inner stride, inner); strides in floats
# ----------------------------------------------------------------------------------------------------------------------
def rows_pc(r, cols):
    base, so, si, inner = r
    return inner <= 0 and so % 4 == 0 and so >= round_up(cols, 4) and base % 16 == 0


def rows_deep(r, cols):
    base, so, si, inner = r
    if base % 16 or so % 4 or (inner > 0 and si % 4):
        return False
    return (si if inner > 0 else so) >= round_up(cols, 4) or cols % 4 == 0


def rows_x6(r, cols):
    base, so, si, inner = r
    if base == 0 or base % 16 or so % 4 or (inner > 0 and si % 4):
        return False
    return (si if inner > 0 else so) >= round_up(cols, 4)


def layout(nblk, MgPad, NgPad, want_cs):
    cs_off = round_up(nblk * MgPad * NgPad, 2)
    return cs_off + (2 * nblk * MgPad if want_cs else 0)


def _pick(need, menu):
    return next((m for m in menu if m >= need), -1)


def geometry(Mg, Ng):
    """big-block menu -> MH, NH, gy, MgPad, NgPad"""
    mt, nt = cdiv(Mg, 16), cdiv(Ng, 16)
    MH, NH = _pick(cdiv(min(mt, 14), 2), (2, 5, 7)), _pick(cdiv(nt, 2), (1, 5, 7, 8))
    gy = cdiv(mt, 2 * MH)
    return MH, NH, gy, gy * 32 * MH, round_up(Ng, 16)


def rdd_gx(Mg, Ng, num_tiles, cus):
    gx = cdiv(3 * cus, cdiv(Mg, 64) * cdiv(Ng, 64))
    gx = min(max(gx, cdiv(num_tiles, 64)), 32, num_tiles // 4)
    return max(gx, 1)


def ws_floats(Mg, Ng):
    """gpe_redgemm_ws"""
    MH, NH, gy, MgPad, NgPad = geometry(Mg, Ng)
    if NH < 0 or gy < 1:
        return -1
    terms = [layout(max(256 // gy, 1), MgPad, NgPad, True) + 8,
             layout(32, round_up(Mg, 64), round_up(Ng, 64), True) + 8,
             layout(32, round_up(Mg, 128), round_up(Ng, 128), True) + 8 + 1024]
    if Ng <= 4:
        terms.append(layout(512, round_up(Mg, 4), 4, True) + 8)
    return max(terms)


def settle_words(math, rows, min_rows, has_u, has_v, gathered, has_ws):
    """gpe_edge_redgemm in front of the plan: does the plan see both amax words"""
    if math != 2 or not has_u or rows < min_rows:
        return False
    return bool(has_v or (gathered and has_ws))


def plan(u, v, rows, Mg, Ng, dense, k, pin, words, lazy, want_cs, math, debug, cus):
    """-> (path, {PLAN_FIELDS}) or (-22, None).  math: 0 exact, 1 bf16x3, 2 f16x3 (the reduce-GEMMs' reading of the mode)"""
    o = dict.fromkeys(PLAN_FIELDS, 0)
    o['vec'] = int(rows_pc(u, Mg) and (not dense or rows_pc(v, Ng)))
    MH, NH, gy, MgPad, NgPad = geometry(Mg, Ng)
    if NH < 0:
        return EINVAL, None
    o['MH'], o['NH'] = MH, NH
    nt = o['num_tiles'] = cdiv(rows, 32)
    cusx = min(cus, 256)
    gx = min(max(cusx // gy, 1), nt) if nt > 0 else 1
    edge = cdiv(Ng, 16) == 13 and cdiv(Mg, 16) in (10, 13) and gy == 1

    def image(nblk, mp, np_, cs):
        o.update(nblk=nblk, MgPad=mp, NgPad=np_, cs=int(cs), floats=layout(nblk, mp, np_, cs))

    if dense and not lazy and Ng <= 4 and Mg <= 1024 and rows >= 4096 and u[3] <= 0 and v[3] <= 0 and rows_pc(u, Mg):
        image(min(rows // 64, 512), round_up(Mg, 4), 4, want_cs)
        o.update(gx=o['nblk'], gy=1, gz=1, ql=cdiv(o['MgPad'], 256))
        return THIN, o
    if (dense and math == 2 and not lazy and not debug & 16384 and not (edge and words) and 32 <= rows < 2 ** 31 and Mg >= 48 and Ng >= 48
            and 2.0 * rows * Mg * Ng >= 2.0e6 and rows_x6(u, Mg) and rows_x6(v, Ng)):
        S = max(min(cus // (cdiv(Mg, 128) * cdiv(Ng, 128)), 32, rows // 128), 1)
        rps = round_up(cdiv(rows, S), 32)
        S = cdiv(rows, rps)
        image(S, round_up(Mg, 128), round_up(Ng, 128), want_cs)
        o.update(gx=S, gy=o['MgPad'] // 128, gz=o['NgPad'] // 128, rows_per_split=rps)
        return TN, o
    in_max = max(u[3], v[3], 1)
    edge_deep = edge and rows_pc(u, Mg) and rows_pc(v, Ng) and nt >= 4 * gx
    if (dense and math != 1 and not lazy and not edge_deep and 0 < nt < 64 * gx and rows * in_max < 2 ** 32 and rows < 2 ** 31
            and rows_deep(u, Mg)):
        image(rdd_gx(Mg, Ng, nt, cusx), round_up(Mg, 64), round_up(Ng, 64), want_cs)
        o.update(gx=o['nblk'], gy=o['MgPad'] // 64, gz=o['NgPad'] // 64, vvec=int(rows_deep(v, Ng)))
        return DEEP, o
    image(gx, MgPad, NgPad, True)
    o.update(gx=gx, gy=gy, gz=1, MT=cdiv(Mg, 16))
    pc_ok = edge and rows_pc(u, Mg) and (not dense or rows_pc(v, Ng)) and nt >= 4 * gx and (dense or (k > 1 and rows * k < 2 ** 32))
    if pc_ok and not dense and pin >= 8 and pin % 8 == 0:
        rpc = rows // pin
        if rpc % 32 == 0 and gx % 8 == 0 and rpc // 32 >= gx // 8:
            o['pin_tpc'] = rpc // 32
    if lazy:
        return (LAZY, o) if pc_ok and math == 2 and words and dense and k == 16 and rows % 16 == 0 else (EINVAL, None)
    if pc_ok and math == 2 and words:
        return B3F16, o
    if pc_ok and math == 1:
        return B3BF16, o
    return (PC if pc_ok else BIG), o


def path_query(args, math_mode, debug, min_rows, cus):
    """gpe_redgemm_path restated: args as the export takes them (without plan_out), the process state beside them"""
    (ub, uso, usi, uin, vb, vso, vsi, vin, rows, Mg, Ng, v_mode, k, pin, has_u, has_v, has_ws, lazy, want_cs) = args
    math = {1: 1, 4: 2}.get(math_mode, 0)
    if v_mode not in (0, 1) or not ub or not vb or Mg <= 0 or Ng <= 0 or Ng > 256:
        return EINVAL, None
    words = False
    if k == 0:
        if v_mode != 1 or lazy or rows < 0:
            return EINVAL, None
    else:
        if uin > 0 or vin > 0 or k < 0 or pin <= 0 or rows <= 0 or rows % (pin * k) or rows >= 2 ** 31:
            return EINVAL, None
        if uso < Mg or (v_mode == 0 and (Ng % 4 or vso % 4)) or (v_mode == 1 and vso < Ng):
            return EINVAL, None
        if lazy and (k != 16 or v_mode != 1 or not has_u or not has_v):
            return EINVAL, None
        usi = vsi = uin = vin = 0
        words = settle_words(math, rows, min_rows, has_u, has_v, v_mode == 0, has_ws)
    v = (vb, vso, vsi, vin) if v_mode == 1 else (0, vso, 0, 0)
    return plan((ub, uso, usi, uin), v, rows, Mg, Ng, v_mode == 1, k, pin, words, bool(lazy), bool(want_cs), math, debug, cus)


def wg_tiles(pl, B):
    """the row tiles each partial's workgroup sums, in its order (rungs 3 - 8) -> list of int arrays"""
    nt, gx, tpc = pl['num_tiles'], pl['gx'], pl['pin_tpc']
    if not tpc:
        return [np.arange(b, nt, gx) for b in range(gx)]
    step, out = gx // 8, []
    for b in range(gx):
        seq = np.arange(b >> 3, (B // 8) * tpc, step)                   # position in XCD (b & 7)'s list of clouds b & 7, + 8, ...
        out.append(((b & 7) + 8 * (seq // tpc)) * tpc + seq % tpc)
    return out


def chain_rows(path, pl, rows, B=0):
    """n_p: the rows of the longest fp32 accumulator chain"""
    if path == THIN:
        return cdiv(cdiv(rows, pl['gx']), 4) + 1                        # + the fp32 write of the workgroup's partial
    if path == TN:
        return min(pl['rows_per_split'], rows)
    return max(1, min(rows, 32 * max(len(t) for t in wg_tiles(pl, B))))


# ----------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------
Rd = collections.namedtuple('Rd', 'rung rows Mg Ng entry gather k B math res u v shift colsum acc words debug')


def C(rung, rows, Mg, Ng, entry='redgemm', gather=0, k=0, B=0, math=0, res=192, u='plain', v='plain', shift=0, colsum=1, acc=0, words='none',
      debug=0):
    """one call.  entry 'redgemm' (k = 0) or 'edge' (B clouds of rows / (B k) points); math: gpe_math_set's mode (0, 1, 4); res: CUs
    reserved; u / v: 'plain' (aligned, pitch round4 + 4), 'tight' (pitch = cols), 'pitch1' (pitch round4 + 5), 'base1' (one float past
    alignment), 'two' (two-level rows); words: 'none', 'both' (gathered: V's word from gpe_edge_pq_amax), 'ws' (V's word NULL, workspace)"""
    if entry == 'edge':
        k, B = k or 1, B or 1
        assert rows % (k * B) == 0 and not acc, (rows, k, B)
    assert not gather or (entry == 'edge' and Ng % 4 == 0)
    return Rd(rung, rows, Mg, Ng, entry, gather, k, B, math, res, u, v, shift, colsum, acc, words, debug)


def case_id(s):
    if not isinstance(s, Rd):
        return str(s)
    out = '%s-%dx%dx%d' % (RUNG_NAMES[s.rung], s.rows, s.Mg, s.Ng)
    out += '-edge' if s.entry == 'edge' and not s.gather else ''
    out += '-g%d' % s.k if s.gather else ''
    out += '-B%d' % s.B if s.B > 1 else ''
    out += '-m%d' % s.math if s.math else ''
    out += '-r%d' % s.res if s.res != 192 else ''
    for tag, val in (('U', s.u), ('V', s.v)):
        out += '-%s%s' % (tag, val) if val != 'plain' else ''
    out += ''.join(t for t, on in (('-sh', s.shift), ('-nocs', not s.colsum), ('-acc', s.acc)) if on)
    out += '-' + s.words if s.words != 'none' else ''
    out += '-d%d' % s.debug if s.debug else ''
    return out


def _edge3(rows, Mg, Ng, rung, math, **kw):
    """an edge shape on rungs 5 / 6 / 7: dense through both entry points (f16x3: the edge entry alone carries words), gathered k 15, 16"""
    w = dict(words='both') if math == 4 else {}
    r15, r16 = rows // 15 * 15, round_up(rows, 16)
    out = [C(rung, rows, Mg, Ng, entry='edge', math=math, shift=1, **w, **kw)]
    if math != 4:
        out.append(C(rung, rows, Mg, Ng, math=math, acc=1, **kw))
    if Ng % 4 == 0:
        out += [C(rung, r15, Mg, Ng, entry='edge', gather=1, k=15, math=math, **w, **kw),
                C(rung, r16, Mg, Ng, entry='edge', gather=1, k=16, math=math, shift=1, **dict(w, words='ws') if math == 4 else {}, **kw)]
    return out


def _edge_cases(rung, math):
    return (_edge3(8205, 150, 200, rung, math) + _edge3(8192, 145, 193, rung, math) + _edge3(32781, 200, 200, rung, math)
            + _edge3(32781, 200, 200, rung, math, res=0)[:1]
            + [C(rung, 8205, 150, 200, entry='edge', math=math, colsum=0, **(dict(words='both') if math == 4 else {})),
               # pinned: 8 clouds, rows per cloud a multiple of 32 (33 and 45 tiles per cloud against gx / 8 = 8)
               C(rung, 8 * 66 * 16, 200, 200, entry='edge', gather=1, k=16, B=8, math=math, shift=1, **(dict(words='both') if math == 4 else {})),
               C(rung, 8 * 96 * 15, 150, 200, entry='edge', gather=1, k=15, B=8, math=math, **(dict(words='ws') if math == 4 else {}))])


BIG_MG = {2: (1, 64), 5: (65, 160), 7: (161, 224, 225)}                   # MH class -> the Mg values at its edges (225: gy 2)
BIG_NG = {1: (5, 32), 5: (33, 160), 7: (161, 224), 8: (225, 256)}          # NH class -> the Ng values at its edges


def _big_dense():
    """dense, math mode 1 (the deep rung is closed to bf16x3), 96 .. 300 rows: the twelve (MH, NH) instances, each with vec 1 and vec 0;
    over the four NH classes and the two loaders every Mg of BIG_MG occurs, over the three MH classes and the loaders every Ng of BIG_NG"""
    out, i = [], 0
    for mi, ms in enumerate(BIG_MG.values()):
        for ni, ns in enumerate(BIG_NG.values()):
            for vec in (1, 0):
                Mg, Ng, rows = ms[(ni + vec) % len(ms)], ns[(mi + vec) % len(ns)], (96, 131, 300, 257)[i % 4]
                kinds = dict(u='plain', v='plain') if vec else (dict(u='pitch1') if i % 4 == 1 else dict(v='pitch1'))
                out.append(C(BIG, rows, Mg, Ng, math=1, shift=i % 3 == 0, acc=i % 2, colsum=i % 5 != 4, **kinds))
                i += 1
    return out


CASES = {
    'thin': (
        [C(THIN, 4096, 37, 1), C(THIN, 4159, 256, 3, shift=1), C(THIN, 4099, 257, 2, acc=1), C(THIN, 4096, 513, 4, shift=1),
         C(THIN, 4096, 1024, 4), C(THIN, 40000, 200, 3, shift=1, acc=1), C(THIN, 32767, 40, 2, shift=1)]
        + [C(THIN, 4159, 256, 3, colsum=0), C(THIN, 4099, 257, 2, shift=1, colsum=0), C(THIN, 32767, 40, 2, colsum=0, acc=1)]
        # every shape with and without the shift and with colsum NULL (no partial column sums are written then)
        + [C(THIN, 4096, 37, 1, shift=1, colsum=0), C(THIN, 4096, 513, 4, colsum=0), C(THIN, 4096, 1024, 4, shift=1, colsum=0),
           C(THIN, 40000, 200, 3, colsum=0)]
        + [C(THIN, 4096, 37, 1, res=0, shift=1)]
        # neighbours: 4095 rows, Mg 1025 and Ng 5 on the deep kernel; a U pitch of 37 on the big-block kernel's scalar loader
        + [C(DEEP, 4095, 37, 1, shift=1), C(DEEP, 4096, 1025, 4), C(DEEP, 4096, 37, 5, shift=1), C(BIG, 4096, 37, 1, u='tight', shift=1)]),
    'tn': (
        [C(TN, 32, 128, 250, math=4), C(TN, 736, 1000, 250, math=4, u='two', v='two', acc=1), C(TN, 4099, 77, 130, math=4, shift=1),
         C(TN, 8205, 150, 200, math=4, shift=1), C(TN, 8205, 150, 200, math=4, res=0, colsum=0)]
        # just under the FLOP gate (2 x 32 x 128 x 244 < 2e6); V one float past alignment: both go on down the ladder
        + [C(DEEP, 32, 128, 244, math=4), C(DEEP, 4099, 77, 130, math=4, v='base1', shift=1)]
        # debug bit 16384: the exact rung
        + [C(DEEP, 4099, 77, 130, math=4, shift=1, debug=16384)]),
    'deep': (
        [C(DEEP, 1, 1, 1), C(DEEP, 31, 64, 64, shift=1), C(DEEP, 33, 65, 65, acc=1), C(DEEP, 300, 23, 153, shift=1, colsum=0),
         C(DEEP, 1050, 200, 50, u='two', v='two', shift=1), C(DEEP, 1050, 200, 50, u='two', acc=1), C(DEEP, 2079, 128, 50, v='tight', shift=1),
         C(DEEP, 8191, 150, 200, res=0, shift=1), C(DEEP, 8160, 160, 208, u='tight', v='tight', acc=1), C(DEEP, 33, 65, 65, entry='edge')]),
    'pc': _edge_cases(PC, 0),
    'b3bf16': _edge_cases(B3BF16, 1),
    'b3f16': _edge_cases(B3F16, 4),
    'big': (
        [C(BIG, 640, 24, 24, entry='edge', gather=1, k=5, shift=1), C(BIG, 640, 24, 24, entry='edge', gather=1, k=5, u='pitch1', colsum=0)]
        + _big_dense()
        + [C(BIG, 200, 225, 256, entry='edge', gather=1, k=5, math=1, shift=1), C(BIG, 192, 160, 32, entry='edge', gather=1, k=16, math=1),
           C(BIG, 24576 + 7, 1000, 8, shift=1), C(BIG, 8160, 160, 208, math=1, acc=1),
           C(BIG, 4099, 161, 33, math=1, res=0, shift=1)]                               # nothing reserved: 129 partials
        + [C(BIG, 0, 65, 33), C(BIG, 0, 65, 33, acc=1), C(BIG, 0, 200, 200, math=1, shift=1)]),
}
GROUPS = list(CASES)
SPLIT_RUNGS = (TN, B3F16, B3BF16)

VARIANTS = ['drop_last_row', 'drop_last_tile', 'dup_row', 'read_past_rows', 'shift_skip_last_quad', 'shift_on_u', 'colsum_incl_Mg',
            'gather_prev_slot', 'gather_local', 'inner_off_by_one', 'acc_ignored', 'acc_when_0', 'g_pitch_Ng']


def case_params():
    return [(g, s) for g in GROUPS for s in CASES[g]]


# ----------------------------------------------------------------------------------------------------------------------
# buffers
# ----------------------------------------------------------------------------------------------------------------------
class Case(types.SimpleNamespace):
    """spec, kind, inp {name: array the call reads}, out0 {name: array it writes, pre-filled}, ru / rv row descriptors"""


def _rows(kind, rows, cols):
    """-> dict(off, so, si, inner, size, start [rows]) in floats"""
    r4 = round_up(cols, 4)
    ld = {'plain': r4 + 4, 'tight': cols, 'pitch1': r4 + 5, 'base1': r4 + 4, 'two': r4 + 4}[kind]
    off = 1 if kind == 'base1' else 0
    r = np.arange(rows, dtype=np.int64)
    if kind == 'two':
        so, si, inner = (INNER + 1) * ld, ld, INNER
        start = (r // INNER) * so + (r % INNER) * si
        nrows = (cdiv(max(rows, 1), INNER) + TAIL_ROWS // INNER + 1) * (INNER + 1)
    else:
        so, si, inner, start, nrows = ld, 0, 0, r * ld, rows + TAIL_ROWS
    return dict(off=off, so=so, si=si, inner=inner, size=off + nrows * ld + 8, start=start + off)


def _values(rng, kind, shape, offset=0.0):
    if kind == 'int':
        return f32(rng.integers(-4, 5, size=shape))
    return f32(rng.standard_normal(shape) + offset)


@functools.lru_cache(maxsize=6)
def build(spec, kind):
    """the call's host buffers (built once per (spec, kind), shared and left unchanged)"""
    s = spec
    rng = np.random.default_rng([zlib.crc32(case_id(s).encode()), int(kind == 'int')])
    rows, Mg, Ng = s.rows, s.Mg, s.Ng
    ru = _rows(s.u, rows, Mg)
    u = np.full(ru['size'], np.nan, np.float32)
    u[ru['start'][:, None] + np.arange(Mg)] = _values(rng, kind, (rows, Mg))
    inp = {'u': u}
    rv = None
    if s.gather:
        npts = rows // s.k
        ldpq = 2 * Ng + 4
        pq = np.full((npts + 8, ldpq), np.nan, np.float32)
        pq[:npts, :2 * Ng] = _values(rng, kind, (npts, 2 * Ng), 0.5 if kind == 'rand' else 0.0)
        N = npts // s.B
        jl = rng.integers(0, N, size=rows).astype(np.int32)
        jg = np.zeros(rows + TAIL_ROWS, np.int32)
        jg[:rows] = jl + (np.arange(rows) // (N * s.k) * N).astype(np.int32)          # GLOBAL neighbour rows
        inp.update(pq=pq.reshape(-1), jg=jg)
        meta = dict(ldpq=ldpq, npts=npts, N=N)
    else:
        rv = _rows(s.v, rows, Ng)
        v = np.full(rv['size'], np.nan, np.float32)
        v[rv['start'][:, None] + np.arange(Ng)] = _values(rng, kind, (rows, Ng), 3.0 if s.shift else 0.0)
        inp['v'] = v
        meta = {}
    c = Case(spec=s, kind=kind, id=case_id(s) + '/' + kind, inp=inp, ru=ru, rv=rv, ldg=Ng + 5, **meta)
    if s.shift:
        sh = np.full(Ng + 4, np.nan, np.float32)
        V = operands(c)[1]
        sh[:Ng] = rng.integers(-4, 5, size=Ng) if kind == 'int' else (V.mean(axis=0) if rows else np.zeros(Ng))
        inp['shift'] = sh
    G = np.full((Mg + 2, c.ldg), SENTINEL, np.float32)
    G[:Mg, :Ng] = rng.choice([-4, -3, -2, -1, 1, 2, 3, 4], size=(Mg, Ng)) if kind == 'int' else rng.standard_normal((Mg, Ng)) * max(rows, 1) ** 0.5
    cs = np.full(Mg + 4, SENTINEL, np.float32)
    cs[:Mg] = rng.choice([-4, -3, -2, -1, 1, 2, 3, 4], size=Mg) if kind == 'int' else rng.standard_normal(Mg) * max(rows, 1) ** 0.5
    ws = ws_floats(Mg, Ng)
    part = np.full(ws + PART_TAIL, np.nan, np.float32)
    part[ws:] = SENTINEL
    c.out0 = {'G': G.reshape(-1), 'part': part}
    if s.colsum:
        c.out0['colsum'] = cs
    c.ws = ws
    # amax words (f16x3): U's is its largest magnitude (int data: 4.0 whatever the draw), a dense V's likewise; a gathered V's word
    # comes from gpe_edge_pq_amax on the device, its bound for the bar is max(0, max P + max Q) (1 + 1e-6) and a rounding
    Uv, Vv = operands(c)[:2]
    c.amax_u = np.float32(4.0 if kind == 'int' else np.abs(Uv).max() if rows else 0.0)
    if s.gather:
        P, Q = pq[:npts, :Ng], pq[:npts, Ng:2 * Ng]
        c.amax_v = np.float32(max(0.0, float(P.max()) + float(Q.max())) * (1 + 2e-6)) if rows else np.float32(0)
    else:
        c.amax_v = np.float32(4.0 if kind == 'int' else np.abs(Vv).max() if rows else 0.0)
    return c


def operands(case, variant=None):
    """fp32 U [rows][Mg], V [rows][Ng] (a gathered V: relu(P_i + Q_j) in fp32, i = r / k, j = jg[r]), shift [Ng] or None"""
    s = case.spec
    rows, Mg, Ng = s.rows, s.Mg, s.Ng
    ru = case.ru
    ustart = ru['start']
    if variant == 'inner_off_by_one' and s.u == 'two':
        r = np.arange(rows, dtype=np.int64)
        ustart = ru['off'] + (r // (INNER + 1)) * ru['so'] + (r % (INNER + 1)) * ru['si']
    Uv = case.inp['u'][ustart[:, None] + np.arange(Mg)]
    if s.gather:
        pq = case.inp['pq'].reshape(-1, case.ldpq)
        r = np.arange(rows)
        j = case.inp['jg'][:rows].astype(np.int64)
        if variant == 'gather_prev_slot':
            j = case.inp['jg'][np.maximum(r - 1, 0)].astype(np.int64)
        if variant == 'gather_local':
            j = j - (r // (case.N * s.k)) * case.N
        Vv = np.maximum(pq[r // s.k, :Ng] + pq[j, Ng:2 * Ng], np.float32(0))
    else:
        Vv = case.inp['v'][case.rv['start'][:, None] + np.arange(Ng)]
    sh = case.inp['shift'][:Ng] if 'shift' in case.inp else None
    return f32(Uv), f32(Vv), sh


def variant_applies(case, variant):
    s = case.spec
    return {'drop_last_row': s.rows > 0, 'drop_last_tile': s.rows % 32 != 0 and s.rows > 32, 'dup_row': s.rows > 0, 'read_past_rows': s.rows % 32 != 0,
            'shift_skip_last_quad': bool(s.shift) and s.rows > 0, 'shift_on_u': bool(s.shift) and s.rows > 0, 'colsum_incl_Mg': bool(s.colsum),
            'gather_prev_slot': bool(s.gather), 'gather_local': bool(s.gather) and s.B > 1, 'inner_off_by_one': s.u == 'two' and s.rows > INNER,
            'acc_ignored': bool(s.acc), 'acc_when_0': not s.acc, 'g_pitch_Ng': s.Mg > 1}[variant]


def reference(case, variant=None):
    """-> G [Mg][Ng], magG, colsum [Mg], magcs, sumabs_u [Mg], sumabs_v [Ng] in fp64 (cached for variant None)"""
    if variant is None:
        if not hasattr(case, '_ref'):
            case._ref = reference(case, '')
        return case._ref
    s = case.spec
    Uv, Vv, sh = operands(case, variant)
    Ud, Vd = f64(Uv), f64(Vv)
    if sh is not None:
        shd = f64(sh)
        if variant == 'shift_on_u':
            Ud = Ud - shd[np.arange(s.Mg) % s.Ng]
        else:
            Vd = Vd - shd
            if variant == 'shift_skip_last_quad':
                q0 = (s.Ng - 1) // 4 * 4
                Vd[:, q0:] = f64(Vv)[:, q0:]
    sel = np.arange(s.rows)
    if variant == 'drop_last_row':
        sel = sel[:-1]
    if variant == 'drop_last_tile':
        sel = sel[:s.rows // 32 * 32]
    if variant == 'dup_row':
        sel = np.concatenate([sel, sel[s.rows // 2:s.rows // 2 + 1]])
    Ud, Vd = Ud[sel], Vd[sel]
    G = Ud.T @ Vd
    cs = Ud.sum(axis=0)
    if variant == 'read_past_rows':                                   # the last tile read 32 rows long: the NaN rows behind `rows`
        G = G + np.nan
        cs = cs + np.nan
    magG = np.abs(Ud).T @ np.abs(Vd)
    magcs = np.abs(Ud).sum(axis=0)
    sau, sav = magcs.copy(), np.abs(Vd).sum(axis=0)
    G0 = f64(case.out0['G'].reshape(s.Mg + 2, case.ldg)[:s.Mg, :s.Ng])
    add = (s.acc and variant != 'acc_ignored') or (not s.acc and variant == 'acc_when_0')
    if add:
        G = G + G0
        if s.colsum:
            cs = cs + f64(case.out0['colsum'][:s.Mg])
    if s.acc:
        magG = magG + np.abs(G0)
        if s.colsum:
            magcs = magcs + np.abs(f64(case.out0['colsum'][:s.Mg]))
    return G, magG, cs, magcs, sau, sav


def case_plan(case, cus=None):
    """the restated plan of the case's call with 16-byte aligned buffers: (path, fields).  cus: usable CUs (default 256 - reserved)"""
    s = case.spec
    math = {1: 1, 4: 2}.get(s.math, 0)
    ru, rv = case.ru, case.rv
    u = (4096 + 4 * ru['off'], ru['so'], ru['si'], ru['inner'])
    v = (0, case.ldpq, 0, 0) if s.gather else (8192 + 4 * rv['off'], rv['so'], rv['si'], rv['inner'])
    words = s.entry == 'edge' and settle_words(math, s.rows, 0, s.words != 'none', s.words == 'both', bool(s.gather), s.words == 'ws')
    return plan(u, v, s.rows, s.Mg, s.Ng, not s.gather, s.k, s.B, words, False, bool(s.colsum), math, s.debug, (256 - s.res) if cus is None else cus)


def bars(case, path, pl):
    """-> bar of G [Mg][Ng], bar of colsum [Mg] for a run on rung `path` with plan numbers pl (derivations: the module's docstring)"""
    s = case.spec
    _, magG, _, magcs, sau, sav = reference(case)
    n_p = chain_rows(path, pl, s.rows, s.B)
    if path == TN:
        bG = gamma(6 * s.rows + 3) * (1 + 2.0 ** -6) * magG
    elif path == B3BF16:
        bG = (3 * 2.0 ** -18 * (1 + 2.0 ** -8) + gamma(3 * n_p + 3) * (1 + 2.0 ** -7)) * magG
    elif path in (B3F16, LAZY):
        Au = float(case.amax_u)
        Av = float(case.amax_v) + (float(np.abs(case.inp['shift'][:s.Ng]).max()) if s.shift else 0.0)
        bG = ((12 * U * (1 + 2.0 ** -10) + gamma(3 * n_p + 3) * (1 + 2.0 ** -9)) * magG
              + 2.0 ** -39 * (1 + 2.0 ** -10) * (Au * sav[None, :] + Av * sau[:, None]) + s.rows * 2.0 ** -78 * Au * Av)
    else:
        bG = gamma(n_p + 3) * magG
    return bG, gamma((n_p if path == THIN else 8) + 2) * magcs


# ----------------------------------------------------------------------------------------------------------------------
# comparison
# ----------------------------------------------------------------------------------------------------------------------
def _fail(case, what, idx, got, ref, extra=''):
    raise AssertionError('%s %s at %s: got %r, reference %r %s' % (case.id, what, tuple(int(i) for i in np.atleast_1d(idx)), got, ref, extra))


def _within(case, what, got, ref, bar, exact):
    """element by element (a NaN fails): int data equal, random data |got - ref| <= bar -> worst |diff| / bar"""
    got, ref, bar = f64(got), f64(ref), f64(bar)
    assert got.shape == ref.shape == bar.shape, (case.id, what, got.shape, ref.shape, bar.shape)
    if got.size == 0:
        return 0.0
    diff = np.abs(got - ref)
    bad = ~(diff == 0) if exact else ~(diff <= bar)
    if bad.any():
        t = tuple(np.argwhere(bad)[0])
        _fail(case, what, t, got[t], ref[t], '(integer data: must be equal)' if exact else
              '|diff| %.3e > bar %.3e (%.2f bars)' % (diff[t], bar[t], diff[t] / bar[t] if bar[t] > 0 else np.inf))
    pos = bar > 0
    return float((diff[pos] / bar[pos]).max()) if pos.any() else 0.0


def _same_bits(case, what, got, ref):
    got, ref = f32(got), f32(ref)
    assert got.shape == ref.shape, (case.id, what, got.shape, ref.shape)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    if bad.any():
        t = tuple(np.argwhere(bad)[0])
        _fail(case, what, t, got[t], ref[t], '(must not be written)')


def check(case, got, variant=None, path=None, pl=None):
    """got = {'G', 'part', 'colsum'} as the call left them; path / pl: the rung and plan of the run that is checked (default: the
    restated plan of the case).  -> {'G': worst in bars, 'colsum': ...} (int data: 0.0, equality was asserted)"""
    s = case.spec
    if path is None:
        path, pl = case_plan(case)
    G, _, cs, _, _, _ = reference(case, variant)
    bG, bcs = bars(case, path, pl)
    exact = case.kind == 'int'
    Mg, Ng, ldg = s.Mg, s.Ng, case.ldg
    g = got['G'].reshape(Mg + 2, ldg)
    g0 = case.out0['G'].reshape(Mg + 2, ldg)
    worst = {}
    if variant == 'g_pitch_Ng':                                         # the wrong kernel writes row m at m * Ng: its image of the buffer
        img = case.out0['G'].copy()
        img[(np.arange(Mg)[:, None] * Ng + np.arange(Ng)).reshape(-1)] = f32(G).reshape(-1)
        if got['G'].tobytes() == img.tobytes() or np.array_equal(bits(got['G']), bits(img)):
            return {'G': 0.0}
        _fail(case, 'G image', (0,), 'pitch ldg', 'pitch Ng')
    worst['G'] = _within(case, 'G', g[:Mg, :Ng], G, bG, exact)
    _same_bits(case, 'G pad columns', g[:Mg, Ng:], g0[:Mg, Ng:])
    _same_bits(case, 'G rows behind Mg', g[Mg:], g0[Mg:])
    if s.colsum:
        c = got['colsum']
        worst['colsum'] = _within(case, 'colsum', c[:Mg], cs, bcs, exact)
        tail0 = case.out0['colsum'][Mg:]
        if variant == 'colsum_incl_Mg':                                 # the wrong kernel sums the pad column too and writes colsum[Mg]
            if bits(c[Mg:Mg + 1])[0] == bits([SENTINEL])[0]:
                _fail(case, 'colsum[Mg]', (Mg,), c[Mg], 'a written value')
            _same_bits(case, 'colsum behind Mg', c[Mg + 1:], tail0[1:])
        else:
            _same_bits(case, 'colsum behind Mg', c[Mg:], tail0)
    _same_bits(case, 'the floats behind gpe_redgemm_ws', got['part'][case.ws:], case.out0['part'][case.ws:])
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# emulation: an fp32 restatement of each rung's partial split, in one plausible order
# ----------------------------------------------------------------------------------------------------------------------
def _rn_bf16(x):
    b = f32(x).view(np.uint32)
    return ((b + (((b >> 16) & 1) + 0x7FFF)) & np.uint32(0xFFFF0000)).view(np.float32)


def _split2_bf16(x):
    h = _rn_bf16(x)
    return h, _rn_bf16((f32(x) - h).astype(np.float32))


def _split3_bf16(x):
    h = _rn_bf16(x)
    r = (f32(x) - h).astype(np.float32)
    m = _rn_bf16(r)
    return h, m, _rn_bf16((r - m).astype(np.float32))


def _split2_f16(x):
    h = f32(x).astype(np.float16)
    return h.astype(np.float32), (f32(x) - h.astype(np.float32)).astype(np.float16).astype(np.float32)


def _h3_scale(amax):
    """gpe_h3_scale_of: the power of two that brings amax into [2^14, 2^15)"""
    b = int(bits([amax])[0])
    e = (b >> 23) & 0xff
    sh = 0 if b == 0 or e == 255 else max(-100, min(100, 141 - e))
    return 2.0 ** sh


def _acc_tiles(acc, Us, Vs, planes):
    """acc [g][M][N] fp32 += per 32-row tile.  Us, Vs: lists of plane arrays [g][32][cols]; planes: the (u plane, v plane) products in order.
    Exact fp32 MFMA (one plane each): four rows per instruction, the 4-term dot in fp64 added to the fp32 accumulator"""
    for pu, pv in planes:
        Ut, V = np.swapaxes(f64(Us[pu]), 1, 2), f64(Vs[pv])
        step = 4 if len(Us) == 1 else 32
        for r0 in range(0, 32, step):
            acc = (acc + np.matmul(Ut[:, :, r0:r0 + step], V[:, r0:r0 + step, :])).astype(np.float32)
    return acc


def _partials(case, path, pl):
    """-> partial G [nblk][Mg][Ng] fp32"""
    s = case.spec
    Uv, Vv, sh = operands(case)
    if sh is not None:
        Vv = (Vv - sh).astype(np.float32)                               # one rounding, before any split
    rows, Mg, Ng = s.rows, s.Mg, s.Ng
    nblk = pl['nblk']
    part = np.zeros((nblk, Mg, Ng), np.float32)
    if path == THIN:
        rpb = cdiv(rows, nblk)
        for b in range(nblk):
            lo, hi = b * rpb, min((b + 1) * rpb, rows)
            w = np.zeros((4, Mg, Ng), np.float32)
            for r in range(lo, hi):                                     # wave r % 4 of the workgroup: one fma per row
                w[(r - lo) % 4] = (f64(w[(r - lo) % 4]) + np.outer(f64(Uv[r]), f64(Vv[r]))).astype(np.float32)
            part[b] = ((f64(w[0]) + f64(w[1])) + (f64(w[2]) + f64(w[3]))).astype(np.float32)
        return part
    if path == TN:
        rps = pl['rows_per_split']
        Up, Vp = _split3_bf16(Uv), _split3_bf16(Vv)
        for b in range(nblk):
            lo, hi = b * rps, min((b + 1) * rps, rows)
            acc = np.zeros((Mg, Ng), np.float32)
            for r0 in range(lo, hi, 32):
                for pa, pw in ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)):
                    acc = (acc + f64(Up[pa][r0:min(r0 + 32, hi)]).T @ f64(Vp[pw][r0:min(r0 + 32, hi)])).astype(np.float32)
            part[b] = acc
        return part
    if path == B3BF16:
        Us, Vs, planes, post = _split2_bf16(Uv), _split2_bf16(Vv), ((1, 0), (0, 1), (0, 0)), 1.0
    elif path == B3F16:
        sU = _h3_scale(case.amax_u)
        sV = _h3_scale(np.float32(case.amax_v) + (np.abs(sh).max() if sh is not None else np.float32(0)))
        Us, Vs, planes, post = _split2_f16(Uv * np.float32(sU)), _split2_f16(Vv * np.float32(sV)), ((1, 0), (0, 1), (0, 0)), 1.0 / (sU * sV)
    else:
        Us, Vs, planes, post = (Uv,), (Vv,), ((0, 0),), 1.0
    tiles = wg_tiles(pl, s.B)
    pad = np.zeros((32, 1), np.float32)
    for step in range(max((len(t) for t in tiles), default=0)):
        live = [b for b in range(nblk) if step < len(tiles[b])]
        ridx = np.stack([tiles[b][step] * 32 + np.arange(32) for b in live])               # [g][32]
        ok = (ridx < rows)[:, :, None]
        ridx = np.minimum(ridx, rows - 1)
        part[live] = _acc_tiles(part[live], [np.where(ok, P[ridx], pad) for P in Us], [np.where(ok, P[ridx], pad) for P in Vs], planes)
    return (part * np.float32(post)).astype(np.float32) if post != 1.0 else part


def emulate(case, path=None, pl=None):
    """what a correct kernel on rung `path` leaves in G, colsum and part"""
    s = case.spec
    if path is None:
        path, pl = case_plan(case)
    key = (path, pl['gx'], pl['nblk'])
    if getattr(case, '_emu_key', None) != key:
        part = _partials(case, path, pl)
        Uv = operands(case)[0]
        G = f64(part).sum(axis=0).astype(np.float32)
        cs32 = np.add.reduceat(f64(Uv), np.arange(0, s.rows, 8), axis=0).astype(np.float32) if s.rows else np.zeros((1, s.Mg), np.float32)
        cs = f64(cs32).sum(axis=0).astype(np.float32)
        out = {n: a.copy() for n, a in case.out0.items()}
        g = out['G'].reshape(s.Mg + 2, case.ldg)
        g[:s.Mg, :s.Ng] = (g[:s.Mg, :s.Ng] + G).astype(np.float32) if s.acc else G
        if s.colsum:
            out['colsum'][:s.Mg] = (out['colsum'][:s.Mg] + cs).astype(np.float32) if s.acc else cs
        out['part'][:pl['floats']] = 0.0                                # the launch's image, written (values are not compared)
        case._emu_key, case._emu = key, out
    return case._emu


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI
# ----------------------------------------------------------------------------------------------------------------------
def path_args(case, d):
    """gpe_redgemm_path's arguments without plan_out; d = {name: anything whose slice [off:] is the pointer}"""
    s = case.spec
    ru, rv = case.ru, case.rv
    vd = (d['pq'][0:], case.ldpq, 0, 0) if s.gather else (d['v'][rv['off']:], rv['so'], rv['si'], rv['inner'])
    return [d['u'][ru['off']:], ru['so'], ru['si'], ru['inner'], *vd, s.rows, s.Mg, s.Ng, 0 if s.gather else 1, s.k, s.B,
            int(s.words != 'none'), int(s.words == 'both'), int(s.words == 'ws'), 0, int(bool(s.colsum))]


def abi_args(case, d):
    """the argument list of gpe_redgemm / gpe_edge_redgemm (include/gpe_hip.h) without the stream; d = {name: device tensor}; absent =
    NULL.  'amax_u' / 'amax_v' are uint32 words, 'ws' the edge workspace with 'ws_bytes'"""
    s = case.spec
    ru, rv = case.ru, case.rv
    if s.entry == 'redgemm':
        return [d['u'][ru['off']:], ru['so'], ru['si'], ru['inner'], d['v'][rv['off']:], rv['so'], rv['si'], rv['inner'], d.get('shift'),
                s.rows, s.Mg, s.Ng, d['G'], case.ldg, d.get('colsum'), d['part'], s.acc]
    assert ru['inner'] == 0 and (rv is None or rv['inner'] == 0)
    return [d['u'][ru['off']:], ru['so'], 0 if s.gather else 1, None if s.gather else d['v'][rv['off']:], 0 if s.gather else rv['so'],
            d.get('pq'), case.ldpq if s.gather else 0, d.get('jg'), d.get('shift'), s.B, s.rows // (s.B * s.k), s.k, s.Mg, s.Ng, d['G'], case.ldg,
            d.get('colsum'), d['part'], d.get('amax_u') if s.words != 'none' else None, d.get('amax_v') if s.words == 'both' else None,
            d.get('ws') if s.words == 'ws' else None, d.get('ws_bytes', 0) if s.words == 'ws' else 0, None, 0, None, None, 0, None]

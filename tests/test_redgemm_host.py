"""CPU: the restated reduce-GEMM ladder of tests/redgemm_restate.py is checked before any GPU time is spent on it.

a) the restated plan is the library's: `path_query` equals gpe_redgemm_path (host only, include/gpe_hip.h) — the rung and every
   plan_out number — on every case at 0 and 192 reserved CUs, and on a seeded sweep of a few thousand random calls over shapes,
   pitches, alignments, modes, words and k; the launch's floats never exceed gpe_redgemm_ws(Mg, Ng), which is restated too;
b) the case lists reach every rung and every kernel instance, each case on the rung it was written for;
c) every bar passes its own reference: the checker accepts `emulate`, an fp32 restatement of the rung's partial split, on random
   data, and that restatement equals fp64 bit for bit on integer data;
d) every wrong variant is rejected on every rung that has a case it changes (integer data);
e) the export refuses what the entry points refuse; a lazy call answers 4 where gpe_edge_lazy_dz3_ok holds."""
import ctypes

import numpy as np
import pytest

import redgemm_restate as R
from gpe_amd import _lib


class _StandIn:
    """host memory stands in for a device buffer: gpe_redgemm_path looks at a pointer's value, never behind it"""

    def __init__(self):
        self.buf = (ctypes.c_double * 16)()
        self.base = (ctypes.addressof(self.buf) + 63) // 64 * 64

    def __getitem__(self, sl):
        return self.base + 4 * (sl.start or 0)


_U, _V = _StandIn(), _StandIn()


@pytest.fixture
def state():
    """the process state the plan reads, restored afterwards"""
    l = _lib.lib()
    math, dbg, gate = l.gpe_math_get(), l.gpe_debug_get(), l.gpe_f16x3_min_rows()
    res = l.gpe_reserve_cus_set(0)
    l.gpe_debug_set(0)
    yield l
    l.gpe_reserve_cus_set(res)
    l.gpe_f16x3_min_rows_set(gate)
    l.gpe_debug_set(dbg)
    l.gpe_math_set(math)


def _export(l, args):
    out = (ctypes.c_long * len(R.PLAN_FIELDS))(*([-1] * len(R.PLAN_FIELDS)))
    rc = l.gpe_redgemm_path(*args, ctypes.addressof(out))
    return rc, (dict(zip(R.PLAN_FIELDS, out)) if rc > 0 else None)


def _case_args(case):
    return R.path_args(case, {'u': _U, 'v': _V, 'pq': _V})


def _set(l, spec, res=None):
    l.gpe_math_set(spec.math)
    l.gpe_debug_set(spec.debug)
    l.gpe_f16x3_min_rows_set(0)
    l.gpe_reserve_cus_set(spec.res if res is None else res)


# ----------------------------------------------------------------------------------------------------------------------
# a) the plan
# ----------------------------------------------------------------------------------------------------------------------
def test_restated_plan_is_the_librarys_on_every_case(state):
    l = state
    for g, spec in R.case_params():
        case = R.build(spec, 'int')
        args = _case_args(case)
        for res in (0, 192):
            _set(l, spec, res)
            got = _export(l, args)
            want = R.path_query(args, spec.math, spec.debug, 0, 256 - res)
            assert got == want, (R.case_id(spec), res, got, want)
            assert got[0] > 0 and got[1]['floats'] <= l.gpe_redgemm_ws(spec.Mg, spec.Ng) == R.ws_floats(spec.Mg, spec.Ng)
            if res == spec.res:                                          # ... and `case_plan`, which the checks use, says the same
                assert R.case_plan(case) == got, R.case_id(spec)
                assert got[0] == spec.rung, (R.case_id(spec), got[0])


def test_restated_plan_is_the_librarys_on_a_sweep(state):
    """6000 random calls; the sweep must itself reach every rung, -22 included"""
    l = state
    rng = np.random.default_rng(5033)
    seen = {}
    pick = lambda *a: a[rng.integers(len(a))]
    for it in range(6000):
        edgy = rng.random() < 0.45                                      # the edge shapes: rungs 4 - 7 are a corner of the space
        Mg = int(pick(rng.integers(1, 1100), rng.integers(1, 260), pick(150, 160, 200, 208, 145, 193), pick(48, 64, 128, 1000, 1024, 1025)))
        Ng = int(pick(rng.integers(1, 258), pick(1, 2, 3, 4, 5), pick(200, 208, 193, 196), pick(48, 128, 250, 256, 257)))
        rows = int(pick(rng.integers(0, 70000), rng.integers(0, 600), pick(0, 31, 32, 4095, 4096, 8160, 8161, 8192, 32736, 32768, 65536),
                        rng.integers(0, 2 ** 21), pick(2 ** 31 - 1, 2 ** 31, 2 ** 32 + 5)))
        k = int(pick(0, 0, 1, 5, 15, 16, 20))
        pin = int(pick(0, 1, 2, 8, 16, 24, 32)) if rng.random() < 0.2 or not k else int(pick(1, 2, 8, 16, 32))
        if edgy:
            Mg, Ng = int(pick(150, 160, 200, 208, 145, 144, 161, 209)), int(pick(200, 208, 196, 193, 192))
            rows = int(pick(rng.integers(7000, 9000), rng.integers(30000, 70000), rng.integers(2 ** 19, 2 ** 21), pick(8160, 8161, 32736, 32737)))
            k = int(pick(0, 1, 15, 16, 16, 16))
        if k and pin and rng.random() < 0.9:
            rows = max(rows // (k * pin), 1) * k * pin
            if rng.random() < 0.5 and pin >= 8:
                rows = max(rows // (k * pin * 32), 1) * k * pin * 32
        v_mode = int(pick(1, 1, 0)) if k else int(pick(1, 1, 1, 1, 1, 1, 0))
        if v_mode == 0 and rng.random() < 0.8:
            Ng = R.round_up(Ng, 4)

        def operand(cols, two_ok):
            r4 = R.round_up(cols, 4)
            so = int(pick(r4, r4 + 4, cols, r4 + 1, cols - 1 if cols > 1 else 1, 2 * r4 + 8)) if not edgy or rng.random() < 0.15 else r4 + 4
            base = (int(pick(0, 0, 0, 1, 2, 4)) * 4 if not edgy or rng.random() < 0.1 else 0) + _U.base if rng.random() < 0.98 else 0
            if two_ok and rng.random() < 0.2:
                inner = int(pick(1, 7, 16))
                si = int(pick(r4 + 4, r4 + 4, r4 + 5, cols))
                return [base, (inner + 1) * si + int(pick(0, 0, 1)), si, inner]
            return [base, so, int(pick(0, 0, 3)), int(pick(0, 0, 0, -1))]
        u, v = operand(Mg, k == 0 or rng.random() < 0.05), operand(Ng if v_mode else 2 * Ng, k == 0 or rng.random() < 0.05)
        flags = [int(rng.random() < 0.7), int(rng.random() < 0.6), int(rng.random() < 0.5), int(rng.random() < (0.25 if edgy else 0.03)), int(rng.random() < 0.6)]
        args = u + v + [rows, Mg, Ng, v_mode, k, pin] + flags
        math, debug = int(pick(0, 1, 2, 3, 4, 4, 4)), int(pick(0, 0, 0, 16384, 32768, 512))
        res, gate = int(pick(0, 192, 64, 8)), int(pick(0, 32768, 32768, 100000))
        l.gpe_math_set(math)
        l.gpe_debug_set(debug)
        l.gpe_reserve_cus_set(res)
        l.gpe_f16x3_min_rows_set(gate)
        got = _export(l, args)
        want = R.path_query(args, math, debug, gate, 256 - res)
        assert got == want, (it, args, math, debug, res, gate, got, want)
        if got[0] > 0:
            assert got[1]['floats'] <= l.gpe_redgemm_ws(Mg, Ng) == R.ws_floats(Mg, Ng), (it, args)
        seen[got[0]] = seen.get(got[0], 0) + 1
    print('sweep:', sorted(seen.items()))
    assert set(seen) == {-22, 1, 2, 3, 4, 5, 6, 7, 8}, seen
    assert min(seen.values()) >= 5, seen


def test_workspace_query_is_restated(state):
    for Mg in list(range(1, 300, 7)) + [1000, 1024, 1025, 4000]:
        for Ng in list(range(1, 258, 5)) + [256, 257]:
            assert state.gpe_redgemm_ws(Mg, Ng) == R.ws_floats(Mg, Ng), (Mg, Ng)


# ----------------------------------------------------------------------------------------------------------------------
# b) the case lists reach every rung and every instance
# ----------------------------------------------------------------------------------------------------------------------
def test_case_lists_reach_every_instance(state):
    inst = set()
    for g, spec in R.case_params():
        case = R.build(spec, 'int')
        path, pl = R.case_plan(case)
        assert path == spec.rung and (R.RUNG_NAMES[path] == g or g in ('thin', 'tn')), R.case_id(spec)
        vm = 'gather' if spec.gather else 'dense'
        inst.add({R.THIN: ('thin', pl['ql'] if pl['ql'] <= 2 else 4), R.TN: ('tn',), R.DEEP: ('deep', pl['vvec']),
                  R.PC: ('pc', pl['MT'], vm), R.B3BF16: ('b3bf16', pl['MT'], vm), R.B3F16: ('b3f16', pl['MT'], vm),
                  R.BIG: ('big', pl['MH'], pl['NH'], vm, pl['vec'])}[path])
    want = {('thin', 1), ('thin', 2), ('thin', 4), ('tn',), ('deep', 0), ('deep', 1)}
    want |= {(r, mt, vm) for r in ('pc', 'b3bf16', 'b3f16') for mt in (10, 13) for vm in ('dense', 'gather')}
    want |= {('big', mh, nh, 'dense', vec) for mh in (2, 5, 7) for nh in (1, 5, 7, 8) for vec in (0, 1)}
    assert want <= inst, sorted(want - inst)
    # the twelve big-block instances with a gathered V are reached where Ng % 4 == 0 allows: at least one per NH class and MH class
    gath = {(i[1], i[2]) for i in inst if i[0] == 'big' and i[3] == 'gather'}
    assert {mh for mh, _ in gath} >= {2, 5, 7} and {nh for _, nh in gath} >= {1, 8}, gath
    # thin: ql 3 runs the <4> instance; 512 partials; workgroups without a row; pinned tiles on rungs 5 - 7; rows = 0
    plans = {s: R.case_plan(R.build(s, 'int'))[1] for _, s in R.case_params()}
    assert {3, 4} <= {p['ql'] for s, p in plans.items() if s.rung == R.THIN}
    assert any(p['nblk'] == 512 for s, p in plans.items() if s.rung == R.THIN)
    assert any(R.cdiv(s.rows, p['nblk']) * (p['nblk'] - 1) >= s.rows for s, p in plans.items() if s.rung == R.THIN)
    for r in (R.PC, R.B3BF16, R.B3F16):
        assert any(p['pin_tpc'] > 0 for s, p in plans.items() if s.rung == r), r
        assert any(s.res == 0 for s in plans if s.rung == r), r
    assert any(s.rows == 0 for s in plans) and any(s.rows == 0 and s.acc for s in plans)
    assert any(p['gx'] == 32 and s.res == 0 for s, p in plans.items() if s.rung == R.DEEP)
    assert any(p['gy'] == 5 for s, p in plans.items() if s.rung == R.BIG)
    assert any(s.res == 0 and p['gx'] > 64 for s, p in plans.items() if s.rung == R.BIG)                # one big-block case with nothing reserved
    # the dense big-block cases: every Mg and Ng at the edges of the MH / NH classes, at 96 .. 300 rows
    small = [s for s in plans if s.rung == R.BIG and not s.gather and 96 <= s.rows <= 300]
    assert {s.Mg for s in small} == {m for ms in R.BIG_MG.values() for m in ms} == {1, 64, 65, 160, 161, 224, 225}
    assert {s.Ng for s in small} == {n for ns in R.BIG_NG.values() for n in ns} == {5, 32, 33, 160, 161, 224, 225, 256}
    assert any(s.rows == 640 and (s.Mg, s.Ng, s.k) == (24, 24, 5) and s.gather for s in plans if s.rung == R.BIG)
    # thin: every shape with and without the shift and with colsum NULL
    for shape in {(s.rows, s.Mg, s.Ng) for s in plans if s.rung == R.THIN}:
        mine = [s for s in plans if s.rung == R.THIN and (s.rows, s.Mg, s.Ng) == shape]
        assert any(s.shift for s in mine) and any(not s.shift for s in mine) and any(not s.colsum for s in mine), shape
    assert any(p['gx'] == 1 and s.math == 4 for s, p in plans.items() if s.rung == R.TN)               # S = 1
    for r in set(R.RUNG_NAMES) - {R.LAZY}:                               # accumulate, colsum NULL and the shift on every rung that takes them
        mine = [s for s in plans if s.rung == r]
        assert any(not s.colsum for s in mine) and any(s.shift for s in mine) and any(not s.shift for s in mine), r
        assert any(s.acc for s in mine) or all(s.entry == 'edge' for s in mine), r


# ----------------------------------------------------------------------------------------------------------------------
# c) every bar passes its own reference; d) every wrong variant is rejected
# ----------------------------------------------------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize('group', R.GROUPS)
def test_bars_accept_the_emulation_and_reject_the_variants(group):
    """per rung: on every case the emulation is bit-exact on integer data and inside the bar on random data, and leaves the case's
    buffers unchanged; every variant is rejected by an integer case of the rung if the rung has a case that the variant changes"""
    rejected, tried = {}, {}
    worst = {}
    for spec in R.CASES[group]:
        for kind in ('int', 'rand'):
            case = R.build(spec, kind)
            before = {n: a.tobytes() for n, a in {**case.inp, **case.out0}.items()}
            emu = R.emulate(case)
            w = R.check(case, emu)
            if kind == 'rand':
                assert all(v <= 1.0 for v in w.values()), (case.id, w)
                key = R.RUNG_NAMES[spec.rung]
                worst[key] = {**worst.get(key, {}), **{n: max(worst.get(key, {}).get(n, 0.0), v) for n, v in w.items()}}
            else:
                assert not np.isnan(emu['G'][:1]).any()
                for variant in R.VARIANTS:
                    if variant in rejected or not R.variant_applies(case, variant):
                        continue
                    tried[variant] = tried.get(variant, 0) + 1
                    try:
                        R.check(case, emu, variant=variant)
                    except AssertionError:
                        rejected[variant] = case.id
            for n, a in {**case.inp, **case.out0}.items():
                assert a.tobytes() == before[n], (case.id, n)
    for variant in R.VARIANTS:
        print('%s / %s: %s' % (group, variant, 'rejected by %s (case %d of those it changes)' % (rejected[variant], tried[variant])
                               if variant in rejected else 'changes no case' if variant not in tried else 'NOT REJECTED'))
        assert variant in rejected or variant not in tried, (group, variant)
    print('%s: the emulation on random data, worst in bars: %s' % (group, worst))
    # what a rung's list cannot show: gathers only on the edge entry (rungs 5 - 8); two-level rows only where a kernel takes them
    always = {'drop_last_row', 'drop_last_tile', 'dup_row', 'read_past_rows', 'shift_skip_last_quad', 'shift_on_u', 'colsum_incl_Mg',
              'acc_when_0', 'g_pitch_Ng'}
    assert always <= set(tried), (group, always - set(tried))
    if group in ('pc', 'b3bf16', 'b3f16'):
        assert {'gather_prev_slot', 'gather_local'} <= set(tried), group
    if group in ('tn', 'deep'):
        assert 'inner_off_by_one' in tried, group
    if group != 'b3f16':
        assert 'acc_ignored' in tried, group


# ----------------------------------------------------------------------------------------------------------------------
# e) refusals, and the lazy rung
# ----------------------------------------------------------------------------------------------------------------------
def test_export_refuses_what_the_entry_points_refuse(state):
    l = state
    _set(l, R.C(R.DEEP, 33, 65, 65))
    good = [_U[0:], 72, 0, 0, _V[0:], 72, 0, 0, 33, 65, 65, 1, 0, 0, 0, 0, 0, 0, 1]
    assert l.gpe_redgemm_path(*good, None) == R.DEEP
    G = _StandIn()
    # position in gpe_redgemm_path's list -> position in gpe_redgemm's; both answer -22 before anything is launched
    for pos, bad, epos in ((0, None, 0), (4, None, 4), (8, -1, 9), (9, 0, 10), (10, 0, 11), (10, 257, 11), (9, -3, 10)):
        args = list(good)
        args[pos] = bad
        assert l.gpe_redgemm_path(*args, None) == -22, (pos, bad)
        entry = [_U[0:], 72, 0, 0, _V[0:], 72, 0, 0, None, 33, 65, 65, G[0:], 70, None, G[0:], 0]
        entry[epos] = bad
        assert l.gpe_redgemm(*entry, None) == -22, (pos, bad)
    for pos, bad in ((11, 0), (11, 2), (17, 1)):                        # a gpe_redgemm call is dense and never lazy
        args = list(good)
        args[pos] = bad
        assert l.gpe_redgemm_path(*args, None) == -22, (pos, bad)
    # the edge entry: B = 2 clouds of 64 points, k = 4
    egood = [_U[0:], 72, 0, 0, _V[0:], 136, 0, 0, 512, 65, 64, 0, 4, 2, 0, 0, 0, 0, 1]
    assert l.gpe_redgemm_path(*egood, None) == R.BIG

    def edge_entry(a):
        dense = a[11] == 1
        return [a[0], a[1], a[11], a[4] if dense else None, a[5] if dense else 0, None if dense else a[4], 0 if dense else a[5],
                None if dense else G[0:], None, a[13], a[8] // (a[13] * a[12]) if a[12] > 0 and a[13] > 0 else 0, a[12], a[9], a[10],
                G[0:], a[10] + 5, None, G[0:], None, None, None, 0, None, 0, None, None, 0, None]
    for pos, bad in ((0, None), (4, None), (1, 64), (9, 0), (10, 0), (10, 260), (10, 66), (5, 134), (12, -1), (13, 0)):
        args = list(egood)
        args[pos] = bad
        assert l.gpe_redgemm_path(*args, None) == -22, (pos, bad)
        assert l.gpe_edge_redgemm(*edge_entry(args), None) == -22, (pos, bad)
    dense = list(egood)
    dense[11], dense[5] = 1, 63                                         # dense V: ldv < Ng
    assert l.gpe_redgemm_path(*dense, None) == -22 and l.gpe_edge_redgemm(*edge_entry(dense), None) == -22
    for pos, bad in ((8, 511), (3, 7), (7, 7), (8, 2 ** 31)):          # what only the export can be handed: rows no multiple of B k, two-level rows
        args = list(egood)
        args[pos] = bad
        assert l.gpe_redgemm_path(*args, None) == -22, (pos, bad)
    # plan_out may be NULL, and is left alone where the call is refused
    out = (ctypes.c_long * 17)(*([-5] * 17))
    bad = list(good)
    bad[10] = 257
    assert l.gpe_redgemm_path(*bad, ctypes.addressof(out)) == -22 and list(out) == [-5] * 17


def test_lazy_calls_answer_rung_4_where_lazy_dz3_ok_holds(state):
    """... and -22 where the plan refuses a lazy call: another mode, k != 16, rows under the f16x3 gate, widths off the edge shape"""
    l = state
    shapes = [(32, 2048, 16, 150, 200), (32, 2048, 16, 200, 200), (2, 1024, 16, 150, 200), (32, 2048, 15, 150, 200), (32, 2048, 16, 150, 192),
              (32, 2048, 16, 120, 200), (1, 2048, 16, 150, 200)]
    answers = set()
    for math in (0, 1, 4):
        for res in (0, 192):
            for gate in (0, 32768, 1 << 30):
                l.gpe_math_set(math)
                l.gpe_reserve_cus_set(res)
                l.gpe_f16x3_min_rows_set(gate)
                for B, N, k, F, Cprev in shapes:
                    ldu, ldv = R.round_up(F, 4), R.round_up(Cprev, 4)
                    rc = l.gpe_redgemm_path(_U[0:], ldu, 0, 0, _V[0:], ldv, 0, 0, B * N * k, F, Cprev, 1, k, B, 1, 1, 1, 1, 1, None)
                    ok = l.gpe_edge_lazy_dz3_ok(B, N, k, F, Cprev)
                    # the plan's own conditions are weaker than gpe_edge_lazy_dz3_ok's (which also asks for 8 tiles per CU and reads debug
                    # bit 512): where the caller's gate holds the answer is 4; where it does not, 4 or -22, never another rung
                    assert rc == R.LAZY if ok else rc in (R.LAZY, -22), (math, res, gate, B, N, k, F, Cprev, rc, ok)
                    if math != 4 or k != 16 or B * N * k < gate or (F, Cprev) in ((150, 192), (120, 200)):
                        assert rc == -22 and not ok, (math, res, gate, B, N, k, F, Cprev, rc, ok)
                    want = R.path_query([_U[0:], ldu, 0, 0, _V[0:], ldv, 0, 0, B * N * k, F, Cprev, 1, k, B, 1, 1, 1, 1, 1], math, 0, gate, 256 - res)
                    assert want[0] == rc
                    answers.add(rc)
    assert answers == {R.LAZY, -22}
    # without both words a lazy call is refused
    l.gpe_math_set(4)
    l.gpe_reserve_cus_set(0)
    l.gpe_f16x3_min_rows_set(32768)
    assert l.gpe_redgemm_path(_U[0:], 152, 0, 0, _V[0:], 200, 0, 0, 32 * 2048 * 16, 150, 200, 1, 16, 32, 1, 0, 1, 1, 1, None) == -22

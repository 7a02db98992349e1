"""CPU: the restated graph-search ladder of tests/knn_restate.py is checked before any GPU time is spent on it.

a) the restated plan is the library's: `plan` equals gpe_knn_path (host only, include/gpe_hip.h) — the return value and every plan_out
   number — on every case at 0 and 192 reserved CUs with the case's switches passed in, and on a seeded sweep of a few thousand
   random calls that must itself reach every path, 0 and -22; `ws_layout` is gpe_knn_ws_bytes, the regions a plan uses neither overlap
   nor pass ws_bytes, the sorted cloud and every granted split fit the list region; in a child process under GPE_DEBUG=1,
   switches = NULL answers what the explicit array answers;
b) the case list reaches every path and every kernel instance `instance` names, each case on the rung and main kernel it was written
   for, on the plan of a 256-CU device with the case's reservation;
c) the definition stands: on the gauss data of every case an fp64 brute-force top-k set differs from the oracle's only for queries
   whose fp64 margin between the k-th and the (k+1)-th distance is below 4 (C + 2) 2^-24 of the k-th, and for at most 1% of a case's
   queries;
d) every wrong variant is rejected by `check` on every case it can change;
e) the export refuses what gpe_knn refuses (step 0 of DESIGN.md 5.32) and answers 0 for B = 0."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_restate as R
from gpe_amd import _lib

X_BASE, WS_BASE = 1 << 20, 1 << 30          # stand-ins: gpe_knn_path looks at a pointer's value, never behind it


@pytest.fixture
def lib():
    l = _lib.lib()
    res = l.gpe_reserve_cus_set(0)
    yield l
    l.gpe_reserve_cus_set(res)


def _export(l, c, sw):
    out = (ctypes.c_long * len(R.PLAN_FIELDS))(*([-5] * len(R.PLAN_FIELDS)))
    arr = None if sw is None else (ctypes.c_int * 10)(*sw)
    rc = l.gpe_knn_path(c.x or None, c.B, c.N, c.C, c.ldx, c.k, c.has_idx_glob, c.has_order_in, c.has_order_out, c.ws or None, c.ws_bytes,
                        arr, ctypes.addressof(out))
    if rc <= 0:
        assert list(out) == [-5] * len(R.PLAN_FIELDS), 'plan_out written without a path'
    return rc, (dict(zip(R.PLAN_FIELDS, out)) if rc > 0 else None)


def _regions_ok(c, path, p):
    spans = sorted((first, first + n, name) for name, first, n in R.regions(c, path, p))
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, (an, bn, c)
    assert all(0 <= a0 and a1 <= c.ws_bytes for a0, a1, _ in spans), (spans, c)
    lists = R.ws_layout(c.B, c.N, c.C)['lists_bytes']
    if path in (R.SORTED3, R.ALLPAIRS):                     # the two aliases of the list region stay inside it
        assert all(a1 <= lists for _, a1, _ in spans), (spans, c)


# ----------------------------------------------------------------------------------------------------------------------
# a) the plan
# ----------------------------------------------------------------------------------------------------------------------
def test_restated_plan_is_the_librarys_on_every_case(lib):
    for s in R.CASES:
        for res in (0, 192):
            lib.gpe_reserve_cus_set(res)
            for flags in (dict(), dict(has_order_in=1), dict(has_idx_glob=0, has_order_out=0)):
                c = R.call_of(s, X_BASE, WS_BASE, **flags)
                got, want = _export(lib, c, s.sw), R.plan(c, 256 - res, s.sw)
                assert got == want, (R.case_id(s), res, flags, got, want)
                assert got[0] > 0
                _regions_ok(c, *got)
                if res == s.res:
                    assert R.case_plan(s, **flags) == got


def test_restated_plan_is_the_librarys_on_a_sweep(lib):
    """5000 random calls; the sweep must itself reach every path, 0 and -22"""
    rng = np.random.default_rng(532)
    pick = lambda *a: a[rng.integers(len(a))]
    seen = {}
    for it in range(5000):
        C = int(pick(rng.integers(1, 16), 3, 3, pick(15, 16, 17), rng.integers(16, 161), pick(160, 161), rng.integers(161, 257), pick(256, 257),
                     rng.integers(257, 400)))
        N = int(pick(rng.integers(1, 70), pick(63, 64, 65), pick(127, 128, 129), rng.integers(128, 700), pick(8191, 8192, 8193),
                     rng.integers(1000, 9000)))
        k = int(pick(rng.integers(1, 66), rng.integers(1, 20), pick(32, 33, 48, 49, 64, 65)))
        if rng.integers(8):
            k = min(k, N)
        B = int(pick(rng.integers(0, 41), rng.integers(1, 41), pick(7, 8, 9), 1, 2, pick(0, 3, 33)))
        ldx = C + int(pick(0, 0, 1, 2, 3, 4, -1 if rng.integers(20) == 0 else 0))
        x = 0 if rng.integers(60) == 0 else X_BASE + 4 * int(rng.integers(0, 8))
        w = R.ws_layout(max(B, 0), N, C)
        edges = [w['sorted_bytes'], w['need_f32'], w['need_h3'], w['total'], R.split_bytes(B, N, 2, k), R.split_bytes(B, N, 3, k),
                 R.split_bytes(B, N, 4, k), w['lists_bytes']]
        nbytes = max(0, int(pick(w['total'], w['total'], w['need_h3'], *edges)) + int(pick(0, 0, 0, -1, 1, -256, 256)))
        ws = 0 if rng.integers(12) == 0 else WS_BASE + int(pick(0, 0, 0, 4, 8, 16))
        sw = R.switches() if rng.integers(3) == 0 else R.switches(
            PIN=pick(-1, -1, 0, 1), VEC=pick(0, 0, 1, 2, 4), SPLIT=pick(0, 0, 2, 3, 4, 5), EXACT=pick(0, 0, 0, 1), F32FILTER=pick(0, 0, 1),
            SORTED=pick(1, 1, 0), NOORDER=pick(0, 1), FT=pick(1, 1, 0, 4, 8), RR2=pick(1, 0), PROBE=pick(0, 0, 0, 0, 1, 4))
        res = int(pick(0, 0, 64, 192, rng.integers(0, 193)))
        lib.gpe_reserve_cus_set(res)
        c = R.Call(x, B, N, C, ldx, k, int(rng.integers(2)), int(rng.integers(2)), int(rng.integers(2)), ws, nbytes)
        got, want = _export(lib, c, sw), R.plan(c, 256 - res, sw)
        assert got == want, (it, c, sw, res, got, want)
        if got[0] > 0:
            _regions_ok(c, *got)
            if got[0] == R.ALLPAIRS and got[1]['nsplit'] > 1:
                seen['split'] = seen.get('split', 0) + 1
                if not sw[R.SW_FIELDS.index('SPLIT')]:
                    seen['natural split'] = seen.get('natural split', 0) + 1
        seen[got[0]] = seen.get(got[0], 0) + 1
    print(sorted(seen.items(), key=str))
    assert all(seen.get(key, 0) >= 20 for key in (-22, 0, R.SORTED3, R.ALLPAIRS, R.SCAN, R.LISTS, R.F32FILTER, 'split')), seen
    assert seen.get('natural split', 0) >= 1, seen


def test_natural_candidate_split_is_restated(lib):
    """the split rule of the all-pairs kernel on the shapes that trigger it (tables of megabytes per cloud: not among the GPU cases)"""
    hit = set()
    for (B, N, C, ldx, k) in [(32, 2048, 150, 152, 64), (32, 2048, 150, 152, 16), (16, 4096, 8, 8, 8), (8, 8192, 12, 12, 16), (9, 1024, 256, 256, 60),
                              (32, 700, 200, 200, 50), (8, 600, 13, 13, 5), (16, 512, 400, 400, 16)]:
        for res in (0, 64, 192):
            lib.gpe_reserve_cus_set(res)
            sw = R.switches(EXACT=1)
            c = R.Call(X_BASE, B, N, C, ldx, k, 1, 0, 1, WS_BASE, R.ws_bytes(B, N, C, k))
            got = _export(lib, c, sw)
            assert got == R.plan(c, 256 - res, sw), (B, N, C, k, res)
            hit.add(got[1]['nsplit'])
    assert hit >= {1, 2, 4}, hit


def test_layout_is_the_librarys(lib):
    rng = np.random.default_rng(7)
    for it in range(2000):
        B, N, C, k = int(rng.integers(0, 40)), int(rng.integers(1, 9000)), int(rng.integers(1, 400)), int(rng.integers(1, 65))
        w = R.ws_layout(B, N, C)
        assert lib.gpe_knn_ws_bytes(B, N, C, k) == w['total'] == R.ws_bytes(B, N, C, k)
        assert w['sorted_bytes'] <= w['lists_bytes'] <= w['need_f32'] <= w['need_h3'] < w['total'] or not (16 <= C <= 256)
        assert w['sorted_bytes'] <= w['lists_bytes'] and w['iscale'] + 4 * B * N <= w['need_h3']
    for bad in ((-1, 5, 3, 1), (1, 0, 3, 1), (1, 5, 0, 1), (1, 5, 3, 0), (1, 5, 3, 65)):
        assert lib.gpe_knn_ws_bytes(*bad) == -22 == R.ws_bytes(*bad)


_SWITCH_CHILD = '''
import ctypes, sys
sys.path[:0] = [%r, %r]
import knn_restate as R
from gpe_amd import _lib
l = _lib.lib()
sw = R.switches(%s)
arr = (ctypes.c_int * 10)(*sw)
n = 0
for s in R.CASES:
    c = R.call_of(s, 1 << 20, 1 << 30)
    a, b = (ctypes.c_long * 24)(), (ctypes.c_long * 24)()
    args = (c.x, c.B, c.N, c.C, c.ldx, c.k, 1, 0, 1, c.ws or None, c.ws_bytes)
    ra, rb = l.gpe_knn_path(*args, None, ctypes.addressof(a)), l.gpe_knn_path(*args, arr, ctypes.addressof(b))
    assert ra == rb > 0 and list(a) == list(b), (s, ra, rb, list(a), list(b))
    n += (ra, dict(zip(R.PLAN_FIELDS, a))) != R.case_plan(s)
print('switches ok', n)
'''


@pytest.mark.parametrize('env', [dict(GPE_KNN_SPLIT=2, GPE_KNN_VEC=2, GPE_KNN_FT=8, GPE_KNN_PIN=0),
                                 dict(GPE_KNN_EXACT=1, GPE_KNN_SORTED=0, GPE_KNN_NOORDER=1),
                                 dict(GPE_KNN_F32FILTER=1, GPE_KNN_RR2=0, GPE_KNN_PROBE=0)])
def test_null_switches_are_the_process_switches(env, tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    kw = ', '.join('%s=%d' % (k[len('GPE_KNN_'):], v) for k, v in env.items())
    script = tmp_path / 'sw.py'
    script.write_text(_SWITCH_CHILD % (os.path.dirname(here), here, kw))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, GPE_DEBUG='1', **{k: str(v) for k, v in env.items()}),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'switches ok' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split('switches ok')[1]) > 0, 'the variables changed no plan: the comparison shows nothing'


# ----------------------------------------------------------------------------------------------------------------------
# b) coverage
# ----------------------------------------------------------------------------------------------------------------------
def test_case_list_reaches_every_path_and_instance():
    seen, mains = set(), {}
    for s in R.CASES:
        path, p = R.case_plan(s)
        assert path == s.rung, (R.case_id(s), path)
        assert R.main_instance(path, p) == s.main, (R.case_id(s), R.instance(path, p))
        seen |= set(R.instance(path, p))
        mains.setdefault(s.main, []).append(s)
        if path in (R.SCAN, R.LISTS):                       # the GPU test adds a hinted call on these rungs
            hinted = R.case_plan(s, has_order_in=1)
            assert hinted[0] == path and hinted[1]['order'] == (0 if s.group == 'NOORDER' else 1)
            seen |= set(R.instance(*hinted))
        bare = R.case_plan(s, has_idx_glob=0, has_order_out=0)
        assert bare[0] == path and not bare[1]['identity']
    assert seen == R.ALL_INSTANCES, sorted(R.ALL_INSTANCES ^ seen)
    assert {s.rung for s in R.CASES} == {1, 2, 3, 4, 5}
    plans = [(s, R.case_plan(s)) for s in R.CASES]
    # both workgroup widths of the scan under both rechecks; the one-query recheck sorted, unsorted and with pieces behind both filters
    combos = {(R.main_instance(*pl), R.instance(*pl)[-1]) for s, pl in plans if pl[0] == R.SCAN}
    assert combos == {('scan<4>', 'rerank2'), ('scan<8>', 'rerank2'), ('scan<4>', 'rerank(unsorted)'), ('scan<8>', 'rerank(unsorted)')}
    assert {pl[0] for s, pl in plans if R.instance(*pl)[-1] == 'rerank(pieces)'} == {R.LISTS, R.F32FILTER}
    # every piece count, a piece shorter than k and an empty piece, on the all-pairs kernel and behind a filter
    for rungs in ((R.ALLPAIRS,), (R.LISTS, R.F32FILTER)):
        split = [(s, pl[1]) for s, pl in plans if pl[0] in rungs and pl[1]['nsplit'] > 1]
        assert {p['nsplit'] for s, p in split} == {2, 3, 4}
        tps = lambda s, p: R.cdiv(p['tiles'], p['nsplit'])
        assert any((p['nsplit'] - 1) * tps(s, p) * 64 >= s.N for s, p in split), 'no empty piece'
        assert any(0 < s.N - (p['nsplit'] - 1) * tps(s, p) * 64 < s.k for s, p in split), 'no piece shorter than k'
    # the edge kinds run once per rung at least, the fall-backs of every kind are there, pinned and unpinned launches on every rung
    for rung in (1, 2, 3, 4, 5):
        assert any(set(R.EDGE_KINDS) <= set(s.kinds) for s in R.GROUPS['default'] if s.rung == rung), rung
        assert {pl[1]['pin'] for s, pl in plans if pl[0] == rung} == {0, 1}, rung
    assert {s.ws for s in R.GROUPS['default']} == set(R.WS_KINDS)
    assert {(s.ws, s.rung) for s in R.CASES if s.ws != 'full'} >= {('null', R.ALLPAIRS), ('mis8', R.ALLPAIRS), ('f32', R.F32FILTER)}
    # the staging rules: vec 4 / 2 next to a pad (rule A), by the base address, and the fp32 filter's C < 32 branch
    assert any(s.main == 'allpairs<4>' and s.ldx > s.C for s in R.CASES) and any(s.main == 'allpairs<2>' and s.ldx > s.C for s in R.CASES)
    assert any(s.main == 'allpairs<2>' and s.off == 2 and s.C % 4 == 0 and s.ldx % 4 == 0 for s in R.CASES)
    assert any(s.main == 'f32filter<4>' and s.C % 4 for s in R.CASES), 'no fp32-filter vector that straddles C'
    assert any(s.rung == R.F32FILTER and 16 <= s.C < 32 and s.C % 16 for s in R.CASES)
    assert sum(s.N > 600 for s in R.CASES) == 1
    for g in R.GROUPS:
        if g != 'default':
            assert len(R.group_env(g)) >= 2


# ----------------------------------------------------------------------------------------------------------------------
# c) the definition
# ----------------------------------------------------------------------------------------------------------------------
def test_the_oracle_is_the_fp64_search_up_to_near_ties():
    for s in R.CASES:
        if 'gauss' not in s.kinds:
            continue
        x = R.table(s, 'gauss').astype(np.float64).reshape(s.B, s.N, s.C)
        ref = R.reference(s, 'gauss')
        differ, bar = 0, 4 * (s.C + 2) * 2.0 ** -24
        for b in range(s.B):
            n = (x[b] * x[b]).sum(1)
            for q0 in range(0, s.N, 1024):
                xq = x[b, q0:q0 + 1024]
                d = ((xq[:, None, :] - x[b][None, :, :]) ** 2).sum(-1) if s.N * s.C <= 10000 else \
                    np.maximum(n[q0:q0 + 1024, None] + n[None, :] - 2 * xq @ x[b].T, 0)
                order = np.argsort(d, 1, kind='stable')
                mine = np.sort(order[:, :s.k], 1)
                theirs = np.sort(ref[b, q0:q0 + 1024], 1)
                for q in np.nonzero((mine != theirs).any(1))[0]:
                    differ += 1
                    dk, dn = d[q, order[q, s.k - 1]], d[q, order[q, s.k]]
                    assert dn - dk < bar * dk, (R.case_id(s), b, q0 + q, dk, dn)
        assert differ <= 0.01 * s.B * s.N, (R.case_id(s), differ)


# ----------------------------------------------------------------------------------------------------------------------
# d) wrong variants
# ----------------------------------------------------------------------------------------------------------------------
def _rejected(s, kind, name):
    """True / False: check rejects / accepts the variant; None: it cannot change this case"""
    case = R.build(s, kind, 'garbage')
    out = R.wrong(case, name)
    if out is None:
        return None
    assert R.check(case, R.correct(case)) == []
    return bool(R.check(case, out))


def test_check_accepts_the_oracle_and_sees_every_buffer():
    s = R.GROUPS['default'][5]
    case = R.build(s, 'gauss')
    good = R.correct(case)
    assert R.check(case, good, path=R.ALLPAIRS, ws=R.ws_image(s, 0xFF)) == []
    for n in ('idx', 'idx_glob', 'order_out'):
        for where in (R.ZONE - 1, -R.ZONE, R.ZONE):
            bad = {m: a.copy() for m, a in good.items()}
            bad[n][where] = R.PREFILL
            assert R.check(case, bad, path=R.ALLPAIRS), (n, where)
    ws = R.ws_image(s, 0)
    ws[-R.WS_TAIL] = 0
    assert R.check(case, good, ws=ws)
    perm = {m: a.copy() for m, a in good.items()}
    R.payload(perm['order_out'])[:2] = [1, 0]
    assert R.check(case, perm, path=R.ALLPAIRS) and R.check(case, perm, path=R.SORTED3) == []
    R.payload(perm['order_out'])[:2] = [1, 1]
    assert R.check(case, perm, path=R.SORTED3)
    assert R.check(case, good, idx_glob=False) and R.check(case, good, order=False)


@pytest.mark.parametrize('name', [n for n in R.WRONG if n != 'no_recheck'])
def test_wrong_variants_are_rejected(name):
    kind = 'lattice' if name == 'swap_ties' else 'gauss'
    can = {'swap_ties': lambda s: s.N >= 40 and s.k >= 2, 'kth_is_next': lambda s: s.k < s.N, 'row_unsorted': lambda s: s.k >= 2,
           'next_cloud': lambda s: s.B >= 2, 'glob_no_offset': lambda s: s.B >= 2, 'pad_column': lambda s: s.ldx > s.C}[name]
    for s in R.CASES:
        if s.N > 600 or kind not in s.kinds:
            continue
        got = _rejected(s, kind, name)
        assert got is not False, (name, R.case_id(s))
        assert (got is True) == can(s), (name, R.case_id(s), got)


def test_a_missing_recheck_shows_on_every_filter_case():
    """top-k by the fp32 GEMM-form distance differs from the oracle on the clusters or the offset data of every filter-rung case with
    C >= 32: that data would expose a recheck that does not recheck"""
    n = 0
    for s in R.CASES:
        if s.rung in (R.SCAN, R.LISTS, R.F32FILTER) and s.C >= 32:
            got = [_rejected(s, kind, 'no_recheck') for kind in ('clusters', 'offset') if kind in s.kinds]
            assert any(got), (R.case_id(s), got)
            n += 1
    assert n >= 30


# ----------------------------------------------------------------------------------------------------------------------
# e) refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_export_refuses_what_gpe_knn_refuses(lib):
    good = dict(x=X_BASE, B=2, N=130, C=24, ldx=24, k=5, has_idx_glob=1, has_order_in=0, has_order_out=1, ws=WS_BASE, ws_bytes=R.ws_bytes(2, 130, 24, 5))
    assert _export(lib, R.Call(**good), None)[0] == R.SCAN
    idx = (ctypes.c_int * 4)()
    for bad in (dict(x=0), dict(B=-1), dict(N=0), dict(N=-3), dict(C=0), dict(ldx=23), dict(k=0), dict(k=65), dict(k=131), dict(k=-1),
                dict(B=1 << 20, N=1 << 10, k=2), dict(B=(1 << 31) - 1, N=1, k=1, C=3, ldx=3)):
        c = R.Call(**dict(good, **bad))
        assert _export(lib, c, None) == (-22, None) == R.plan(c, 256), bad
        assert _export(lib, c, R.switches(EXACT=1)) == (-22, None), bad
        # ... and so does the entry point, before anything is launched (idx is a host stand-in: a refused call follows no pointer)
        assert lib.gpe_knn(c.x or None, c.B, c.N, c.C, c.ldx, c.k, ctypes.addressof(idx), None, None, None, None, 0, None) == -22, bad
    c = R.Call(**dict(good, B=0))
    assert _export(lib, c, None) == (0, None) == R.plan(c, 256)
    assert lib.gpe_knn(c.x, 0, c.N, c.C, c.ldx, c.k, ctypes.addressof(idx), None, None, None, None, 0, None) == 0
    assert lib.gpe_knn(c.x, 2, c.N, c.C, c.ldx, c.k, None, None, None, None, None, 0, None) == -22      # a NULL idx: the entry point's own
    assert lib.gpe_knn_path(c.x, 2, c.N, c.C, c.ldx, c.k, 1, 0, 1, None, 0, None, None) == R.ALLPAIRS   # plan_out may be NULL

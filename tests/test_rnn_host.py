"""CPU: the restated recurrence ladders, references and bars of tests/rnn_restate.py are checked before any GPU time is spent on them.

a) the restated plans are the library's: fwd_path / bwd_path equal gpe_rnn_seq_fwd_path / gpe_rnn_seq_bwd_path (host only,
   include/gpe_hip.h) — the family and every plan_out number — on every case at 0 and 192 reserved CUs and on a seeded sweep of a few
   thousand random calls over gates, L, T, Bn, H, alignments, workspace present / short / misaligned, tables complete or not, math
   mode 0 / 4 and the debug bits 1024, 2048, 4096, 65536, 131072; the restated workspace queries are the library's and what a launch
   touches of the workspace never exceeds them;
b) every case reaches the family it was written for, under its own process state;
c) the whole-sequence references are torch.nn.LSTM / torch.nn.GRU in fp64 (outputs, final states and, through the gate gradients, the
   weight and input gradients);
d) every bar accepts `emulate`, an fp32 restatement of its family's arithmetic, on random data (the margin it leaves is printed in
   units of the bar); on small-integer data the restated products are exact;
e) every wrong reference is rejected on every family that has a case it changes;
f) ACT_ULPS is four times what torch's CPU fp32 sigmoid / tanh differ from fp64 over the cases' own pre-activations;
g) the exports refuse what the entry points refuse."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rnn_restate as R
from gpe_amd import _lib

_BUF = (ctypes.c_double * 64)()
_BASE = (ctypes.addressof(_BUF) + 63) // 64 * 64          # host memory stands in for device buffers: the exports never follow a pointer
HS, WS = _BASE, _BASE + 128
GROUP_FAMILY = {'persist_fwd': R.PERSIST, 'multi_fwd': R.MULTI, 'diag_fwd': R.DIAG, 'persist_bwd': R.PERSIST, 'diag_bwd': R.DIAG}
ALL = [(g, c) for g in R.CASES for c in R.CASES[g]]
_ids = [g + ':' + R.case_id(c) for g, c in ALL]


@pytest.fixture
def state():
    """the process state the plans read, restored afterwards"""
    l = _lib.lib()
    math, dbg = l.gpe_math_get(), l.gpe_debug_get()
    res = l.gpe_reserve_cus_set(0)
    yield l
    l.gpe_reserve_cus_set(res)
    l.gpe_debug_set(dbg)
    l.gpe_math_set(math)


def _set(l, st):
    l.gpe_math_set(st.math)
    l.gpe_debug_set(st.debug)
    l.gpe_reserve_cus_set(st.reserved)


def _export(l, fwd, args):
    out = (ctypes.c_long * len(R.PLAN_FIELDS))(*([-5] * len(R.PLAN_FIELDS)))
    rc = (l.gpe_rnn_seq_fwd_path if fwd else l.gpe_rnn_seq_bwd_path)(*args, ctypes.addressof(out))
    return rc, (dict(zip(R.PLAN_FIELDS, out)) if rc > 0 else list(out))


def _both(l, fwd, args, st):
    _set(l, st)
    got = _export(l, fwd, args)
    want = (R.fwd_path if fwd else R.bwd_path)(*args, st)
    if want[0] < 0:
        assert got[0] == -22 and got[1] == [-5] * len(R.PLAN_FIELDS), (args, st, got)     # plan_out is written only with a family
    else:
        assert got == want, (args, st, got, want)
    G, L, T, Bn, H = args[:5]
    if R._dims_ok(G, L, T, Bn, H):
        assert l.gpe_rnn_seq_fwd_ws(G, L, T, Bn, H) == R.fwd_ws(G, L, T, Bn, H, st)
        assert l.gpe_rnn_seq_bwd_ws(G, L, T, Bn, H) == R.bwd_ws(G, L, T, Bn, H, st)
        if want[0] > 0:                                                                  # what a launch touches never exceeds the query
            assert want[1]['ws_used'] <= (R.fwd_ws if fwd else R.bwd_ws)(G, L, T, Bn, H, st)
    return want


def _args(group, c, st=None):
    fwd = group.endswith('fwd')
    if st is not None:
        c = R.dataclasses.replace(c, reserved=st.reserved)
    return fwd, (R.fwd_path_args(c, HS, WS) if fwd else R.bwd_path_args(c, HS, WS))


@pytest.mark.parametrize('group, case', ALL, ids=_ids)
def test_every_case_reaches_its_family_and_the_restated_plan_is_the_librarys(state, group, case):
    fwd, args = _args(group, case)
    fam, plan = _both(state, fwd, args, case.state)
    assert fam == case.family == GROUP_FAMILY[group], (R.case_id(case), R.FAMILY.get(fam, fam), plan)
    for reserved in (0, R.R64):
        st = R.State(case.math, case.debug, reserved)
        _both(state, *_args(group, case, st), st)


def test_the_hand_derived_plans_of_the_multi_tile_cases():
    """the numbers the cases were chosen for (64 usable CUs)"""
    st = R.State(4, 0, R.R64)
    a = R.pm_plan(4, 4, 3, 80, 64, st)
    assert (a['rgmax'], a['NRT'], a['RG']) == (4, 5, 2)
    b = R.pm_plan(4, 4, 3, 309, 64, st)
    assert (b['NRT'], b['RG']) == (20, 3) and R.cdiv(b['NRT'], b['RG']) == 7
    assert R.cdiv(R.cdiv(R.cdiv(1025, 16), R.pm_plan(4, 4, 2, 1025, 64, st)['RG']), R.PM_NW) > R.PM_MAXQ
    assert R.ps_plan(4, 4, 2, 80, 64, False, R.State(0, 0, R.R64)) is None and R.ps_plan(4, 4, 2, 80, 64, False, R.State(0, 2048, R.R64))


def test_seeded_sweep_of_random_calls(state):
    rng = np.random.default_rng(20240611)
    bits = (1024, 2048, 4096, 65536, 131072)
    seen = {}
    for it in range(4000):
        G = int(rng.choice([3, 4, 4, 4]))
        L, T = int(rng.integers(1, 7)), int(rng.choice([1, 2, 3, 5, 14, 23]))
        Bn = int(rng.choice([1, 5, 16, 17, 32, 33, 64, 65, 80, 192, 193, 309, 736, 1025, 2000]))
        H = int(rng.choice([1, 15, 16, 17, 32, 40, 64, 128, 129, 250, 256, 257, int(rng.integers(1, 301))]))
        st = R.State(int(rng.choice([0, 4])), int(sum(b for b in bits if rng.random() < 0.25)), int(rng.choice([0, 0, 64, R.R64])))
        packs, planes = int(rng.choice([16, 16, 16, 8, 0])), int(rng.choice([16, 16, 16, 8, 0]))
        fwd = bool(rng.random() < 0.5)
        off = int(rng.choice([0, 0, 0, 4, 8]))
        sl_odd = 2 * int(rng.random() < 0.1)
        friendly = rng.random() < 0.5          # half of the calls keep away from most refusals, so that the persistent plans are drawn
        if friendly:
            G, L, packs, planes, off, sl_odd = 4, int(rng.integers(1, 5)), 16, 16, 0, 0
            H = int(rng.choice([20, 30, 50, 64, 250, 256, int(rng.integers(1, 257))]))
            st = R.State(int(rng.choice([0, 4, 4])), int(sum(b for b in bits if rng.random() < 0.08)), st.reserved)
        if fwd:
            Hp = R.rup(H, 4) + 4 * int(rng.integers(0, 2))
            hs_sb = (T + 1) * Hp
            need = R.fwd_ws(G, L, T, Bn, H, st)
            ws_kind = 'ok' if friendly else rng.choice(['ok', 'ok', 'ok', 'short', 'none', 'off4', 'off8'])
            ws = 0 if ws_kind == 'none' else WS + (4 if ws_kind == 'off4' else 8 if ws_kind == 'off8' else 0)
            nbytes = need - 4 if ws_kind == 'short' else need + 64 * int(rng.integers(0, 2))
            args = (G, L, T, Bn, H, HS + off, Bn * hs_sb + sl_odd, hs_sb, Hp, packs, planes, int(rng.random() < 0.9), ws, int(nbytes))
        else:
            GHp = R.rup(G * H, 4)
            args = (G, L, T, Bn, H, HS + off, Bn * T * GHp + sl_odd, T * GHp, GHp, WS + int(rng.choice([0, 0, 4])), packs, planes)
        fam, plan = _both(state, fwd, args, st)
        seen[fwd, fam] = seen.get((fwd, fam), 0) + 1
    assert all(seen.get(k, 0) >= 50 for k in ((True, 1), (True, 2), (True, 3), (False, 1), (False, 3))), seen


def test_exports_refuse_what_the_entry_points_refuse(state):
    l = state
    good = (4, 2, 3, 17, 20, HS, 17 * 4 * 20, 4 * 20, 20, 16, 16, 1, WS, 1 << 20)
    assert l.gpe_rnn_seq_fwd_path(*good, None) == R.PERSIST
    for pos, bad in ((0, 5), (0, 2), (1, 0), (2, 0), (3, 0), (4, 0), (5, None), (7, 82), (8, 22), (9, -1), (10, -1)):
        args = list(good)
        args[pos] = bad
        assert l.gpe_rnn_seq_fwd_path(*args, None) == -22, (pos, bad)
    goodb = (4, 2, 3, 17, 20, HS, 17 * 3 * 80, 3 * 80, 80, WS, 16, 16)
    assert l.gpe_rnn_seq_bwd_path(*goodb, None) == R.PERSIST
    for pos, bad in ((0, 1), (1, 0), (2, -1), (3, 0), (4, 0), (5, None), (7, 242), (8, 82), (9, None), (10, -1), (11, -1)):
        args = list(goodb)
        args[pos] = bad
        assert l.gpe_rnn_seq_bwd_path(*args, None) == -22, (pos, bad)
    # the entry points themselves answer -22 to the same dimensions and pitches before anything is launched
    assert l.gpe_rnn_seq_fwd(4, 2, 3, 17, 20, None, 0, 0, None, None, None, None, None, 0, 82, 20, None, 0, 0, None, 0, 0, None, None,
                             None, None, None, 0, None) == -22


# ---- references -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(group, case):
    return R.make_problem(case)


@functools.lru_cache(maxsize=None)
def _emulated(group, case):
    """(forward history, backward or None) in fp32 as the group's family computes them"""
    p = _problem(group, case)
    fam = GROUP_FAMILY[group]
    if group in R.FORWARD:
        return R.emulate_fwd(p, fam), None
    fam = R.HISTORY_OF[group]
    f = R.emulate_fwd(p, fam, f16=case.f16)
    return f, R.emulate_bwd(p, f, fam)


def _torch_rnn(p):
    c = p.case
    m = (torch.nn.LSTM if c.gates == 4 else torch.nn.GRU)(p.x.shape[-1], c.H, c.L, batch_first=True).double()
    with torch.no_grad():
        for l in range(c.L):
            getattr(m, 'weight_ih_l%d' % l).copy_(torch.from_numpy(p.w_ih[l]))
            getattr(m, 'weight_hh_l%d' % l).copy_(torch.from_numpy(p.w_hh[l]))
            getattr(m, 'bias_ih_l%d' % l).copy_(torch.from_numpy(p.b_ih[l]))
            getattr(m, 'bias_hh_l%d' % l).copy_(torch.from_numpy(p.b_hh[l]))
    return m


@pytest.mark.parametrize('group, idx', [('persist_fwd', 2), ('diag_fwd', 1), ('diag_fwd', 10), ('persist_bwd', 1), ('diag_bwd', 0), ('diag_bwd', 8)])
def test_whole_sequence_references_are_torchs(group, idx):
    """ref_fwd / ref_bwd against torch.nn.LSTM / GRU with autograd in fp64.  (xproj0 is rounded to fp32 as the kernels receive it: 1e-7)"""
    case = R.CASES[group][idx]
    p = R.make_problem(case)
    c = case
    m = _torch_rnn(p)
    x = torch.from_numpy(np.broadcast_to(p.x, (c.Bn, c.T, p.x.shape[-1])).copy()).requires_grad_(True)
    h0 = torch.from_numpy(p.h0)
    st0 = (h0, torch.from_numpy(p.c0)) if c.gates == 4 else h0
    y, stN = m(x, st0)
    ref = R.ref_fwd(p)
    assert R.whole_seq(ref['hs'][c.L - 1, :, 1:], y.detach().numpy()) < 1e-6
    hN = (stN[0] if c.gates == 4 else stN).detach().numpy()
    assert R.whole_seq(ref['hs'][:, :, c.T], hN) < 1e-6
    if c.gates == 4:
        assert R.whole_seq(ref['cs'][:, c.T], stN[1].detach().numpy()) < 1e-6
    loss = 0
    if p.dtop is not None:
        loss = loss + (y * torch.from_numpy(p.dtop)).sum()
    if p.d_hN is not None:
        loss = loss + ((stN[0] if c.gates == 4 else stN) * torch.from_numpy(p.d_hN)).sum()
    if p.d_cN is not None:
        loss = loss + (stN[1] * torch.from_numpy(p.d_cN)).sum()
    loss.backward()
    b = R.ref_bwd(p, ref)
    GH = c.gates * c.H
    for l in range(c.L):
        gx, gh = b['dgx'][l].reshape(-1, GH), b['dgh'][l].reshape(-1, GH)
        src = np.broadcast_to(p.x, (c.Bn, c.T, p.x.shape[-1])) if l == 0 else ref['hs'][l - 1][:, 1:]
        assert R.whole_seq(gx.T @ src.reshape(c.Bn * c.T, -1), getattr(m, 'weight_ih_l%d' % l).grad.numpy()) < 1e-6, l
        assert R.whole_seq(gh.T @ ref['hs'][l][:, :c.T].reshape(c.Bn * c.T, -1), getattr(m, 'weight_hh_l%d' % l).grad.numpy()) < 1e-6, l
        assert R.whole_seq(gh.sum(0), getattr(m, 'bias_hh_l%d' % l).grad.numpy()) < 1e-6, l
    assert R.whole_seq(b['dgx'][0] @ p.w_ih[0], x.grad.numpy()) < 1e-6


GPU_ALL = [(g, c) for g in R.CASES for c in R.gpu_cases(g)]
_gids = [g + ':' + R.case_id(c) for g, c in GPU_ALL]


@pytest.mark.parametrize('group, case', GPU_ALL, ids=_gids)
def test_every_bar_accepts_the_fp32_restatement_of_its_family(group, case):
    p = _problem(group, case)
    f, b = _emulated(group, case)
    w = R.check_fwd(p, f) if b is None else R.check_bwd(p, f, b)
    print('%s %s: emulate leaves %s' % (group, R.case_id(case), w))
    assert w.worst < 1.0, str(w)
    ref = R.ref_fwd(p)
    if b is None:
        assert R.whole_seq(f['hs'], ref['hs']) < R.SEQ_FWD_BAR and R.whole_seq(f['saved'], ref['saved']) < R.SEQ_FWD_BAR
    else:
        want = R.ref_bwd(p, ref)
        assert R.whole_seq(b['dgx'], want['dgx']) < R.SEQ_BWD_BAR and R.whole_seq(b['carry0'], want['carry0']) < R.SEQ_BWD_BAR


def test_emulate_margins_by_family(capsys):
    """the worst figure `emulate` leaves per family and direction, in bars (profiles/rnn_tests.md records them)"""
    for group in R.CASES:
        worst = 0.0
        for case in R.gpu_cases(group):
            p = _problem(group, case)
            f, b = _emulated(group, case)
            worst = max(worst, (R.check_fwd(p, f) if b is None else R.check_bwd(p, f, b)).worst)
        with capsys.disabled():
            print('\n  emulate, %-12s worst %.3f bars' % (group, worst), end='')
        assert worst < 1.0


@pytest.mark.parametrize('family', [R.PERSIST, R.MULTI, R.DIAG])
@pytest.mark.parametrize('f16', [False, True])
def test_restated_products_are_exact_on_small_integers(family, f16):
    rng = np.random.default_rng(7)
    for Bn, K, N in ((5, 20, 80), (33, 130, 24), (17, 257, 8)):
        a = rng.integers(-2, 3, size=(Bn, K)).astype(np.float64)
        w = rng.integers(-2, 3, size=(N, K)).astype(np.float64)
        got = R._product32(a, w, family, f16, Bn, sa=R.STATE_SA)
        assert np.array_equal(got.astype(np.float64), a @ w.T)
    # ... and so is a whole cell's pre-activation in the checker's restatement
    case = R.CASES['persist_fwd'][2]
    p = R.make_problem(case, integer=True)
    zx, zh, S = R._cell_pre(p, 1, 0, p.h0[1], p.h0[0])
    assert np.array_equal(zx + zh, np.rint(zx + zh)) and np.all(S >= np.abs(zx + zh))


@pytest.mark.parametrize('group', ['persist_fwd', 'multi_fwd', 'persist_bwd'])
def test_two_families_agree_element_by_element_and_a_wrong_unit_shows(group):
    """R.agree on the fp32 restatements of a persistent family and of the diagonals: inside the sum of the per-cell bars (plus what the
    consumed rows' difference propagates); one unit of a ragged unit block moved by four times its own bar in one run is seen"""
    for case in R.gpu_cases(group):
        p = _problem(group, case)
        f, b = _emulated(group, case)
        if b is None:
            fd = R.emulate_fwd(p, R.DIAG)
            wa, wb = R.check_fwd(p, f), R.check_fwd(p, fd)
            name, arr = 'saved', f['saved']
        else:
            bd = R.emulate_bwd(p, f, R.DIAG, f16=False)
            wa, wb = R.check_bwd(p, f, b), R.check_bwd(p, f, bd, f16=False)
            name, arr = 'dgx', b['dgx']
        w = R.agree(wa, wb)
        print('%s %s: the two restatements agree within %s' % (group, R.case_id(case), w))
        assert w.worst < 1.0, str(w)
        # the last unit of the last row of the last cell of layer 0
        at = (0, case.T - 1) if b is None else (0, 0)
        got, want, bar = wa.cells[name, at]
        moved = got.copy()
        moved[-1, case.H - 1] += 4 * (bar[-1, case.H - 1] + wb.cells[name, at][2][-1, case.H - 1])
        wa.cells[name, at] = (moved, want, bar)
        assert R.agree(wa, wb).worst > 1.0


@pytest.mark.parametrize('name', list(R.VARIANTS))
def test_every_wrong_reference_is_rejected(name):
    direction, changes = R.VARIANTS[name]
    hit = 0
    for group in (R.FORWARD if direction == 'fwd' else R.BACKWARD):
        cases = [c for c in R.gpu_cases(group) if changes(c)]
        for case in cases:
            p = _problem(group, case)
            f, b = _emulated(group, case)
            w = R.check_fwd(p, f, variant=name) if b is None else R.check_bwd(p, f, b, variant=name)
            assert w.worst > 1.0, (name, group, R.case_id(case), str(w))
            hit += 1
    assert hit > 0
    if name != 'bhn_outside':                      # (only the diagonals run a GRU)
        for group in (R.FORWARD if direction == 'fwd' else R.BACKWARD):
            assert any(changes(c) for c in R.gpu_cases(group)), (name, group)


def test_activation_multiple():
    """ACT_ULPS = 4 x the worst difference of torch's CPU fp32 sigmoid / tanh against fp64, in ulps of the value, over the
    pre-activations of every case (and the cell states tanh is taken of)"""
    sig, tanh = [], []
    for group in R.FORWARD:
        for case in R.gpu_cases(group):
            p = _problem(group, case)
            ref = R.ref_fwd(p)
            H = case.H
            for l in range(case.L):
                for t in range(case.T):
                    zx, zh, _ = R._cell_pre(p, l, t, ref['hs'][l, :, t], ref['hs'][l - 1, :, t + 1] if l else None)
                    if case.gates == 4:
                        z = zx + zh
                        sig += [z[:, :2 * H].ravel(), z[:, 3 * H:].ravel()]
                        tanh += [z[:, 2 * H:3 * H].ravel(), ref['cs'][l, t + 1].ravel()]
                    else:
                        sig.append((zx + zh)[:, :2 * H].ravel())
                        tanh.append((zx[:, 2 * H:] + ref['saved'][l, t][:, :H] * ref['saved'][l, t][:, 3 * H:]).ravel())
    s, t = R.activation_ulps(np.concatenate(sig), np.concatenate(tanh))
    print('torch CPU fp32 against fp64 over %d + %d pre-activations: sigmoid %.3f ulp, tanh %.3f ulp' % (sum(map(len, sig)), sum(map(len, tanh)), s, t))
    assert 4 * max(s, t) <= R.ACT_ULPS, (s, t)
    assert 4 * max(s, t) > R.ACT_ULPS / 4, 'ACT_ULPS is far above the measurement it stands for: %r' % ((s, t),)

"""-m gpu: the recurrence kernels family by family through the C ABI (gpe_rnn_seq_fwd / gpe_rnn_seq_bwd, called through _lib with raw
buffers) against the fp64 references of tests/rnn_restate.py: cases, layouts, references, checkers and the derivation of their bars
are there, and tests/test_rnn_host.py checks them on the CPU first (the restated plans are the library's, every case reaches its
family, every bar accepts an fp32 restatement of its family and every wrong reference is rejected).

One test per family and direction, parametrised over that family's cases.  Packs come from the library's own pack entry points as ops
builds them (pack_gates, pack_weight, a PackPlan for the fp16 planes).  Every case runs twice on freshly pre-filled buffers:
  - gpe_rnn_seq_fwd_path / _bwd_path, asked with the device's own pointers, names the family the case was written for, and its plan
    is the restated one;
  - the two runs are bit-identical in every output (every family promises a fixed summation order);
  - every cell is recomputed in fp64 from what the kernel itself produced and consumed, every element against its own bar
    (rnn_restate.check_fwd / check_bwd), and the whole sequence meets the project's 2e-5 / 1e-4 bars against the fp64 reference;
  - NaN prefill: hs slots 1 .. T, cs slots 1 .. T, saved, dgx / dgh, carry, the forward workspace (the multi-tile kernel's published
    state planes lie there) and `part` are NaN before each launch, and so is everything the contract of include/gpe_hip.h says is not
    read as a value: the pad columns of the hs rows, every gap of a strided layout, the targets of the unused table entries.  No NaN
    may come out: a cell that reads a row before its producer published it shows;
  - sentinels: everything outside what the contract says is written — hs pad columns and slot / row / layer gaps, hs slot 0 and cs
    slot 0, the gaps of strided cs / saved / dgx, the bytes behind gpe_rnn_seq_fwd_ws and the floats behind gpe_rnn_seq_bwd_ws —
    comes back bit for bit;
  - a case written in f16x3 mode with incomplete plane tables gives the bits of mode 0, forward and backward; a persistent family's
    outputs agree with the diagonals' on the same case ELEMENT BY ELEMENT within the sum of the two families' per-cell bars, plus, where
    the two cells consumed different rows, exactly what that difference propagates to the element (rnn_restate.agree).
The backward cases run on a history made by the same family's forward (the diagonals' where the family has none).  The math mode, the
debug word and the CU reservation are restored in `finally`.  Worst figures observed on an MI355X are in profiles/rnn_tests.md."""
import ctypes

import numpy as np
import pytest
import torch

import rnn_restate as R

pytestmark = pytest.mark.gpu
NAN = float('nan')
TAIL = 256                                    # bytes / floats of sentinel behind a workspace


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _cases(group):
    return pytest.mark.parametrize('case', R.gpu_cases(group), ids=R.case_id)


class _State:
    """the process state of a case, the previous one restored on exit"""

    def __init__(self, gpe, math, debug, reserved):
        self.l, self.want = gpe._lib.lib(), (math, debug, reserved)

    def __enter__(self):
        l = self.l
        self.prev = (l.gpe_math_get(), l.gpe_debug_get(), l.gpe_reserve_cus_set(0))
        l.gpe_math_set(self.want[0])
        l.gpe_debug_set(self.want[1])
        l.gpe_reserve_cus_set(self.want[2])
        return self

    def __exit__(self, *exc):
        self.l.gpe_math_set(self.prev[0])
        self.l.gpe_debug_set(self.prev[1])
        self.l.gpe_reserve_cus_set(self.prev[2])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _view(flat, shape, strides):
    """a strided view of a flat host array (strides in elements)"""
    return np.lib.stride_tricks.as_strided(flat, shape=shape, strides=tuple(s * flat.itemsize for s in strides))


def _bits(a):
    return a.view(np.uint32)


class Weights:
    """the operands of a stack on the device, packed by the library as ops packs them.  Lives through a test: the packs of a PackPlan
    are keyed by the parameters' addresses"""

    def __init__(self, gpe, p, planes):
        ops = gpe.ops
        c = p.case
        G, L, H = c.gates, c.L, c.H
        self.nan = torch.full((64,), NAN, device='cuda')                     # what an unused table entry points at
        self.w_hh = [_dev(p.w_hh[l]) for l in range(L)]
        self.w_ih = [_dev(p.w_ih[l]) for l in range(L)]
        self.bias = [self.nan] + [_dev(p.bias[l]) for l in range(1, L)]
        self.bhn = None if G == 4 else [_dev(p.bhn[l]) for l in range(L)]
        self.whh = [ops.pack_gates(w, H, G) for w in self.w_hh]
        self.wih = [self.nan] + [ops.pack_gates(w, H, G) for w in self.w_ih[1:]]
        self.whh_t = [ops.pack_weight(w, transpose=True) for w in self.w_hh]
        self.wih_t = [self.nan] + [ops.pack_weight(w, transpose=True) for w in self.w_ih[1:]]
        self.fwd_planes = self.bwd_planes = ops.NO_PLANES
        if planes and c.math == 4:
            # the plan's launches fill the planes only in f16x3 mode
            with _State(gpe, 4, 0, 0):
                self.plan = ops.PackPlan()
                for w in self.w_hh + self.w_ih[1:]:
                    self.plan.add_gates(w, H, G)
                self.plan.refresh()
                torch.cuda.synchronize()
                self.fwd_planes = self._planes(ops, ops.K_GATES_H3)
                self.bwd_planes = self._planes(ops, ops.K_TRANS_H3) if G == 4 else ops.NO_PLANES

    def _planes(self, ops, kind):
        hh = [ops.planned_planes(w, kind) for w in self.w_hh]
        ih = [ops.planned_planes(w, kind) for w in self.w_ih[1:]]
        assert all(t is not None for pair in hh + ih for t in pair)
        return [a for a, _ in hh], [self.nan] + [a for a, _ in ih], [b for _, b in hh], [self.nan] + [b for _, b in ih]


def _tables(ops, lists):
    return [None if ts is None else ops._ptr_array(ts) for ts in lists]


def _plan(gpe, fwd, args):
    out = (ctypes.c_long * len(R.PLAN_FIELDS))()
    fam = gpe._lib.query('gpe_rnn_seq_fwd_path' if fwd else 'gpe_rnn_seq_bwd_path', *args, ctypes.addressof(out))
    return fam, dict(zip(R.PLAN_FIELDS, out))


def _device_state(c, debug=None):
    return R.State(c.math, c.debug if debug is None else debug, c.reserved, torch.cuda.get_device_properties(0).multi_processor_count)


def _check_untouched(name, before, after, written):
    same = _bits(before)[~written] == _bits(after)[~written]
    assert same.all(), '%s: %d elements outside the written region changed, first at flat index %d' % (
        name, int((~same).sum()), int(np.flatnonzero(~written)[np.argmin(same)]))
    assert not np.isnan(after[written]).any(), '%s: NaN came out (%d elements)' % (name, int(np.isnan(after[written]).sum()))


def run_forward(gpe, c, p, W, family, debug=None, math=None):
    """gpe_rnn_seq_fwd on freshly pre-filled buffers, twice -> dense host arrays hs, cs, saved (what the checkers take)"""
    L_ = gpe._lib
    G, L, T, Bn, H = c.gates, c.L, c.T, c.Bn, c.H
    lay = R.layout(c)
    st = _device_state(c, debug)
    if math is not None:
        st = R.dataclasses.replace(st, math=math)
    cc = R.dataclasses.replace(c, debug=st.debug, math=st.math)
    with _State(gpe, st.math, st.debug, st.reserved):
        # ---- host images: NaN everywhere but the start states and the layer-0 addends
        hs0 = np.full(lay['hs_n'] + 64, NAN, np.float32)
        _view(hs0, (L, Bn, H), (lay['hs_sl'], lay['hs_sb'], 1))[...] = p.h0
        hs_w = np.zeros(hs0.shape, bool)
        _view(hs_w[lay['hs_st']:], (L, Bn, T, H), (lay['hs_sl'], lay['hs_sb'], lay['hs_st'], 1))[...] = True
        cs0 = cs_w = None
        if G == 4:
            cs0 = np.full(lay['cs_n'] + 64, NAN, np.float32)
            _view(cs0, (L, Bn * H), (lay['cs_sl'], 1))[...] = p.c0.reshape(L, -1)
            cs_w = np.zeros(cs0.shape, bool)
            _view(cs_w[lay['cs_st']:], (L, T, Bn * H), (lay['cs_sl'], lay['cs_st'], 1))[...] = True
        sv0 = np.full(lay['sv_n'] + 64, NAN, np.float32)
        sv_w = np.zeros(sv0.shape, bool)
        _view(sv_w, (L, T, Bn * 4 * H), (lay['sv_sl'], lay['sv_st'], 1))[...] = True
        xp = np.full(lay['xp_n'] + 64, NAN, np.float32)
        Tx = T if c.seq else 1
        _view(xp, (Bn, Tx, G * H), (lay['xp0_sb'], lay['xp0_st'] or 1, 1))[...] = p.xproj0[:, :Tx]
        need = L_.query('gpe_rnn_seq_fwd_ws', G, L, T, Bn, H)
        assert need == R.fwd_ws(G, L, T, Bn, H, st, True)
        given = R.ws_bytes_given(cc, True)
        d_xp = torch.from_numpy(xp).cuda()
        tabs = _tables(gpe.ops, (W.whh, W.wih, W.bias, W.bhn))
        ptabs = _tables(gpe.ops, W.fwd_planes)
        runs = []
        for rep in range(2):
            d_hs, d_sv = torch.from_numpy(hs0).cuda(), torch.from_numpy(sv0).cuda()
            d_cs = torch.from_numpy(cs0).cuda() if G == 4 else None
            ws_all = torch.full((need + TAIL + 64,), 0xFF, dtype=torch.uint8, device='cuda')
            ws = None if c.ws == 'none' else ws_all[c.ws_off:]
            fam, plan = _plan(gpe, True, R.fwd_path_args(cc, d_hs.data_ptr(), ws_all.data_ptr(), True))
            want = R.fwd_path(*R.fwd_path_args(cc, d_hs.data_ptr(), ws_all.data_ptr(), True), st, True)
            assert (fam, plan) == want, (R.case_id(c), fam, plan, want)
            assert fam == family, '%s: the export says %s, wanted %s: %r' % (R.case_id(c), R.FAMILY.get(fam, fam), R.FAMILY[family], plan)
            L_.call('gpe_rnn_seq_fwd', G, L, T, Bn, H, d_xp, lay['xp0_sb'], lay['xp0_st'], *tabs, d_hs, lay['hs_sl'], lay['hs_sb'],
                    lay['hs_st'], d_cs, lay['cs_sl'], lay['cs_st'], d_sv, lay['sv_sl'], lay['sv_st'], *ptabs, ws, given)
            torch.cuda.synchronize()
            out = dict(hs=d_hs.cpu().numpy(), sv=d_sv.cpu().numpy(), cs=d_cs.cpu().numpy() if G == 4 else None)
            assert plan['ws_used'] <= need
            tail = ws_all[c.ws_off + plan['ws_used']:].cpu().numpy()           # (the diagonal launches touch nothing of it)
            assert (tail == 0xFF).all(), 'bytes behind what the plan says the launch touches of the workspace were written'
            runs.append(out)
        a, b = runs
        for k in ('hs', 'sv', 'cs'):
            if a[k] is not None:
                assert a[k].tobytes() == b[k].tobytes(), '%s: two runs differ in %s' % (R.case_id(c), k)
        _check_untouched('hs', hs0, a['hs'], hs_w)
        _check_untouched('saved', sv0, a['sv'], sv_w)
        if G == 4:
            _check_untouched('cs', cs0, a['cs'], cs_w)
        dense = dict(hs=_view(a['hs'], (L, Bn, T + 1, H), (lay['hs_sl'], lay['hs_sb'], lay['hs_st'], 1)).copy(),
                     saved=_view(a['sv'], (L, T, Bn, 4 * H), (lay['sv_sl'], lay['sv_st'], 4 * H, 1)).copy(),
                     cs=_view(a['cs'], (L, T + 1, Bn, H), (lay['cs_sl'], lay['cs_st'], H, 1)).copy() if G == 4 else None)
        dense['flat'] = a
        dense['f16'] = bool(plan['f16'])
        return dense


def run_backward(gpe, c, p, W, fwd, family):
    """gpe_rnn_seq_bwd on the history `fwd` (run_forward's result), twice -> dense dgx, dgh, carry0"""
    L_ = gpe._lib
    G, L, T, Bn, H = c.gates, c.L, c.T, c.Bn, c.H
    lay = R.layout(c)
    st = _device_state(c)
    GH = G * H
    with _State(gpe, st.math, st.debug, st.reserved):
        dg0 = np.full(lay['dg_n'] + 64, NAN, np.float32)
        dg_w = np.zeros(dg0.shape, bool)
        _view(dg_w, (L, Bn, T, GH), (lay['dg_sl'], lay['dg_sb'], lay['dg_st'], 1))[...] = True
        d_top = None
        if p.dtop is not None:
            dt = np.full(lay['dt_n'] + 64, NAN, np.float32)
            _view(dt, (Bn, T, H), (lay['dt_sb'], lay['dt_st'], 1))[...] = p.dtop
            d_top = torch.from_numpy(dt).cuda()
        d_hN = None if p.d_hN is None else _dev(p.d_hN)
        d_cN = None if p.d_cN is None else _dev(p.d_cN)
        d_hs, d_sv = torch.from_numpy(fwd['flat']['hs']).cuda(), torch.from_numpy(fwd['flat']['sv']).cuda()
        d_cs = torch.from_numpy(fwd['flat']['cs']).cuda() if G == 4 else None
        need = L_.query('gpe_rnn_seq_bwd_ws', G, L, T, Bn, H)
        assert need == R.bwd_ws(G, L, T, Bn, H, st, True)
        tabs = _tables(gpe.ops, (W.whh_t, W.wih_t))
        ptabs = _tables(gpe.ops, W.bwd_planes)
        runs = []
        for rep in range(2):
            d_gx = torch.from_numpy(dg0).cuda()
            d_gh = d_gx if G == 4 else torch.from_numpy(dg0).cuda()
            part_all = torch.full((need + TAIL + 16,), NAN, device='cuda')
            part = part_all[c.part_off // 4:]
            carry = torch.full((2, L, Bn, H), NAN, device='cuda')
            args = R.bwd_path_args(R.dataclasses.replace(c, part_off=0), d_gx.data_ptr(), part.data_ptr())
            fam, plan = _plan(gpe, False, args)
            want = R.bwd_path(*args, st, True)
            assert (fam, plan) == want, (R.case_id(c), fam, plan, want)
            assert fam == family, '%s: the export says %s, wanted %s: %r' % (R.case_id(c), R.FAMILY.get(fam, fam), R.FAMILY[family], plan)
            L_.call('gpe_rnn_seq_bwd', G, L, T, Bn, H, d_top, lay['dt_sb'], lay['dt_st'], d_hN, d_cN, *tabs, d_hs, lay['hs_sl'],
                    lay['hs_sb'], lay['hs_st'], d_cs, lay['cs_sl'], lay['cs_st'], d_sv, lay['sv_sl'], lay['sv_st'], d_gx, d_gh,
                    lay['dg_sl'], lay['dg_sb'], lay['dg_st'], part, carry, *ptabs)
            torch.cuda.synchronize()
            tail = part[need:].cpu().numpy()
            assert np.isnan(tail).all(), 'floats behind gpe_rnn_seq_bwd_ws were written'
            assert np.isnan(part[plan['ws_used']:need].cpu().numpy()).all(), 'the launch wrote past what its plan says it touches'
            runs.append(dict(gx=d_gx.cpu().numpy(), gh=d_gh.cpu().numpy(), carry=carry.cpu().numpy()))
            # the history is read only
            assert d_hs.cpu().numpy().tobytes() == fwd['flat']['hs'].tobytes() and d_sv.cpu().numpy().tobytes() == fwd['flat']['sv'].tobytes()
        a, b = runs
        for k in ('gx', 'gh'):
            assert a[k].tobytes() == b[k].tobytes(), '%s: two runs differ in %s' % (R.case_id(c), k)
        assert a['carry'][0].tobytes() == b['carry'][0].tobytes(), '%s: two runs differ in carry[0]' % R.case_id(c)
        _check_untouched('dgx', dg0, a['gx'], dg_w)
        _check_untouched('dgh', dg0, a['gh'], dg_w)
        assert not np.isnan(a['carry'][0]).any(), 'carry[0]: NaN came out'
        shape, strides = (L, Bn, T, GH), (lay['dg_sl'], lay['dg_sb'], lay['dg_st'], 1)
        return dict(dgx=_view(a['gx'], shape, strides).copy(), dgh=_view(a['gh'], shape, strides).copy(), carry0=a['carry'][0].copy(),
                    f16=bool(plan['f16']))


def _report(group, c, family, w, seq):
    print('RNNFIG %s %s family %d (%s): %s; whole sequence %s' % (group, R.case_id(c), family, R.FAMILY[family], w,
                                                                ', '.join('%s %.2e' % kv for kv in seq.items())))


def _forward_case(gpe, group, c, family):
    p = R.make_problem(c)
    W = Weights(gpe, p, c.planes)
    out = run_forward(gpe, c, p, W, family)
    assert out['f16'] == c.f16
    w = R.check_fwd(p, out, f16=out['f16'])
    ref = R.ref_fwd(p)
    seq = {k: R.whole_seq(out[k], ref[k]) for k in ('hs', 'saved', 'cs') if out[k] is not None}
    _report(group, c, family, w, seq)
    assert w.worst < 1.0, str(w)
    assert max(seq.values()) < R.SEQ_FWD_BAR, seq
    if c.math == 4 and not c.f16:
        # incomplete tables: the exact kernels, bit for bit what mode 0 gives with the same plan
        exact = run_forward(gpe, c, p, W, family, math=0)
        for k in ('hs', 'sv', 'cs'):
            assert exact['flat'][k] is None or exact['flat'][k].tobytes() == out['flat'][k].tobytes(), k
    if family != R.DIAG:
        # the same case on the diagonals: element by element within the sum of the two families' per-cell bars (R.agree)
        diag = run_forward(gpe, c, p, W, R.DIAG, debug=c.debug | 1024 | 131072)
        wd = R.check_fwd(p, diag, f16=diag['f16'])
        assert wd.worst < 1.0, str(wd)
        both = R.agree(w, wd)
        print('RNNFIG %s %s against the diagonals: %s' % (group, R.case_id(c), both))
        assert both.worst < 1.0, str(both)
    return p, W, out


@_cases('persist_fwd')
def test_k_split_persistent_forward(gpe, case):
    _forward_case(gpe, 'persist_fwd', case, R.PERSIST)


@_cases('multi_fwd')
def test_multi_tile_persistent_forward(gpe, case):
    _forward_case(gpe, 'multi_fwd', case, R.MULTI)


@_cases('diag_fwd')
def test_diagonal_forward(gpe, case):
    _forward_case(gpe, 'diag_fwd', case, R.DIAG)


def _backward_case(gpe, group, c, family):
    p = R.make_problem(c)
    W = Weights(gpe, p, c.planes)
    hist_family = R.HISTORY_OF[group]
    if hist_family == R.PERSIST:            # the K-split forward takes several row tiles per workgroup under its own bit
        fdebug = c.debug | (2048 if c.debug & 4096 else 0)
    else:
        fdebug = c.debug | 1024 | 131072
    cf = R.dataclasses.replace(c, part_off=0)
    fwd = run_forward(gpe, cf, p, W, hist_family, debug=fdebug)
    out = run_backward(gpe, c, p, W, fwd, family)
    w = R.check_bwd(p, fwd, out, f16=out['f16'])
    want = R.ref_bwd(p, R.ref_fwd(p))
    seq = {k: R.whole_seq(out[k], want[k]) for k in (('dgx', 'carry0') if c.gates == 4 else ('dgx', 'dgh', 'carry0'))}
    _report(group, c, family, w, seq)
    assert w.worst < 1.0, str(w)
    assert max(seq.values()) < R.SEQ_BWD_BAR, seq
    if c.math == 4 and not out['f16']:
        # incomplete tables: the exact kernels, bit for bit what mode 0 gives with the same plan
        exact = run_backward(gpe, R.dataclasses.replace(c, math=0), p, W, fwd, family)
        for k in ('dgx', 'dgh', 'carry0'):
            assert exact[k].tobytes() == out[k].tobytes(), k
    if family != R.DIAG:
        # the same case, on the same history, on the diagonals: element by element within the sum of the two per-cell bars
        cd = R.dataclasses.replace(c, debug=c.debug | 1024)
        diag = run_backward(gpe, cd, p, W, fwd, R.DIAG)
        wd = R.check_bwd(p, fwd, diag, f16=diag['f16'])
        assert wd.worst < 1.0, str(wd)
        both = R.agree(w, wd)
        print('RNNFIG %s %s against the diagonals: %s' % (group, R.case_id(c), both))
        assert both.worst < 1.0, str(both)


@_cases('persist_bwd')
def test_k_split_persistent_backward(gpe, case):
    _backward_case(gpe, 'persist_bwd', case, R.PERSIST)


@_cases('diag_bwd')
def test_diagonal_backward(gpe, case):
    _backward_case(gpe, 'diag_bwd', case, R.DIAG)

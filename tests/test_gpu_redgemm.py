"""-m gpu: the reduce-GEMM kernels rung by rung through the C ABI (gpe_redgemm, gpe_edge_redgemm) against the fp64 references of
tests/redgemm_restate.py: cases, buffers, references, checkers and the derivation of their bars are there, and
tests/test_redgemm_host.py checks them on the CPU first (the restated plan is the library's, the lists reach every rung and kernel
instance, every bar accepts an fp32 restatement of its rung and every wrong reference is rejected on every rung).

Every case runs on integer data (EXACT: every summation order gives the fp64 reference bit for bit) and on random data (every
element of G and colsum on its own against its bar; nothing is filtered), each twice on freshly pre-filled outputs:
  - the two runs are bit-identical;
  - gpe_redgemm_path, asked with the device's own pointers, names the rung the case was written for, and its plan is the restated one;
  - the sentinels in G (pad columns, rows behind Mg), behind colsum and behind gpe_redgemm_ws floats of `part` come back untouched;
  - no NaN comes through: U, V and [P|Q] are NaN wherever a kernel must not read, `part` is NaN before the launch;
  - a case on an exact rung gives the same bits in every other math mode (0, 1, 4) whose plan is the same; the cases written in
    f16x3 mode that fall off the TN rung (under the FLOP gate, a misaligned V, debug bit 16384) must have mode 0's plan and bits.
The math mode, the debug word, the f16x3 gate and the CU reservation are restored in `finally`.

Worst figures observed on an MI355X are in profiles/redgemm_tests.md, in units of the bar."""
import ctypes

import numpy as np
import pytest
import torch

import redgemm_restate as R

pytestmark = pytest.mark.gpu

H3_WORD = 64 * 512                      # float index of the in-call f16x3 words in the edge workspace (csrc/gpe_common.h GPE_WS_DUMMY_BYTES / 4)


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _cases(group):
    return pytest.mark.parametrize('spec', R.CASES[group], ids=R.case_id)


def _raw(args):
    return [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]


def _word(x):
    """a device amax word: the bit pattern of the fp32 value x"""
    return torch.from_numpy(R.bits([x]).view(np.int32).copy()).cuda()


def _plan(L, case, dev):
    out = (ctypes.c_long * len(R.PLAN_FIELDS))()
    path = L.query('gpe_redgemm_path', *_raw(R.path_args(case, dev)), ctypes.addressof(out))
    return path, dict(zip(R.PLAN_FIELDS, out))


def _once(L, case, dev):
    """the call on freshly pre-filled outputs -> {name: host array}"""
    for n, a in case.out0.items():
        dev[n] = torch.from_numpy(a.copy()).cuda()
    L.call('gpe_redgemm' if case.spec.entry == 'redgemm' else 'gpe_edge_redgemm', *R.abi_args(case, dev))
    torch.cuda.synchronize()
    return {n: dev[n].cpu().numpy() for n in case.out0}


def _same(a, b):
    return all(a[n].tobytes() == b[n].tobytes() for n in ('G', 'colsum') if n in a)


def _run(gpe, spec, kind):
    L = gpe._lib
    case = R.build(spec, kind)
    s = spec
    dev = {n: torch.from_numpy(a).cuda() for n, a in case.inp.items()}
    saved = (L.query('gpe_math_get'), L.query('gpe_debug_get'), L.query('gpe_f16x3_min_rows'), L.get_reserved_cus())
    try:
        L.query('gpe_math_set', s.math)
        L.query('gpe_debug_set', s.debug)
        L.query('gpe_f16x3_min_rows_set', 0)
        L.query('gpe_reserve_cus_set', s.res)
        if s.words != 'none':
            dev['amax_u'] = _word(case.amax_u)
            if s.gather:
                nbytes = L.query('gpe_edge_ws_bytes', s.B, case.N, s.k, 512)
                dev['ws'], dev['ws_bytes'] = torch.zeros(nbytes // 4 + 4, dtype=torch.float32, device='cuda'), nbytes
            if s.words == 'both' and s.gather:                          # V's word: the library's own bound over the [P|Q] table
                dev['amax_v'] = torch.zeros(1, dtype=torch.int32, device='cuda')
                L.call('gpe_edge_pq_amax', dev['pq'], case.ldpq, s.Ng, case.npts, dev['amax_v'], dev['ws'], dev['ws_bytes'])
                bound = dev['amax_v'].cpu().numpy().view(np.float32)[0]
                assert 0 <= bound <= case.amax_v, 'the bar of rung 5 assumes a bound of at most %r, gpe_edge_pq_amax gave %r' % (case.amax_v, bound)
            elif s.words == 'both':
                dev['amax_v'] = _word(case.amax_v)
        path, pl = _plan(L, case, dev)
        assert path == s.rung, '%s: gpe_redgemm_path says rung %d, the case was written for %d' % (case.id, path, s.rung)
        assert (path, pl) == R.case_plan(case), case.id                 # (the restated plan of the 256-CU device the cases were written for)
        a, b = _once(L, case, dev), _once(L, case, dev)
        assert _same(a, b), '%s: two runs differ' % case.id
        worst = R.check(case, a, path=path, pl=pl)
        assert not np.isnan(a['G']).any() and ('colsum' not in a or not np.isnan(a['colsum']).any()), case.id
        if s.words == 'ws':                                             # the word the bound passes left in the workspace: the bar's A_v covers it
            bound = dev['ws'][H3_WORD:H3_WORD + 1].cpu().numpy().view(np.float32)[0]
            assert 0 <= bound <= case.amax_v, 'the bar of rung 5 assumes a bound of at most %r, the in-call passes gave %r' % (case.amax_v, bound)
        if path not in R.SPLIT_RUNGS and kind == 'rand':                # an exact rung: every mode with the same plan gives the same bits
            for mode in (0, 1, 4):
                L.query('gpe_math_set', mode)
                if mode != s.math and _plan(L, case, dev) == (path, pl):
                    assert _same(a, _once(L, case, dev)), '%s: math mode %d changed the bits of a call on exact rung %d' % (case.id, mode, path)
            if s.math == 4:                                             # fell off the TN rung in f16x3 mode: mode 0 must have been one of them
                L.query('gpe_math_set', 0)
                assert _plan(L, case, dev) == (path, pl), '%s: mode 0 takes another plan, its bits were not compared' % case.id
        if s.debug and kind == 'rand':                                  # the debug bit gave the exact rung: without it the bits differ
            L.query('gpe_math_set', s.math)
            L.query('gpe_debug_set', 0)
            p2, _ = _plan(L, case, dev)
            assert p2 == R.TN and not _same(a, _once(L, case, dev)), case.id
    finally:
        L.query('gpe_reserve_cus_set', saved[3])
        L.query('gpe_f16x3_min_rows_set', saved[2])
        L.query('gpe_debug_set', saved[1])
        L.query('gpe_math_set', saved[0])
    print('redgemm[%s] rung %d, n_p %d, worst in bars: %s' % (case.id, path, R.chain_rows(path, pl, s.rows, s.B),
                                                             ', '.join('%s %.4f' % kv for kv in sorted(worst.items()))))


def _both(gpe, spec):
    _run(gpe, spec, 'int')
    _run(gpe, spec, 'rand')


@_cases('thin')
def test_redgemm_thin(gpe, spec):
    """rung 1 (gpe_redgemm_thin_kernel<1, 2, 4>): ql 1 .. 4, a ragged row split, 512 partials, workgroups without a row, with and
    without the shift and the column sums (partial column sums only when wanted); the neighbours on the deep and big-block kernels."""
    _both(gpe, spec)


@_cases('tn')
def test_redgemm_bf16_pipe_tn(gpe, spec):
    """rung 2 (gpe_gemm_x6_tn_kernel, f16x3 mode): S = 1 at the FLOP gate, two-level rows, a short last piece with the shift, an edge
    shape without words; just under the gate, a 4-byte-misaligned V and debug bit 16384 go down the ladder to the exact deep kernel."""
    _both(gpe, spec)


@_cases('deep')
def test_redgemm_deep(gpe, spec):
    """rung 3 (gpe_redgemm_deep_kernel<vvec>): one element, one block, a 2 x 2 block grid, ragged blocks, two-level rows with a spare
    slot, the scalar V loader, gx 32 at 256 CUs, one tile short of the producer/consumer switch."""
    _both(gpe, spec)


@_cases('pc')
def test_redgemm_producer_consumer(gpe, spec):
    """rung 7 (gpe_redgemm_pc_kernel<MT, 13, vmode>): MT 10 and 13, dense through both entry points and gathered with k 15 and 16,
    a partial last tile, ragged last column tiles, nothing reserved, clouds pinned to XCDs."""
    _both(gpe, spec)


@_cases('b3bf16')
def test_redgemm_b3_bf16x3(gpe, spec):
    """rung 6 (gpe_redgemm_b3_kernel<MT, 13, vmode>): the producer/consumer cases in math mode 1."""
    _both(gpe, spec)


@_cases('b3f16')
def test_redgemm_b3_f16x3(gpe, spec):
    """rung 5 (gpe_redgemm_b3_kernel<MT, 13, vmode, F16>): the same in math mode 4 with both words; a gathered V's word once from
    gpe_edge_pq_amax and once NULL with a workspace."""
    _both(gpe, spec)


@_cases('big')
def test_redgemm_big_block(gpe, spec):
    """rung 8 (gpe_redgemm_kernel<MH, NH, vmode>): the twelve (MH, NH) instances with the 16-byte and the scalar-tail loader, gathered
    ones, gy 1 -> 5, rows = 0 (zeros, or the old values under accumulate)."""
    _both(gpe, spec)

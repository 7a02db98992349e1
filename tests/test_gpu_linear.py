"""-m gpu: the dense Linear kernels rung by rung through the C ABI (gpe_linear, gpe_linear_splitk, gpe_pack_weight) against the fp64
references of tests/linear_restate.py: cases, references, checkers and the derivation of their bars are there, and
tests/test_linear_host.py checks them on the CPU first (every bar accepts an fp32 restatement of its rung, every wrong reference is
rejected on every rung, and the library's own gpe_linear_path puts every case on the rung it was written for).

Every output element is compared on its own, in units of u = 2^-24 times sum_k |a_k w_k| + |bias| + |addend|; no case is filtered.
Pitches are padded; A, the addend and the source weight hold NaN wherever the kernel must not read (behind column K too: the
bf16-pipe kernel loads the last quad whole); the packed weight is NaN before gpe_pack_weight fills it; all of y outside the valid
elements holds a sentinel and must come back untouched (pad columns, rows >= M, the unused slot of two-level rows).

Every Linear case runs in BOTH arithmetic modes, each run twice (bit-identical: no atomics):
  math mode 0   gpe_linear_path answers the case's exact rung, the result meets the exact bar gamma(K + 2)
  math mode 4   where gpe_linear_path does not answer 100, the bits are those of mode 0; where it does, the result meets the
                bf16-pipe bar gamma(6 K + 3) (1 + 2^-6), the run under gpe_debug_set(16384) answers the exact rung again with mode 0's
                bits, and the two differ: the bf16 pipe really ran.
The debug word and the math mode are restored in `finally`.

Worst figures observed on an MI355X are in each test's docstring, in units of the bar."""
import pytest
import torch

import linear_restate as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _cases(group):
    return pytest.mark.parametrize('spec', R.CASES[group], ids=R.case_id)


def _device(case):
    return {n: torch.from_numpy(a.copy()).cuda() for n, a in {**case.inp, **case.out0}.items()}


def _raw(args):
    return [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]


def _twice(gpe, case, dev, out):
    """the call, twice on freshly pre-filled outputs: bit-identical -> the output `out` as a host array"""
    got = []
    for _ in range(2):
        dev[out].copy_(torch.from_numpy(case.out0[out]))
        gpe._lib.call(case.kernel, *R.abi_args(case, dev))
        torch.cuda.synchronize()
        got.append(dev[out].cpu().numpy())
    assert got[0].tobytes() == got[1].tobytes(), '%s[%s]: two runs differ' % (case.kernel, case.id)
    return got[0]


def _linear_run(gpe, case, dev):
    """-> the rung gpe_linear_path names for the call on the device's own pointers, and y"""
    path = gpe._lib.query('gpe_linear_path', *_raw(R.abi_args(case, dev)))
    return path, _twice(gpe, case, dev, 'y')


def _linear(gpe, group, spec):
    L = gpe._lib
    case = R.build(group, spec)
    dev = _device(case)
    L.call('gpe_pack_weight', *R.pack_args(case, dev))
    math, dbg = L.query('gpe_math_get'), L.query('gpe_debug_get')
    try:
        L.query('gpe_debug_set', 0)
        L.query('gpe_math_set', 0)
        p0, y0 = _linear_run(gpe, case, dev)
        assert p0 == spec.path != R.X6, (p0, spec.path)
        worst = {'exact %d' % p0: R.check(case, {'y': y0}, x6=False, path=p0)['y']}
        L.query('gpe_math_set', 4)
        p4, y4 = _linear_run(gpe, case, dev)
        assert p4 == spec.path4, (p4, spec.path4)
        if p4 != R.X6:
            assert y4.tobytes() == y0.tobytes(), 'f16x3 mode changed the bits of a call that is not on the bf16 pipe'
        else:
            worst['bf16 pipe'] = R.check(case, {'y': y4}, x6=True, path=p4)['y']
            L.query('gpe_debug_set', 16384)
            pd, yd = _linear_run(gpe, case, dev)
            assert pd == p0 and yd.tobytes() == y0.tobytes(), 'debug bit 16384 must give the exact rung and its bits'
            assert yd.tobytes() != y4.tobytes(), 'the bf16 pipe gave the bits of the exact kernel: did it run?'
    finally:
        L.query('gpe_debug_set', dbg)
        L.query('gpe_math_set', math)
    print('gpe_linear[%s/%s] worst, in bars: %s' % (group, case.id, ', '.join('%s %.4f' % kv for kv in sorted(worst.items()))))
    assert group != 'x6' or 'bf16 pipe' in worst


@_cases('x6')
def test_linear_bf16_pipe(gpe, spec):
    """rung 100 (gpe_gemm_x6_nt_kernel), 128 x 128 blocks in 32-wide K steps: the menu's smallest shapes (M 2048, N 48, K 32, the FLOP
    gate), ragged M / N / K with scalar stores, a scalar addend and NaN inside the last loaded quad, all eight epilogues, two-level
    rows, A scaled by 1e-25 and 1e20 at the same bar, and the operands whose third split term is as large as it gets.  In mode 0 the
    same cases run on rungs 301, 304 and 416 at the exact bar.
    MI355X: worst 0.011 bars on the bf16 pipe (16384 x 256 x 32; 0.010 on the low-bits operands, where a two-term split would
    stand at 1.26; 0.005 and 0.004 at the scales 1e-25 and 1e20), 0.19 on the exact rungs."""
    _linear(gpe, 'x6', spec)


@_cases('smallk')
def test_linear_small_k(gpe, spec):
    """rung 200 (gpe_linear_smallk_kernel): K 1 / 3 / 8, N from one quad to two column blocks (252, 256, 260), 131 077 rows on the
    4096-block grid (the stride loop), all eight epilogues, two-level rows.  MI355X: worst 0.53 bars (4096 x 256 x 3)."""
    _linear(gpe, 'smallk', spec)


@_cases('single1')
def test_linear_single_stage_16(gpe, spec):
    """rung 301 (gpe_smallgemm_kernel<1>): M 1 / 63 / 64 / 65, N 1 .. 250, K around the quad, the 16-wide chunk and the 256-wide slab up
    to 520, the vector staging path (K % 4 == 0, aligned rows) beside the guarded one (misaligned base or pitch), all eight epilogues,
    two-level rows, and everything that falls off the K <= 8 and bf16-pipe rungs onto this one.
    MI355X: worst 0.47 bars (4096 x 4 x 3 with a misaligned addend)."""
    _linear(gpe, 'single1', spec)


@_cases('single4')
def test_linear_single_stage_64(gpe, spec):
    """rung 304 (gpe_smallgemm_kernel<4>): 32 tiles with a one-row last tile, N 193 / 250 / 256, K around the slab, 128 block columns
    exactly, all eight epilogues, two-level rows, the bf16-pipe menu's near misses.
    MI355X: worst 0.59 bars (4096 x 150 x 3)."""
    _linear(gpe, 'single4', spec)


@_cases('stream')
def test_linear_streaming(gpe, spec):
    """rungs 404 .. 416 (gpe_rowgemm_kernel<NT, A_DENSE, E_LINEAR>): every NT at both ends of its N class on 256 tiles with a one-row
    last tile, the first streaming shapes at 128 tiles, N = 400 as four 112-wide and as two 208-wide blocks, N = 1000, K 255 .. 520
    on a narrow and a wide instance (in f16x3 mode those eight run on the bf16 pipe and are held against its bar too), all eight
    epilogues, two-level rows.
    MI355X: worst 0.61 bars on NT 4 (4096 x 252 x 3), 0.33 / 0.40 / 0.39 / 0.36 on NT 7 / 10 / 13 / 16; 0.003 on the bf16 pipe."""
    _linear(gpe, 'stream', spec)


@_cases('splitk')
def test_linear_splitk(gpe, spec):
    """gpe_linear_splitk (gpe_smallgemm_kernel<4> with gridDim.z K slabs): every partial y[z] against its own slab's fp64 product
    within gamma(slab width) of the slab's magnitude sum; the floats behind the last partial untouched; twice, bit-identical.
    MI355X: worst 0.99 bars (64 x 64 x 257: the second slab is one product, its bar one rounding), 0.02 on whole slabs."""
    case = R.build('splitk', spec)
    dev = _device(case)
    gpe._lib.call('gpe_pack_weight', *R.pack_args(case, dev))
    worst = R.check(case, {'y': _twice(gpe, case, dev, 'y')})
    print('gpe_linear_splitk[%s] worst, in bars: %.4f' % (case.id, worst['y']))


@pytest.mark.parametrize('N,transpose,ldpad,cs', [(N, t, ld, cs) for N in (1, 16, 17) for t in (0, 1) for ld in (0, 1) for cs in (0, 1)])
def test_pack_weight(gpe, N, transpose, ldpad, cs):
    """gpe_pack_weight into a NaN-filled buffer, K 1 .. 209 (the 160 / 208 fill-up from both sides): the whole gpe_packed_size image bit
    for bit — the zeros of k in [K, kpad) and n in [N, Npad) included — and the floats behind it untouched.  MI355X: exact."""
    specs = [s for s in R.CASES['pack'] if (s.N, s.transpose, s.ldpad, s.cs) == (N, transpose, ldpad, cs)]
    assert len(specs) == 11
    for spec in specs:
        case = R.build('pack', spec)
        R.check(case, {'wp': _twice(gpe, case, _device(case), 'wp')})


@pytest.mark.parametrize('group', R.LINEAR_GROUPS)
def test_linear_empty_and_refused(gpe, group):
    """on one case of every rung: M = 0 returns 0 and act = 2 returns -22, in both modes, and neither writes anything"""
    L = gpe._lib
    case = R.build(group, R.CASES[group][-1] if group != 'x6' else R.CASES[group][0])
    dev = _device(case)
    L.call('gpe_pack_weight', *R.pack_args(case, dev))
    math = L.query('gpe_math_get')
    try:
        for mode in (0, 4):
            L.query('gpe_math_set', mode)
            for pos, bad, want in ((14, 0, 0), (17, 2, -22)):
                args = _raw(R.abi_args(case, dev))
                args[pos] = bad
                assert L.query('gpe_linear_path', *args) == want
                assert L.query('gpe_linear', *args, torch.cuda.current_stream().cuda_stream) == want
                torch.cuda.synchronize()
                assert dev['y'].cpu().numpy().tobytes() == case.out0['y'].tobytes()
    finally:
        L.query('gpe_math_set', math)

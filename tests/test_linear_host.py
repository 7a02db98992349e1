"""CPU: the restated dense Linear kernels of tests/linear_restate.py are checked before any GPU time is spent on them.

a) the reference is the right operation: it equals torch's fp64 addmm (+ ReLU) on three cases, and its packed image follows the
   library's own gpe_packed_size;
b) every bar passes its own reference: each checker accepts `emulate`, an fp32 restatement of the rung in one plausible order (with
   the three-term bf16 split on the bf16-pipe rung), on every case of the GPU test;
c) every bar discriminates: each `variant` (a reference that is wrong in one plausible way) is rejected by at least one case;
d) the case lists cover the ladder: gpe_linear_path (host only, include/gpe_hip.h) is asked for every case, with host memory standing
   in for the device pointers, and answers the code the case was written for; every rung, every NT instance and both sides of
   every edge have a case; in math mode 0 nothing answers the bf16-pipe rung;
e) gpe_linear_path refuses what gpe_linear refuses."""
import ctypes

import numpy as np
import pytest
import torch

import linear_restate as R
from gpe_amd import _lib


# ----------------------------------------------------------------------------------------------------------------------
# a) the restated reference against torch
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('group,spec', [('single1', R.L(65, 35, 20, R.SINGLE1, bias=1, addend=1, act=1, ad='two')),
                                        ('stream', R.L(8129, 70, 12, R.STREAM[4], bias=1, addend=1, act=1, a='two')),
                                        ('x6', R.L(2050, 130, 470, R.SINGLE1, R.X6, addend=1, act=1))], ids=R.case_id)
def test_reference_is_torch_addmm(group, spec):
    """y = act(addmm(bias + addend, A, W^T)) in fp64 from the rows the buffers hold: 1e-13 of the element's magnitude sum"""
    case = R.build(group, spec)
    A, W, b, ad = (None if t is None else torch.from_numpy(np.asarray(t, np.float64)) for t in R._lin_operands(case))
    want = torch.addmm(b + ad, A, W.t())
    if spec.act:
        want = torch.relu(want)
    ref, mag = R._ref_linear(case)
    assert np.isfinite(ref).all() and (mag > 0).all()
    assert (np.abs(ref - want.numpy()) <= 1e-13 * mag).all()


def test_packed_size_is_the_librarys():
    l = _lib.lib()
    for N in (1, 16, 17, 200, 1000):
        for K in list(range(1, 260)) + [520, 1000]:
            assert l.gpe_packed_size(N, K) == R.packed_size(N, K), (N, K)
    # the layout rule on a hand-sized example: N = 2, K = 5 -> Npad 16, kpad 16; element (n, k) at ((k / 4) * 16 + n) * 4 + k % 4
    w = np.arange(10, dtype=np.float32).reshape(2, 5) + 1
    img = R.ref_packed(w, 2, 5)
    assert img.size == 256 and img[(1 * 16 + 1) * 4 + 0] == w[1, 4] and img[(0 * 16 + 0) * 4 + 3] == w[0, 3]
    assert np.count_nonzero(img) == 10
    assert (R.ref_packed(np.ascontiguousarray(w.T), 2, 5, transpose=1) == img).all()


# ----------------------------------------------------------------------------------------------------------------------
# b) every bar passes its own reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('group,spec', R.case_params(), ids=R.case_id)
def test_bar_accepts_its_reference(group, spec):
    case = R.build(group, spec)
    before = {n: a.copy() for n, a in {**case.inp, **case.out0}.items()}
    worst = R.check(case, R.emulate(case))
    assert all(v <= 1.0 for v in worst.values())
    if group != 'x6' and group in R.LINEAR_GROUPS and spec.path4 == R.X6:
        R.check(case, R.emulate(case, x6=True), x6=True)             # a case of another group that f16x3 mode moves to the bf16 pipe
    for n, a in {**case.inp, **case.out0}.items():                   # the shared case is left unchanged
        assert a.tobytes() == before[n].tobytes(), n


# ----------------------------------------------------------------------------------------------------------------------
# c) every bar discriminates
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', sorted(R.VARIANTS))
def test_every_variant_is_rejected(kernel):
    """... and, for the Linear, by at least one case of EVERY rung that has a case the variant changes (the first is enough)"""
    groups = [g for g in R.GROUPS if R.KERNEL_OF.get(g, 'linear') == kernel]
    for variant in R.VARIANTS[kernel]:
        for g in groups:
            rejecting, tried = None, 0
            for spec in R.CASES[g]:
                case = R.build(g, spec)
                if rejecting or not R.variant_applies(case, variant):
                    continue
                tried += 1
                try:
                    R.check(case, R.emulate(case), variant=variant)
                except AssertionError:
                    rejecting = case.id
            print('%s / %s / %s: %s' % (kernel, variant, g, 'rejected by %s (case %d of those it changes)' % (rejecting, tried) if rejecting
                                        else 'changes no case' if not tried else 'NOT REJECTED'))
            assert rejecting or not tried, 'no case of %s tells the variant %r from the kernel: the case list is missing an input' % (g, variant)
            # every rung has a case for every variant, but: the K <= 8 rung has neither a second K slab nor a ragged column quad
            assert tried or variant == 'x6_two_term' or (g, variant) in (('smallk', 'drop_slab2'), ('smallk', 'last_quad_shift')), (g, variant)


def test_two_term_split_needs_the_crafted_case():
    """the module's note: on random operands a two-term split stays inside the bf16-pipe bar; the low-bits case rejects it"""
    rnd = R.build('x6', R.L(16384, 256, 32, R.STREAM[16], R.X6))
    low = R.build('x6', R.L(16384, 256, 32, R.STREAM[16], R.X6, bias=0, kind='lowbits'))
    R.check(rnd, R.emulate(rnd), variant='x6_two_term')
    with pytest.raises(AssertionError, match='bars'):
        R.check(low, R.emulate(low), variant='x6_two_term')


# ----------------------------------------------------------------------------------------------------------------------
# d) the case lists cover the ladder, by the library's own answer
# ----------------------------------------------------------------------------------------------------------------------
class _StandIn:
    """host memory stands in for a device buffer: gpe_linear_path looks at a pointer's value, never behind it"""

    def __init__(self):
        self.buf = (ctypes.c_double * 16)()
        self.base = (ctypes.addressof(self.buf) + 63) // 64 * 64

    def __getitem__(self, sl):
        return self.base + 4 * (sl.start or 0)


def _path_args(case):
    d = {n: _StandIn() for n in ('a', 'wp', 'y')}
    d.update({n: _StandIn() for n in ('bias', 'addend') if n in case.inp})
    return [a[0:] if isinstance(a, _StandIn) else a for a in R.abi_args(case, d)]


def _paths(case):
    l = _lib.lib()
    args = _path_args(case)
    out = []
    for mode in (0, 4):
        l.gpe_math_set(mode)
        out.append(l.gpe_linear_path(*args))
    return tuple(out)


@pytest.fixture
def clean_state():
    l = _lib.lib()
    math, dbg = l.gpe_math_get(), l.gpe_debug_get()
    l.gpe_debug_set(0)
    yield l
    l.gpe_debug_set(dbg)
    l.gpe_math_set(math)


def test_case_lists_cover_the_issue(clean_state):
    seen0, seen4 = set(), set()
    for g in R.LINEAR_GROUPS:
        for spec in R.CASES[g]:
            p0, p4 = _paths(R.build(g, spec))
            assert (p0, p4) == (spec.path, spec.path4), (g, R.case_id(spec), p0, p4)
            assert p0 != R.X6                                       # exact mode never answers the bf16 pipe
            want = {'single1': {R.SINGLE1}, 'single4': {R.SINGLE4}, 'smallk': {R.SMALLK}, 'stream': set(R.STREAM.values())}
            assert p4 == R.X6 if g == 'x6' else p0 in want[g], (g, R.case_id(spec))   # a case stands in the group of its rung
            seen0.add(p0)
            seen4.add(p4)
    assert seen0 == set(R.ALL_CODES) - {R.X6} and R.X6 in seen4      # every rung and every NT instance
    flat = {s for g in R.LINEAR_GROUPS for s in R.CASES[g]}
    for name, (lo, hi) in R.EDGES.items():                           # both sides of every edge are cases
        assert lo in flat and hi in flat, name
        assert (lo.path, lo.path4) != (hi.path, hi.path4) or 'K slab' in name or 'N 16/17' in name or 'grid' in name, name
    # the debug bit keeps the exact kernels in f16x3 mode
    case = R.build('x6', R.L(16384, 256, 32, R.STREAM[16], R.X6))
    clean_state.gpe_math_set(4)
    clean_state.gpe_debug_set(16384)
    assert clean_state.gpe_linear_path(*_path_args(case)) == R.STREAM[16]
    # the epilogue cases: all eight combinations and the three two-level operands on every rung
    for g in R.LINEAR_GROUPS:
        combos = {(s.bias, s.addend, s.act) for s in R.CASES[g]}
        assert len(combos) == 8, g
        assert {'two'} <= {s.a for s in R.CASES[g]} and {'two'} <= {s.ad for s in R.CASES[g]} and {'two'} <= {s.y for s in R.CASES[g]}, g
    # split-K and the packer
    assert {s.M for s in R.CASES['splitk']} >= {1, 64, 65} and {s.N for s in R.CASES['splitk']} >= {63, 64, 65}
    assert {s.K for s in R.CASES['splitk']} >= {256, 257, 1000} and {s.a for s in R.CASES['splitk']} >= {'plain', 'pitch1'}
    assert len(R.CASES['pack']) == 3 * 11 * 8


# ----------------------------------------------------------------------------------------------------------------------
# e) the path query refuses what the entry point refuses
# ----------------------------------------------------------------------------------------------------------------------
def test_path_agrees_with_gpe_linear_on_refused_arguments(clean_state):
    """position in the argument list of include/gpe_hip.h, bad value: both answer -22 before anything is launched; M = 0 is 0 for both"""
    l = clean_state
    case = R.build('single1', R.L(65, 35, 20, R.SINGLE1, bias=1, addend=1, act=1))
    good = _path_args(case)
    assert l.gpe_linear_path(*good) == R.SINGLE1
    for pos, bad in ((0, None), (4, None), (10, None), (14, -1), (15, 0), (15, -3), (16, 0), (16, -1), (17, 2), (17, -1)):
        args = list(good)
        args[pos] = bad
        assert l.gpe_linear_path(*args) == -22, (pos, bad)
        assert l.gpe_linear(*args, None) == -22, (pos, bad)
    args = list(good)
    args[14] = 0
    assert l.gpe_linear_path(*args) == 0 and l.gpe_linear(*args, None) == 0
    # bias and addend may be NULL
    args = list(good)
    args[5] = args[6] = None
    assert l.gpe_linear_path(*args) == R.SINGLE1

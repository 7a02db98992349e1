"""-m gpu: the EdgeConv glue kernels between the fused edge GEMMs, one by one through the C ABI against the fp64 references of
tests/edge_glue_restate.py (cases, references, checkers and their bars are there; tests/test_edge_glue_host.py checks them on the
CPU first).  Every comparison is element by element, in units of u = 2^-24 times a magnitude taken from the reference; the four
kernels whose fp32 order of operations is fixed are compared bit for bit.  No case is filtered.

Pitches are padded, pad columns the kernel must not read hold NaN, everything it must not write holds a sentinel, and an amax
word holds a large pattern that only the call's own reset removes.  The shapes are the smallest that reach each branch:

  gpe_edge_gather_stats    B 1 / 7 | 8 / 9, 16 (unpinned | pinned even / uneven clouds per XCD), k around the 8 rows in flight up to 64,
                           H from one quad to all 64 lanes, self loops, duplicate neighbours, a hub, one channel negative everywhere
  gpe_bn_finalize          nblk around the 64 row slots and their 4 chains (1 .. 513), C around the 16 channels of a workgroup, a constant
                           channel whose variance is negative before the clamp, count = 1, gamma +, -, 0, -0.0, running buffers or NULL
  gpe_bn_from_running      C around the 64 threads of a workgroup
  gpe_edge_finish, gpe_bn_apply     rows 0, 1, 255 .. 257, C 1 / 150 / 257, all four scale signs, mx != mn
  gpe_edge_sum_k           F around the 64 lanes, k 1 / 5 / 16, 8200 points for the grid-stride loop
  gpe_edge_bwd_point_sums  rows around the 512 blocks and their 8 rows in flight, C around 256, with and without the word
  gpe_bn_bwd_coef          nblk around the 16 waves, C around 64, dgamma / dbeta given or NULL
  gpe_edge_dz3, _all       F around the quad and the 256 columns of a workgroup, k around the 8 rows in flight, every selector slot,
                           exact zeros, -0.0 and negatives in a3, a dead channel, gscale 1 and 1 / k, 16390 points for the stride loop
  gpe_edge_dz3_bound       F around the 256 threads
  gpe_bn_bwd_from_G        Cn around the 16 f-lanes and their two chains, C around 64, dw given or NULL
  gpe_knn_reverse          N around the 1024 threads; (1, 2048, 20) and (1, 1025, 40) sort in global memory, the others in LDS (the
                           launcher's 150 KB rule, asserted below); a hub of in-degree 4000 beside isolated points
  gpe_edge_pull_dq         in-degrees 0, 1, 3, 4, 5 and 300, output into the right half of a [BN][2H] buffer
  gpe_edge_inputs_fwd/bwd  C 1 / 3 / 5, k 1 / 4 / 9, the whole output pad written 0

Worst figures observed on an MI355X are in each test's docstring, in units of the bar."""
import pytest
import torch

import edge_glue_restate as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _ids(v):
    return v if isinstance(v, str) else '-'.join(str(int(a)) for a in v)


def _device(case):
    return {n: torch.from_numpy(a.copy()).cuda() for n, a in {**case.inp, **case.out0}.items()}


def _run(gpe, case):
    dev = _device(case)
    gpe._lib.call(case.kernel, *R.abi_args(case, dev))
    torch.cuda.synchronize()
    return {n: dev[n].cpu().numpy() for n in case.out0}


def _cases(kernel):
    return pytest.mark.parametrize('args', R.CASES[kernel], ids=_ids)


def _check(gpe, kernel, args):
    case = R.build(kernel, args)
    worst = R.check(case, _run(gpe, case))
    print('%s[%s] worst, in bars: %s' % (case.kernel, case.id, ', '.join('%s %.3f' % kv for kv in sorted(worst.items())) or 'exact'))


@_cases('edge_gather_stats')
def test_edge_gather_stats(gpe, args):
    """sum and sum of squares per channel within (k + 2) u relative, after the fp64 sum of the 512 partial blocks; exactly 0 in the
    channel that is negative on every edge.  MI355X: worst 0.05 bars (sum), 0.14 (sum of squares)."""
    _check(gpe, 'edge_gather_stats', args)


@_cases('bn_finalize')
def test_bn_finalize(gpe, args):
    """mean, rstd, s within 2u, t within 2u (|beta| + |mean s|), running statistics within 2u (|old| + |new|), the counter + 1.
    MI355X: worst 0.46 bars (mean, rstd), 0.48 (s), 0.85 (t), 0.50 (running)."""
    _check(gpe, 'bn_finalize', args)


@_cases('bn_from_running')
def test_bn_from_running(gpe, args):
    """MI355X: worst 0.47 bars (rstd), 0.48 (s), 0.68 (t); the mean row is a copy."""
    _check(gpe, 'bn_from_running', args)


@_cases('edge_finish')
def test_edge_finish(gpe, args):
    """y = s (s >= 0 ? mx : mn) + t within 2u (|s v| + |t|); under a zero scale (+0 and -0.0 both select mx) the result is t = -0.0
    plus a zero whose sign is the selected operand's, compared bit for bit.  MI355X: worst 0.50 bars."""
    _check(gpe, 'edge_finish', args)


@_cases('bn_apply')
def test_bn_apply(gpe, args):
    """y = s a + t within 2u (|s a| + |t|).  MI355X: worst 0.88 bars."""
    _check(gpe, 'bn_apply', args)


@_cases('edge_sum_k')
def test_edge_sum_k(gpe, args):
    """bit-exact against the fp32 sum over the slots in ascending order from +0.  MI355X: exact; against fp64, 0.50 of k u sum|terms|."""
    _check(gpe, 'edge_sum_k', args)


@_cases('edge_inputs_fwd')
def test_edge_inputs_fwd(gpe, args):
    """[x_i | x_j - x_i] bit-exact (one fp32 subtraction); every pad column up to the pitch written 0.  MI355X: exact."""
    _check(gpe, 'edge_inputs_fwd', args)


@_cases('edge_inputs_bwd')
def test_edge_inputs_bwd(gpe, args):
    """bit-exact against: sum over the slots of (g1 - g2), ascending, then the pulled g2 in ascending edge id (graph built on the CPU).
    MI355X: exact; against fp64, 0.89 of (k + in-degree) u sum|terms|."""
    _check(gpe, 'edge_inputs_bwd', args)


@_cases('edge_bwd_point_sums')
def test_edge_bwd_point_sums(gpe, args):
    """sum g within 1e-13 sum|g|, sum g xhat within 4u sum|g xhat|, the amax_sg word reset by the call and in [true, true (1 + 8u)].
    MI355X: worst below 0.001 bars (sum g), 0.41 (sum g xhat), the word 0.62 of its 8u above the true maximum."""
    _check(gpe, 'edge_bwd_point_sums', args)


@_cases('bn_bwd_coef')
def test_bn_bwd_coef(gpe, args):
    """coef = {s, c1, k2, mean}, dgamma, dbeta within 2u.  MI355X: worst 0.49 bars."""
    _check(gpe, 'bn_bwd_coef', args)


@_cases('edge_dz3')
def test_edge_dz3(gpe, args):
    """exactly 0 where a3 <= 0, else within 8u (|s g| + |c1| + |(a - mean) k2|); columns F .. round_up(F, 4) written 0, the rest of
    the pitch untouched; the word reset and equal to the bits of the largest |value| written.  MI355X: worst 0.28 bars."""
    _check(gpe, 'edge_dz3', args)


@_cases('edge_dz3_all')
def test_edge_dz3_all(gpe, args):
    """as gpe_edge_dz3 with every slot carrying gscale g.  MI355X: worst 0.31 bars."""
    _check(gpe, 'edge_dz3_all', args)


@_cases('edge_dz3_bound')
def test_edge_dz3_bound(gpe, args):
    """within 4u of (amax_sg + max_c (|c1| + (1.001 amax_a3 + |mean|) |k2|)) 1.000001 in fp64, sign bit clear, not below max |dz3|
    of the eager reference.  MI355X: worst 0.32 bars."""
    _check(gpe, 'edge_dz3_bound', args)


@_cases('bn_bwd_from_G')
def test_bn_bwd_from_G(gpe, args):
    """the fp64 sums within 1e-13 of their magnitude sums, dW within 2u.  MI355X: worst 0.004 bars (sums), 0.50 (dW)."""
    _check(gpe, 'bn_bwd_from_G', args)


# which sort each gpe_knn_reverse case takes: counters and offsets (2 N + 1 ints) + the N k edge ids within 150 KB -> in LDS
KNN_REVERSE_LDS = {(1, 1, 1): True, (3, 2, 1): True, (2, 1023, 3): True, (2, 1024, 3): True, (2, 1025, 3): True, (1, 2048, 16): True,
                   (1, 2048, 20): False, (1, 1025, 40): False, (2, 1024, 5): True}


@_cases('knn_reverse')
def test_knn_reverse_cases(gpe, args):
    """integers, exact: rev_off the exclusive scan of the in-degrees with rev_off[N] = N k, every bucket the cloud-local edge ids in
    ascending order (a stable argsort of the targets).  MI355X: exact, both sorts."""
    B, N, k, _ = args
    assert R.knn_reverse_uses_lds(N, k) == KNN_REVERSE_LDS[(B, N, k)]
    _check(gpe, 'knn_reverse', args)


@_cases('edge_pull_dq')
def test_edge_pull_dq(gpe, args):
    """bit-exact against the fp32 sum of the incoming edges in ascending edge id from +0; the left half of the buffer untouched.
    MI355X: exact; against fp64, 0.61 of in-degree u sum|terms|."""
    _check(gpe, 'edge_pull_dq', args)


# ----------------------------------------------------------------------------------------------------------------------
# argument checks: one call per -22 condition a launcher states; the code comes back and nothing is written
# ----------------------------------------------------------------------------------------------------------------------
# (kernel, case, position in the argument list of include/gpe_hip.h, bad value)
EINVAL = [
    ('edge_gather_stats', (1, 33, 1, 4), 2, 6),          # H % 4
    ('edge_gather_stats', (1, 33, 1, 4), 2, 260),        # H > 256
    ('edge_gather_stats', (1, 33, 1, 4), 1, 4),          # ldpq < 2 H
    ('edge_gather_stats', (1, 33, 1, 4), 1, 13),         # ldpq % 4
    ('edge_gather_stats', (1, 33, 1, 4), 6, 65),         # k > 64
    ('edge_gather_stats', (1, 33, 1, 4), 6, 0),          # k <= 0
    ('edge_gather_stats', (1, 33, 1, 4), 3, None),       # jg NULL
    ('bn_finalize', (63, 1, 1000.0, True), 1, 0),        # nblk <= 0
    ('bn_finalize', (63, 1, 1000.0, True), 3, 0.0),      # count <= 0
    ('bn_finalize', (63, 1, 1000.0, True), 4, None),     # gamma NULL
    ('bn_from_running', (1,), 2, 0),                     # C <= 0
    ('bn_from_running', (1,), 1, None),                  # running_var NULL
    ('edge_finish', (255, 1), 2, 0),                     # ldagg < C
    ('edge_finish', (255, 1), 7, 0),                     # ldy < C
    ('edge_finish', (255, 1), 4, -1),                    # rows < 0
    ('bn_apply', (255, 1), 1, 0),                        # lda < C
    ('bn_apply', (255, 1), 6, 0),                        # ldy < C
    ('edge_sum_k', (5, 5, 63), 1, 62),                   # lda < F
    ('edge_sum_k', (5, 5, 63), 6, 62),                   # ldo < F
    ('edge_sum_k', (5, 5, 63), 2, 0),                    # npts <= 0
    ('edge_sum_k', (5, 5, 63), 3, 0),                    # k <= 0
    ('edge_inputs_fwd', (7, 20, 4, 3), 1, 2),            # ldx < C
    ('edge_inputs_fwd', (7, 20, 4, 3), 7, 5),            # ldo < 2 C
    ('edge_inputs_bwd', (7, 20, 4, 3), 1, 5),            # ldg < 2 C
    ('edge_inputs_bwd', (7, 20, 4, 3), 9, 2),            # ldgx < C
    ('edge_inputs_bwd', (7, 20, 4, 3), 3, None),         # rev_off NULL
    ('edge_bwd_point_sums', (511, 1, False), 6, 0),      # rows <= 0
    ('edge_bwd_point_sums', (511, 1, False), 5, None),   # stats NULL
    ('bn_bwd_coef', (15, 1, False), 1, 0),               # nblk <= 0
    ('bn_bwd_coef', (15, 1, False), 4, 0.0),             # count <= 0
    ('edge_dz3', (1, 4, 8, 4, True), 4, None),           # amx NULL
    ('edge_dz3', (1, 4, 8, 4, True), 5, None),           # amn NULL
    ('edge_dz3', (1, 4, 8, 4, True), 1, 6),              # lda3 % 4
    ('edge_dz3', (1, 5, 9, 5, False), 1, 4),             # lda3 < F
    ('edge_dz3', (1, 4, 8, 4, True), 6, 6),              # ldagg % 4
    ('edge_dz3', (1, 5, 9, 5, False), 6, 4),             # ldagg < F
    ('edge_dz3', (1, 4, 8, 4, True), 10, 0),             # k <= 0
    ('edge_dz3_all', (1, 4, 8, 4, False, True), 1, 6),   # lda3 % 4
    ('edge_dz3_all', (1, 5, 9, 5, True, False), 1, 4),   # lda3 < F
    ('edge_dz3_bound', (1,), 2, 0),                      # F <= 0
    ('edge_dz3_bound', (1,), 3, None),                   # amax_a3 NULL
    ('bn_bwd_from_G', (17, 64, True), 1, 63),            # ldG < C
    ('bn_bwd_from_G', (17, 64, True), 4, 63),            # ldw < C
    ('bn_bwd_from_G', (17, 64, True), 5, 0),             # Cn <= 0
    ('knn_reverse', (3, 2, 1, 0), 3, 0),                 # k <= 0
    ('knn_reverse', (3, 2, 1, 0), 2, 19200),             # 2 N + 1 ints past the 150 KB of LDS
    ('edge_pull_dq', (1, 40, 16, 4), 7, 6),              # H % 4
    ('edge_pull_dq', (1, 40, 16, 4), 7, 260),            # H > 256
    ('edge_pull_dq', (1, 40, 16, 4), 1, 9),              # lddz % 4
    ('edge_pull_dq', (1, 40, 16, 4), 9, 10),             # lddq % 4
]


@pytest.mark.parametrize('kernel,args,pos,bad', EINVAL, ids=lambda v: _ids(v) if isinstance(v, (str, tuple)) else repr(v))
def test_bad_arguments_are_refused(gpe, kernel, args, pos, bad):
    """GPE_EINVAL (-22) for every argument condition the launchers state, and no output is written.  MI355X: all 50 refused."""
    case = R.build(kernel, args)
    dev = _device(case)
    call = R.abi_args(case, dev)
    call[pos] = bad
    raw = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in call]
    rc = gpe._lib.query(case.kernel, *raw, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -22, rc
    for n, a in case.out0.items():
        assert dev[n].cpu().numpy().tobytes() == a.tobytes(), n

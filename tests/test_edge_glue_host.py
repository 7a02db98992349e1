"""CPU: the restated EdgeConv glue kernels of tests/edge_glue_restate.py are checked before any GPU time is spent on them.

a) the references are the right operation: composed into a whole EdgeConv layer (forward and backward, with plain fp64 matrix
   products where the layer runs a GEMM) they reproduce fp64 autograd of the oracle's DynamicEdgeConv on the same graph and the same
   winners of the max, for all three aggregations, in training and in eval mode, with a negative scale in every BatchNorm;
b) every bar passes its own reference: each checker accepts what a correct kernel returns for each case of the GPU test — the
   fp64 reference rounded once to fp32, or, for the four kernels whose fp32 order of operations is the contract (their bar is
   bit-exactness), the fp32 sequential restatement, which the checker itself holds against fp64;
c) every bar discriminates: each `variant` of each checker (a reference that is wrong in one plausible way) is rejected by at
   least one case.  The table of which cases reject which variant is printed (profiles/edge_glue_tests.md quotes it)."""
import numpy as np
import pytest
import torch

import edge_glue_restate as R

F64 = torch.float64


# ----------------------------------------------------------------------------------------------------------------------
# a) the restated pieces, composed, against fp64 autograd of the oracle
# ----------------------------------------------------------------------------------------------------------------------
def _restated_layer(x, idx, params, aggr, training, g_out, eps):
    """forward and backward of one EdgeConv layer (widths C -> H0 -> H1 -> F) from the restated kernels; GEMMs in plain fp64.
    params: per block (W, b, gamma, beta, running_mean, running_var).  -> out, (amx, amn), gradients {name: array}"""
    B, N, k = idx.shape
    BN, E = B * N, B * N * k
    C = x.shape[1]
    (W1, b1, g1, be1, rm1, rv1), (W2, b2, g2, be2, rm2, rv2), (W3, b3, g3, be3, rm3, rv3) = params
    H0 = W1.shape[0]
    jg = R.to_global(idx).reshape(BN, k)

    def stats_of(S, Q, gamma, beta, rm, rv):
        if training:
            mean, _, rstd, s, t = R.f_bn_finalize(S, Q, float(E), gamma, beta, eps)
        else:
            mean, rstd, s, t = R.f_bn_from_running(rm, rv, gamma, beta, eps)
        return mean, rstd, s, t

    # forward: [P|Q] projection -> gather statistics -> finalize -> two dense blocks -> aggregation -> finish
    Wa, Wb = W1[:, :C], W1[:, C:]
    P, Q = x @ (Wa - Wb).T + b1, x @ Wb.T
    st0 = stats_of(*R.f_gather_stats(P, Q, jg), g1, be1, rm1, rv1)
    a1 = np.maximum(P[:, None, :] + Q[jg], 0.0).reshape(E, H0)
    a2 = np.maximum((st0[2] * a1 + st0[3]) @ W2.T + b2, 0.0)
    st1 = stats_of(a2.sum(0), (a2 * a2).sum(0), g2, be2, rm2, rv2)
    a3 = np.maximum((st1[2] * a2 + st1[3]) @ W3.T + b3, 0.0)
    st2 = stats_of(a3.sum(0), (a3 * a3).sum(0), g3, be3, rm3, rv3)
    mean2, rstd2, s2, t2 = st2
    a3k = a3.reshape(BN, k, -1)
    amx = amn = None
    if aggr == 'max':
        amx, amn = a3k.argmax(1), a3k.argmin(1)
        mx, mn = a3k.max(1), a3k.min(1)
        out = R.f_finish(mx, mn, s2, t2)
        S1, S2, _, _ = R.f_point_sums(g_out, mx, mn, mean2, rstd2, s2)
        gscale = 1.0
    else:
        abar = a3k.sum(1) / k                                   # gpe_edge_sum_k, then the scale by 1 / k
        out = s2 * abar + t2 if aggr == 'mean' else s2 * (abar * k) + t2 * k
        gs = g_out if aggr == 'mean' else g_out * k             # every message carries w g_i: sums over edges = k w x point sums
        S1, S2, _, _ = R.f_point_sums(gs, abar, abar, mean2, rstd2, s2)
        gscale = 1.0 / k if aggr == 'mean' else 1.0

    def coef_of(S1, S2, st):
        coef, dgamma, dbeta = R.f_bn_bwd_coef(S1, S2, st[0], st[1], st[2], float(E))
        if not training:
            coef[1:3] = 0.0                                      # eval mode: the statistics are constants
        return coef, dgamma, dbeta

    grads = {}
    coef2, grads['gamma3'], grads['beta3'] = coef_of(S1, S2, st2)
    if aggr == 'max':
        dz3, _ = R.f_dz3(a3, g_out, coef2, k, 1.0, amx, amn)
    else:
        dz3, _ = R.f_dz3(a3, g_out * gscale, coef2, k, 1.0)     # (f_dz3 would round gscale to fp32, as the kernel's argument is)

    def block_bwd(dz, W, a_prev, st_prev, name_w, name_b, name_g, name_be):
        G = dz.T @ (a_prev - st_prev[0])                         # the centred reduce-GEMM
        db = dz.sum(0)
        sums, _, dW = R.f_bn_bwd_from_G(G, db, W, *st_prev)
        coef, grads[name_g], grads[name_be] = coef_of(sums[0], sums[1], st_prev)
        grads[name_w], grads[name_b] = dW, db
        return R.f_dz3(a_prev, dz @ W, coef, 1)[0]               # propagate + BN / ReLU backward: one row = one point of one slot

    dz2 = block_bwd(dz3, W3, a2, st1, 'W3', 'b3', 'gamma2', 'beta2')
    dz1 = block_bwd(dz2, W2, a1, st0, 'W2', 'b2', 'gamma1', 'beta1')
    # block 0: dP = the sum over each point's slots, dQ = the pull through the restated reverse graph
    off, edge = R.reverse_graph(idx)
    dP = dz1.reshape(BN, k, H0).sum(1)
    dQ = R._pull(dz1, off, edge, B, N, k, np.zeros((BN, H0)), dtype=np.float64)
    dWp, dWq = dP.T @ x, dQ.T @ x
    grads['W1'] = np.concatenate([dWp, dWq - dWp], 1)
    grads['b1'] = dP.sum(0)
    grads['x'] = dP @ (Wa - Wb) + dQ @ Wb
    return out, (amx, amn), grads


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('aggr', ['max', 'add', 'mean'])
def test_restated_layer_matches_oracle_autograd(aggr, training):
    """B = 2, N = 24, k = 5, widths 3 -> 8 -> 8 -> 6: output and every gradient at 1e-10 of the tensor's largest entry (both sides
    fp64; the margin covers the different summation order).  The oracle runs on the same graph (knn_override) and on the restated
    winners of the max (argsel_override), as tests/relu_align.py pins them for the whole-layer tests."""
    from oracle import ref_path as O
    B, N, k, widths = 2, 24, 5, [3, 8, 8, 6]
    g = torch.Generator().manual_seed(11 + 7 * training + len(aggr))
    rng = np.random.default_rng(5)
    x = torch.randn(B * N, widths[0], generator=g, dtype=F64)
    idx = R.make_graph(rng, B, N, k)
    conv = O.DynamicEdgeConv(O.MLP([2 * widths[0]] + widths[1:]), k, aggr).double()
    for blk in conv.nn:
        bn = blk[2]
        with torch.no_grad():
            bn.weight.copy_(torch.rand(bn.weight.shape, generator=g, dtype=F64) + 0.5)
            bn.weight[1::2] *= -1.0                                 # a negative scale in every BatchNorm
            bn.bias.copy_(torch.randn(bn.bias.shape, generator=g, dtype=F64))
            bn.running_mean.copy_(torch.randn(bn.bias.shape, generator=g, dtype=F64) * 0.3)
            bn.running_var.copy_(torch.rand(bn.bias.shape, generator=g, dtype=F64) + 0.5)
    conv.train(training)
    params = [tuple(t.detach().numpy().copy() for t in (blk[0].weight, blk[0].bias, blk[2].weight, blk[2].bias, blk[2].running_mean,
                                                         blk[2].running_var)) for blk in conv.nn]
    g_out = torch.randn(B * N, widths[-1], generator=g, dtype=F64)
    out, (amx, amn), grads = _restated_layer(x.numpy(), idx, params, aggr, training, g_out.numpy(), conv.nn[0][2].eps)

    conv.knn_override = torch.from_numpy(idx.reshape(B * N, k).astype(np.int64))
    if aggr == 'max':
        conv.argsel_override = (torch.from_numpy(amx), torch.from_numpy(amn))
    xr = x.clone().requires_grad_()
    ref = conv(xr, torch.arange(B * N) // N)
    ref.backward(g_out)
    assert conv.argsel_gap < 1e-12                                  # the restated winners are the oracle's
    want = {'x': xr.grad}
    for l, blk in enumerate(conv.nn, 1):
        want.update({'W%d' % l: blk[0].weight.grad, 'b%d' % l: blk[0].bias.grad, 'gamma%d' % l: blk[2].weight.grad,
                     'beta%d' % l: blk[2].bias.grad})

    def rel(a, b):
        b = b.detach().numpy()
        return float(np.abs(a - b).max() / np.abs(b).max())

    assert rel(out, ref) < 1e-10, rel(out, ref)
    assert set(want) == set(grads)
    for name in sorted(want):
        print('%s %s training=%d  %-7s %.2e' % ('restated layer', aggr, training, name, rel(grads[name], want[name])))
        assert rel(grads[name], want[name]) < 1e-10, (name, rel(grads[name], want[name]))


# ----------------------------------------------------------------------------------------------------------------------
# b) every bar passes its own reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel,args', R.case_params(), ids=lambda v: v if isinstance(v, str) else '-'.join(str(int(a)) for a in v))
def test_bar_accepts_its_reference(kernel, args):
    case = R.build(kernel, args)
    before = {n: a.copy() for n, a in {**case.inp, **case.out0}.items()}
    R.check(case, R.emulate(case, seq=kernel in R.SEQ_KERNELS))
    for n, a in {**case.inp, **case.out0}.items():                   # the shared case is left unchanged
        assert a.tobytes() == before[n].tobytes(), n


def test_bn_finalize_inputs_are_well_conditioned():
    """|mean| <= 10 std in every channel of every gpe_bn_finalize case, so that the fp64 cancellation in q / count - mean^2 moves
    rstd by less than 1e-13 relative (against 80-bit arithmetic): far inside the 2u bar"""
    worst = worst_const = 0.0
    for args in R.CASES['bn_finalize']:
        case = R.build('bn_finalize', args)
        live = case.std > 0
        assert (np.abs(case.mean[live]) <= 10 * case.std[live]).all()
        part, n = case.inp['part'], case.p['count']
        S, Q = part[:, 0].sum(0), part[:, 1].sum(0)
        eps = float(np.float32(case.p['eps']))
        r64 = 1 / np.sqrt(np.maximum(Q / n - (S / n) ** 2, 0.0) + eps)
        err = np.abs(r64 / R._ref_bn_finalize(case)['rstd'] - 1)
        worst = max(worst, float(err[live].max()) if live.any() else 0.0)
        worst_const = max(worst_const, float(err[~live].max()) if (~live).any() else 0.0)
    print('bn_finalize: fp64 against 80-bit rstd, worst relative difference %.2e; constant channels (var = 0 against eps) %.2e'
          % (worst, worst_const))
    assert worst < 1e-13
    # a constant channel (and count = 1) has no std to be within 10 of: the rounding of v^2 (1e-16 x 64) stands against eps = 1e-5
    assert worst_const < 1e-9


# ----------------------------------------------------------------------------------------------------------------------
# c) every bar discriminates
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', R.KERNELS)
def test_every_variant_is_rejected(kernel):
    assert R.VARIANTS[kernel]
    for variant in R.VARIANTS[kernel]:
        rejecting = []
        for args in R.CASES[kernel]:
            case = R.build(kernel, args)
            got = R.emulate(case, seq=kernel in R.SEQ_KERNELS)
            try:
                R.check(case, got, variant=variant)
            except AssertionError:
                rejecting.append(case.id)
        print('%s / %s: rejected by %d of %d cases: %s' % (kernel, variant, len(rejecting), len(R.CASES[kernel]), ', '.join(rejecting)))
        assert rejecting, 'no case of %s tells the variant %r from the kernel: the case list is missing an input' % (kernel, variant)


def test_case_lists_cover_the_issue():
    """every kernel has cases and variants; the knn_reverse cases take the LDS / global variant the GPU test says they take"""
    assert set(R.CASES) == set(R.VARIANTS) == set(R.KERNELS)
    lds = {(N, k): R.knn_reverse_uses_lds(N, k) for _, N, k, _ in R.CASES['knn_reverse']}
    assert lds[(2048, 16)] and lds[(1025, 3)] and not lds[(2048, 20)] and not lds[(1025, 40)]

"""-m gpu: ops.rnn_stack with start states that carry gradient, against torch.nn.LSTM / torch.nn.GRU in fp64 on the CPU.

The whole-model fixtures reach these lines of RNNStackFn.backward only in passing: the start-state loop (gpe_linear_splitk +
gpe_reduce_inner per layer), the GRU's extra gpe_add of the carry, d_c0 from carry[0], and a loss through the final states alone
(g_top is None: what LSTMEncoderModule produces).  Here each is a case of its own: LSTM and GRU, the repeated input [Bn, In] and a
sequence [Bn, T, In], both losses, exact and f16x3 arithmetic (with a refreshed PackPlan, so the fp16-pipe kernels run).

Bars: those of test_gpu_kernels.py::test_diagonal_launches_in_several_groups_and_slabs — 2e-5 for outputs and states, 1e-4 for
gradients, largest difference over largest reference magnitude.  The fp64 reference is not near them: torch's own fp32 against
fp64 at exactly these cases (seeds included), on the CPU, comes to at most 1.9e-7 on outputs and 4.6e-7 on gradients.  Worst seen
on an MI355X over the 32 cases: 1.8e-7 on outputs and states, 5.7e-7 on gradients."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(5, 12, 20, 3, 2), (17, 12, 20, 7, 3)]                  # (Bn, In, H, T, L): a ragged row tile, and two of them
OUT_BAR, GRAD_BAR = 2e-5, 1e-4


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def loss_of(top, hN, cN, w, states_only):
    """through the final states alone, or through the top layer's outputs as well; w: (w_top, w_h, w_c) of the outputs' dtype"""
    loss = (hN * w[1]).sum()
    if cN is not None:
        loss = loss + (cN * w[2]).sum()
    return loss if states_only else loss + (top * w[0]).sum()


@functools.lru_cache(maxsize=None)
def case(kind, shape, seq, states_only):
    """-> (the fp32 module, inputs, loss weights, the fp64 reference {name: tensor}); computed once, shared by the modes, never written"""
    Bn, In, Hh, T, L = shape
    lstm = kind == 'lstm'
    torch.manual_seed(Bn + T)
    rnn = (torch.nn.LSTM if lstm else torch.nn.GRU)(In, Hh, L, batch_first=True)
    ref = copy.deepcopy(rnn).double()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(Bn, T, In, generator=g) if seq else torch.randn(Bn, In, generator=g)
    h0 = torch.randn(L, Bn, Hh, generator=g) * 0.3
    c0 = torch.randn(L, Bn, Hh, generator=g) * 0.3 if lstm else None
    w = (torch.randn(Bn, T, Hh, generator=g), torch.randn(L, Bn, Hh, generator=g), torch.randn(L, Bn, Hh, generator=g))
    xr, h0r = x.double().requires_grad_(), h0.double().requires_grad_()
    c0r = c0.double().requires_grad_() if lstm else None
    inp = xr if seq else xr[:, None, :].expand(Bn, T, In)
    if lstm:
        top, (hN, cN) = ref(inp, (h0r, c0r))
    else:
        (top, hN), cN = ref(inp, h0r), None
    loss_of(top, hN, cN, [t.double() for t in w], states_only).backward()
    want = {'top': top.detach(), 'hN': hN.detach(), 'd_x': xr.grad, 'd_h0': h0r.grad}
    if lstm:
        want.update(cN=cN.detach(), d_c0=c0r.grad)
    want.update({'d_' + n: p.grad for n, p in ref.named_parameters()})
    return rnn, (x, h0, c0), w, want


@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
@pytest.mark.parametrize('states_only', [False, True], ids=['top+states', 'states'])
@pytest.mark.parametrize('seq', [False, True], ids=['repeated', 'sequence'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', ['lstm', 'gru'])
def test_rnn_stack_with_start_state_gradients(gpe, kind, shape, seq, states_only, mode):
    from gpe_amd import ops, net_blocks
    Bn, In, Hh, T, L = shape
    lstm = kind == 'lstm'
    cpu_rnn, (x, h0, c0), w, want = case(kind, shape, seq, states_only)
    rnn = copy.deepcopy(cpu_rnn).cuda()
    params = net_blocks._rnn_params(rnn, L)
    plan = ops.PackPlan()
    net_blocks._register_rnn_packs(plan, rnn, L, Hh, 4 if lstm else 3)
    prev = gpe.set_math(mode)
    try:
        plan.refresh()
        assert (ops.planned_planes(rnn.weight_hh_l0, ops.K_GATES_H3)[0] is not None) == (mode == 'f16x3')
        xd, h0d = x.cuda().requires_grad_(), h0.cuda().requires_grad_()
        c0d = c0.cuda().requires_grad_() if lstm else None
        top, hN, cN = ops.rnn_stack(xd, h0d, c0d, T, L, kind, params, want_state=True, h0_bounded=True)
        assert (cN is not None) == lstm
        loss_of(top, hN, cN, [t.cuda() for t in w], states_only).backward()
        got = {'top': top, 'hN': hN, 'd_x': xd.grad, 'd_h0': h0d.grad}
        if lstm:
            got.update(cN=cN, d_c0=c0d.grad)
        got.update({'d_' + n: p.grad for n, p in rnn.named_parameters()})
    finally:
        gpe.set_math(prev)
    assert set(got) == set(want) and all(t is not None for t in got.values())
    errs = {n: relerr(got[n], want[n]) for n in want}
    print('rnn glue %s %s %s %s %s: %s' % (kind, shape, 'sequence' if seq else 'repeated', 'states' if states_only else 'top+states', mode,
                                          ', '.join('%s %.2e' % (n, e) for n, e in errs.items())))
    for n, e in errs.items():
        assert got[n].shape == want[n].shape, n
        assert e < (GRAD_BAR if n.startswith('d_') else OUT_BAR), (n, e)

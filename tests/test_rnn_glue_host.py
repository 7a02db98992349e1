"""not-gpu: the Python that feeds the recurrence kernels (ops.py) — the flat layout of a recurrent stack's parameters and its named view,
the gradients filed by (layer, field), the all-or-nothing gathering of the f16x3 plane operands, and the argument order of the keyword
wrappers of gpe_rnn_seq_fwd / gpe_rnn_seq_bwd against the declarations of include/gpe_hip.h.  No tensor reaches a kernel and no library
is loaded."""
import inspect

import pytest
import torch

from gpe_amd import net_blocks, ops
from glue_host import Named, Ptrs, check, declared, missing_each, named, recorded  # noqa: F401  (recorded: a fixture)

FIELDS = ('w_ih', 'w_hh', 'b_ih', 'b_hh')


# ---- the layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('module', [torch.nn.LSTM, torch.nn.GRU])
def test_rnn_params_and_the_layer_view_are_inverses(module, n_layers):
    rnn = module(6, 8, n_layers, batch_first=True)
    flat = net_blocks._rnn_params(rnn, n_layers)
    assert ops.RNN_PARAMS == FIELDS and len(flat) == 4 * n_layers
    layers = ops.rnn_layers(tuple(flat), n_layers)
    assert len(layers) == n_layers
    for l, ly in enumerate(layers):
        theirs = dict(w_ih='weight_ih_l%d', w_hh='weight_hh_l%d', b_ih='bias_ih_l%d', b_hh='bias_hh_l%d')
        assert ly._fields == FIELDS
        for i, field in enumerate(FIELDS):
            assert getattr(ly, field) is getattr(rnn, theirs[field] % l), (l, field)
            assert flat[4 * l + i] is ly[i]                    # the flat order autograd sees: 4 parameters per layer
    for wrong in (flat[:-1], flat + flat[:1]):
        with pytest.raises(AssertionError):
            ops.rnn_layers(wrong, n_layers)


def test_lead_is_the_number_of_forward_arguments_in_front_of_the_parameters():
    params = list(inspect.signature(ops.RNNStackFn.forward).parameters.values())
    assert params[-1].kind is inspect.Parameter.VAR_POSITIONAL
    assert ops.RNNStackFn.LEAD == len(params) - 2 == 8        # (without ctx and *params)


@pytest.mark.parametrize('n_layers', [1, 2, 3])
def test_gradients_are_filed_where_the_flat_layout_has_the_parameter(n_layers):
    lead = ops.RNNStackFn.LEAD
    filed = {(l, f): Named('d_%s_%d' % (f, l)) for l in range(n_layers) for f in FIELDS}
    d_x, d_h0, d_c0 = Named('d_x'), Named('d_h0'), Named('d_c0')
    out = ops.rnn_grads(n_layers, filed, d_x, d_h0, d_c0)
    assert isinstance(out, tuple) and len(out) == lead + 4 * n_layers
    assert out[0] is d_x and out[1] is d_h0 and out[2] is d_c0 and out[3:lead] == (None,) * 5 and lead == 8
    for l in range(n_layers):
        for i, f in enumerate(FIELDS):
            assert out[lead + 4 * l + i] is filed[l, f], (l, f)
    # a gradient that was not filed is None, and so is everything when no gradient arrived
    part = ops.rnn_grads(n_layers, {(n_layers - 1, 'b_ih'): filed[n_layers - 1, 'b_ih']}, d_h0=d_h0)
    assert [i for i, g in enumerate(part) if g is not None] == [1, lead + 4 * (n_layers - 1) + 2]
    none = ops.rnn_grads(n_layers)
    assert len(none) == lead + 4 * n_layers and all(g is None for g in none)


# ---- the plane operands ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [ops.K_GATES_H3, ops.K_TRANS_H3])
@pytest.mark.parametrize('n_layers', [1, 2, 3])
def test_plane_operands_are_all_there_or_none(monkeypatch, n_layers, kind):
    layers = [ops.RNNLayer(*[Named('%s_%d' % (f, l)) for f in FIELDS]) for l in range(n_layers)]
    asked = [ly.w_hh for ly in layers] + [ly.w_ih for ly in layers[1:]]          # (layer 0's input weight has no planes: never asked)
    table = {id(w): [Named('planes of %r' % w), Named('amax of %r' % w)] for w in asked}

    def planned_planes(w, k):
        assert k == kind
        return tuple(table[id(w)])                            # (KeyError: a tensor that has no planes was asked for)

    monkeypatch.setattr(ops, 'planned_planes', planned_planes)
    got = ops.rnn_planes(layers, kind)
    assert len(got) == 4 and all(len(g) == n_layers for g in got)
    hh_pl, ih_pl, hh_am, ih_am = got
    assert ih_pl[0] is None and ih_am[0] is None               # entry 0 of the ih arrays is unused
    for l, ly in enumerate(layers):
        assert hh_pl[l] is table[id(ly.w_hh)][0] and hh_am[l] is table[id(ly.w_hh)][1]
        if l > 0:
            assert ih_pl[l] is table[id(ly.w_ih)][0] and ih_am[l] is table[id(ly.w_ih)][1]
    for w in asked:                                            # any single plane pack or amax word missing: none at all
        for which in (0, 1):
            kept, table[id(w)][which] = table[id(w)][which], None
            assert ops.rnn_planes(layers, kind) == (None, None, None, None) == ops.NO_PLANES, (w, which)
            table[id(w)][which] = kept
    assert ops.rnn_planes(layers, kind)[0][0] is table[id(layers[0].w_hh)][0]


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------
class Strided(Named):
    """a stand-in for a tensor whose strides the wrapper reads"""

    def __init__(self, name, strides):
        super().__init__(name)
        self.strides = tuple(strides)

    def stride(self):
        return self.strides


@pytest.fixture
def ptr_arrays(monkeypatch):
    monkeypatch.setattr(ops, '_ptr_array', Ptrs)


def per_layer(name, n_layers, first=True):
    return [Named('%s_%d' % (name, l)) if (l > 0 or first) else None for l in range(n_layers)]


def planes_of(n_layers, present):
    if not present:
        return (None, None, None, None)
    return (per_layer('hh_pl', n_layers), per_layer('ih_pl', n_layers, first=False), per_layer('hh_am', n_layers),
            per_layer('ih_am', n_layers, first=False))


def ptrs_or_none(lists):
    return [None if ts is None else Ptrs(ts) for ts in lists]


@pytest.mark.parametrize('with_ws', [True, False])
@pytest.mark.parametrize('with_planes', [True, False])
@pytest.mark.parametrize('lstm', [True, False])
def test_rnn_seq_fwd_wrapper_passes_the_declared_order(recorded, ptr_arrays, lstm, with_planes, with_ws):
    s = named(*declared('gpe_rnn_seq_fwd')[:-1])
    n_layers = 3
    hs, saved = Strided('hs', (101, 102, 103, 1)), Strided('saved', (301, 302, 303, 1))
    cs = Strided('cs', (201, 202, 203, 1)) if lstm else None
    whh, wih, bias = per_layer('whh', n_layers), per_layer('wih', n_layers, first=False), per_layer('bias', n_layers, first=False)
    bhn = None if lstm else per_layer('bhn', n_layers)
    planes = planes_of(n_layers, with_planes)
    ws = (s['ws'], s['ws_bytes']) if with_ws else (None, 0)
    kw = dict(gates=s['gates'], dims=(s['L'], s['T'], s['Bn'], s['H']), xproj=(s['xproj0'], s['xp0_sb'], s['xp0_st']), whh=whh, wih=wih,
              bias=bias, bhn=bhn, hs=hs, cs=cs, saved=saved, planes=planes, ws=ws)
    ops.rnn_seq_fwd(**kw)
    a_whh, a_wih, a_bias, a_bhn = ptrs_or_none((whh, wih, bias, bhn))
    p_hh, p_ih, m_hh, m_ih = ptrs_or_none(planes)
    expect = dict(s, whh=a_whh, wih=a_wih, bias=a_bias, bhn=a_bhn, hs=hs, hs_sl=101, hs_sb=102, hs_st=103, cs=cs,
                  cs_sl=201 if lstm else 0, cs_st=202 if lstm else 0, saved=saved, sv_sl=301, sv_st=302,
                  whh_pl=p_hh, wih_pl=p_ih, whh_amax=m_hh, wih_amax=m_ih, ws=ws[0], ws_bytes=ws[1])
    check(recorded, 'gpe_rnn_seq_fwd', expect)
    missing_each(ops.rnn_seq_fwd, kw, recorded)


@pytest.mark.parametrize('absent', [None, 'g_top', 'd_hN', 'd_cN'])
@pytest.mark.parametrize('with_planes', [True, False])
@pytest.mark.parametrize('lstm', [True, False])
def test_rnn_seq_bwd_wrapper_passes_the_declared_order(recorded, ptr_arrays, lstm, with_planes, absent):
    s = named(*declared('gpe_rnn_seq_bwd')[:-1])
    n_layers = 3
    hs, saved = Strided('hs', (101, 102, 103, 1)), Strided('saved', (301, 302, 303, 1))
    cs = Strided('cs', (201, 202, 203, 1)) if lstm else None
    g_top = Strided('g_top', (401, 402, 1)) if absent != 'g_top' else None
    d_hN = s['d_hN'] if absent != 'd_hN' else None
    d_cN = s['d_cN'] if (lstm and absent != 'd_cN') else None
    dgx = Strided('dgx', (501, 502, 503, 1))
    dgh = dgx if lstm else Strided('dgh', (501, 502, 503, 1))
    whh_t, wih_t = per_layer('whh_t', n_layers), per_layer('wih_t', n_layers, first=False)
    planes = planes_of(n_layers, with_planes)
    kw = dict(gates=s['gates'], dims=(s['L'], s['T'], s['Bn'], s['H']), g_top=g_top, d_hN=d_hN, d_cN=d_cN, whh_t=whh_t, wih_t=wih_t, hs=hs,
              cs=cs, saved=saved, dgx=dgx, dgh=dgh, part=s['part'], carry=s['carry'], planes=planes)
    ops.rnn_seq_bwd(**kw)
    a_whh, a_wih = ptrs_or_none((whh_t, wih_t))
    p_hh, p_ih, m_hh, m_ih = ptrs_or_none(planes)
    expect = dict(s, dtop=g_top, dt_sb=401 if g_top is not None else 0, dt_st=402 if g_top is not None else 0, d_hN=d_hN, d_cN=d_cN,
                  whh_t=a_whh, wih_t=a_wih, hs=hs, hs_sl=101, hs_sb=102, hs_st=103, cs=cs, cs_sl=201 if lstm else 0,
                  cs_st=202 if lstm else 0, saved=saved, sv_sl=301, sv_st=302, dgx=dgx, dgh=dgh, dg_sl=501, dg_sb=502, dg_st=503,
                  whh_tpl=p_hh, wih_tpl=p_ih, whh_amax=m_hh, wih_amax=m_ih)
    check(recorded, 'gpe_rnn_seq_bwd', expect)
    missing_each(ops.rnn_seq_bwd, kw, recorded)
    # the two gate-gradient tensors share the three dg_* strides: anything else is refused before the call
    with pytest.raises(AssertionError):
        ops.rnn_seq_bwd(**dict(kw, dgh=Strided('dgh', (501, 502, 504, 1))))
    assert recorded == []

"""not-gpu: the Python that feeds the edge kernels (ops.py) — the flat layout of an MLP's tensors and its named view, the gradients filed
by (block, field), the saved tensors by name, and the argument order of the keyword wrappers of gpe_edge_mlp_fwd / gpe_edge_redgemm /
gpe_edge_mlp_bwd against the declarations of include/gpe_hip.h.  No tensor reaches a kernel and no library is loaded."""
import inspect

import pytest
import torch

from gpe_amd import net_blocks, ops
from glue_host import Named, check, declared, missing_each, named, recorded  # noqa: F401  (recorded: a fixture)

CHANNELS = {2: [6, 8, 5], 3: [6, 8, 12, 5], 4: [6, 8, 12, 16, 5]}
FUNCTIONS = [(ops.EdgeConvFn, 11), (ops.DenseMLPFn, 5)]


# ---- the layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb', [2, 3, 4])
def test_mlp_tensors_and_the_block_view_are_inverses(nb):
    mlp = net_blocks.MLP(CHANNELS[nb])
    eps, momentum, n, flat = ops.mlp_tensors(mlp)
    assert (eps, momentum, n, len(flat)) == (mlp[0][2].eps, mlp[0][2].momentum, nb, 7 * nb)
    blocks = ops.mlp_blocks(flat, nb)
    assert len(blocks) == nb
    for l, blk in enumerate(blocks):
        lin, bn = mlp[l][0], mlp[l][2]
        named = dict(W=lin.weight, b=lin.bias, gamma=bn.weight, beta=bn.bias, running_mean=bn.running_mean, running_var=bn.running_var,
                     num_batches_tracked=bn.num_batches_tracked)
        assert blk._fields == tuple(named)
        for field, t in named.items():
            assert getattr(blk, field) is t, (l, field)
        # the flat order autograd sees: 4 parameters per block, then 3 buffers per block
        for i, t in enumerate(list(named.values())[:4]):
            assert flat[4 * l + i] is t
        for j, t in enumerate(list(named.values())[4:]):
            assert flat[4 * nb + 3 * l + j] is t
    # a backward sees the parameters alone: same names, no buffers
    for l, blk in enumerate(ops.mlp_blocks(flat[:4 * nb], nb)):
        assert all(a is b for a, b in zip(blk[:4], blocks[l][:4])) and blk[4:] == (None, None, None)


@pytest.mark.parametrize('fn, lead', FUNCTIONS)
def test_lead_is_the_number_of_forward_arguments_in_front_of_the_tensors(fn, lead):
    params = list(inspect.signature(fn.forward).parameters.values())
    assert params[-1].kind is inspect.Parameter.VAR_POSITIONAL
    assert fn.LEAD == len(params) - 2 == lead                 # (without ctx and *tensors)


@pytest.mark.parametrize('nb', [2, 3, 4])
@pytest.mark.parametrize('fn, lead', FUNCTIONS)
def test_gradients_are_filed_where_the_flat_layout_has_the_parameter(fn, lead, nb):
    fields = ('W', 'b', 'gamma', 'beta')
    assert ops.MLP_PARAMS == fields
    filed = {(l, f): Named('d%s_%d' % (f, l)) for l in range(nb) for f in fields}
    gx = Named('gx')
    out = ops.mlp_grads(fn.LEAD, nb, filed, gx)
    assert isinstance(out, tuple) and len(out) == lead + 7 * nb
    assert out[0] is gx and all(g is None for g in out[1:lead])
    for l in range(nb):
        for i, f in enumerate(fields):
            assert out[lead + 4 * l + i] is filed[l, f], (l, f)
    assert all(g is None for g in out[lead + 4 * nb:]) and len(out[lead + 4 * nb:]) == 3 * nb
    # a gradient that was not filed is None, and so is everything when no gradient arrived
    part = ops.mlp_grads(fn.LEAD, nb, {(1, 'gamma'): filed[1, 'gamma']})
    assert [i for i, g in enumerate(part) if g is not None] == [lead + 4 + 2]
    none = ops.mlp_grads(fn.LEAD, nb)
    assert len(none) == lead + 7 * nb and all(g is None for g in none)


# ---- saved tensors ---------------------------------------------------------------------------------------------------------------
class Ctx:
    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


@pytest.mark.parametrize('tail_len', [4, 1])
@pytest.mark.parametrize('nb', [2, 3, 4])
def test_saved_groups_round_trip_in_the_flat_order(nb, tail_len):
    def make(n):
        return [torch.zeros(1) for _ in range(n)]

    x, idx, jg, PQ = make(4)
    params, acts, stats, tail = tuple(make(4 * nb)), make(nb - 1), make(nb), make(tail_len)
    ctx = Ctx()
    ops.save_groups(ctx, x=x, idx=idx, jg=jg, PQ=PQ, params=params, acts=acts, stats=stats, tail=tail)
    flat = [x, idx, jg, PQ, *params, *acts, *stats, *tail]
    assert len(ctx.saved_tensors) == len(flat) == 4 + 6 * nb - 1 + tail_len
    assert all(a is b for a, b in zip(ctx.saved_tensors, flat))
    back = ops.saved_groups(ctx)
    assert list(back) == ['x', 'idx', 'jg', 'PQ', 'params', 'acts', 'stats', 'tail']
    for name, single in (('x', x), ('idx', idx), ('jg', jg), ('PQ', PQ)):
        assert back[name] is single
    for name, group in (('params', params), ('acts', acts), ('stats', stats), ('tail', tail)):
        assert len(back[name]) == len(group) and all(a is b for a, b in zip(back[name], group)), name
    # DenseMLPFn's set: x, the parameters, every activation, the stat blocks
    ctx = Ctx()
    acts = make(nb)
    ops.save_groups(ctx, x=x, params=params, acts=acts, stats=stats)
    assert all(a is b for a, b in zip(ctx.saved_tensors, [x, *params, *acts, *stats])) and len(ctx.saved_tensors) == 1 + 6 * nb
    back = ops.saved_groups(ctx)
    assert back['x'] is x and all(a is b for a, b in zip(back['acts'], acts)) and len(back['stats']) == nb


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------
def source(s, is_gathered, rows, pitch):
    """(the EdgeSrc of a variant, what the declaration's source parameters must then receive)"""
    if is_gathered:
        return ops.EdgeSrc(s['pq'], s['ldpq'], s['jg'], None, 0), {rows: None, pitch: 0}
    return ops.EdgeSrc(None, 0, None, s[rows], s[pitch]), {'pq': None, 'ldpq': 0, 'jg': None}


LAZY = ('lz_g', 'lz_ldg', 'lz_amx', 'lz_amn', 'lz_ldagg', 'lz_coef')
NO_LAZY = dict(zip(LAZY, (None, 0, None, None, 0, None)))


@pytest.mark.parametrize('with_agg', [True, False])
@pytest.mark.parametrize('is_gathered', [True, False])
def test_edge_mlp_fwd_wrapper_passes_the_declared_order(recorded, is_gathered, with_agg):
    s = named(*declared('gpe_edge_mlp_fwd')[:-1])
    src, absent = source(s, is_gathered, 'a_in', 'lda')
    agg = (s['mx'], s['mn'], s['amx'], s['amn']) if with_agg else None
    kw = dict(src=src, dims=(s['B'], s['N'], s['k']), Cin=s['Cin'], Cout=s['Cout'], wp=s['wp'], bias=s['bias'], out=s['out'], ldo=s['ldo'],
              stats_part=s['stats_part'], agg=agg, ldagg=s['ldagg'], amax_a=s['amax_a'], amax_out=s['amax_out'],
              ws=(s['ws'], s['ws_bytes']), out_half=s['out_half'])
    ops.edge_mlp_fwd(**kw)
    expect = dict(s, a_mode=0 if is_gathered else 1, agg=int(with_agg), **absent)
    if not with_agg:
        expect.update(mx=None, mn=None, amx=None, amn=None)
    check(recorded, 'gpe_edge_mlp_fwd', expect)
    missing_each(ops.edge_mlp_fwd, kw, recorded)


@pytest.mark.parametrize('with_lazy', [True, False])
@pytest.mark.parametrize('is_gathered', [True, False])
def test_edge_redgemm_wrapper_passes_the_declared_order(recorded, is_gathered, with_lazy):
    s = named(*declared('gpe_edge_redgemm')[:-1])
    v, absent = source(s, is_gathered, 'v', 'ldv')
    kw = dict(u=s['u'], ldu=s['ldu'], v=v, v_shift=s['v_shift'], dims=(s['B'], s['N'], s['k']), Mg=s['Mg'], Ng=s['Ng'], G=s['G'],
              ldG=s['ldG'], colsum=s['colsum'], part=s['part'], amax_u=s['amax_u'], amax_v=s['amax_v'], ws=(s['ws'], s['ws_bytes']))
    if with_lazy:
        kw['lazy'] = tuple(s[n] for n in LAZY)
    ops.edge_redgemm(**kw)
    check(recorded, 'gpe_edge_redgemm', dict(s, v_mode=0 if is_gathered else 1, **absent, **({} if with_lazy else NO_LAZY)))
    missing_each(ops.edge_redgemm, kw, recorded, optional=('lazy',))


@pytest.mark.parametrize('with_lazy', [True, False])
@pytest.mark.parametrize('is_gathered', [True, False])
def test_edge_mlp_bwd_wrapper_passes_the_declared_order(recorded, is_gathered, with_lazy):
    s = named(*declared('gpe_edge_mlp_bwd')[:-1])
    act = ops.EdgeSrc(s['pq'], s['ldpq'], s['jg'], None, 0) if is_gathered else None
    kw = dict(a=s['a'], lda=s['lda'], act=act, dims=(s['B'], s['N'], s['k']), Cin=s['Cin'], Cout=s['Cout'], wp=s['wp'], coef=s['coef_out'],
              out=s['dz_out'], ldo=s['ldo'], dP=s['dP'], lddp=s['lddp'], amax_a=s['amax_a'], amax_out=s['amax_out'],
              ws=(s['ws'], s['ws_bytes']))
    if with_lazy:
        kw['lazy'] = tuple(s[n] for n in LAZY)
    ops.edge_mlp_bwd(**kw)
    expect = dict(s, act_mode=int(is_gathered), **({} if with_lazy else NO_LAZY))
    if not is_gathered:
        expect.update(pq=None, ldpq=0, jg=None)
    check(recorded, 'gpe_edge_mlp_bwd', expect)
    missing_each(ops.edge_mlp_bwd, kw, recorded, optional=('lazy',))


def test_edge_sources_take_their_pitch_from_the_tensor():
    PQ, jg, rows = torch.zeros(6, 16), torch.zeros(6, 3, dtype=torch.int32), torch.zeros(18, 12)[:, :10]
    g = ops.edge_gathered(PQ, jg)
    assert g.pq is PQ and g.ldpq == 16 and g.jg is jg and g[3:] == (None, 0)
    r = ops.edge_rows(rows)
    assert r[:3] == (None, 0, None) and r.t is rows and r.ld == 12

"""not-gpu: the host side of DynamicASAPool / EdgeConvFeatures(graph_pooling) / EdgeConvPoolingFeatures — constructors, state-dict
layout, the kept-count rule, the errors — and the fp64 restatement of tests/asap_restate.py on small clouds."""
import copy

import pytest
import torch

import asap_restate as R
import gpe_amd
from gpe_amd import net_blocks as nb
from gpe_amd import ops


@pytest.mark.parametrize('ratio,N,M', [(0.3, 50, 16), (0.1, 2048, 205), (0.1, 2000, 200), (0.5, 7, 4), (1.0, 9, 1), (3, 9, 3)])
def test_kept_count_is_fp32_ceil(ratio, N, M):
    assert ops.asap_count(N, ratio) == M == R.pool_count(N, ratio)


def test_pool_state_dict_layout():
    p = nb.DynamicASAPool(56, k=5, pool_ratio=0.1)
    assert p.k == 10                                          # the reference ignores k (nn/net_blocks.py:204)
    shapes = {k: tuple(v.shape) for k, v in p.state_dict().items()}
    assert shapes == {'edge_pool.lin.weight': (56, 56), 'edge_pool.lin.bias': (56,), 'edge_pool.att.weight': (1, 112),
                      'edge_pool.att.bias': (1,), 'edge_pool.gnn_score.lin1.weight': (1, 56),
                      'edge_pool.gnn_score.lin1.bias': (1,), 'edge_pool.gnn_score.lin2.weight': (1, 56),
                      'edge_pool.gnn_score.lin3.weight': (1, 56), 'edge_pool.gnn_score.lin3.bias': (1,)}


@pytest.mark.parametrize('depth,widths', [(2, [(100, 56), (200, 112)]), (3, [(66, 37), (100, 56), (200, 112)])])
def test_pooled_encoder_widths_and_keys(depth, widths):
    enc = nb.EdgeConvFeatures(32, {'conv_depth': depth, 'graph_pooling': True, 'EConv_feature': 112, 'EConv_hidden': 200})
    orac = R.PooledEdgeConvFeatures(32, {'conv_depth': depth, 'EConv_feature': 112, 'EConv_hidden': 200})
    assert {k: v.shape for k, v in enc.state_dict().items()} == {k: v.shape for k, v in orac.state_dict().items()}
    sd = enc.state_dict()
    for l, (h, f) in enumerate(widths):
        assert sd['conv_layers.%d.nn.0.0.weight' % l].shape[0] == h
        assert sd['conv_layers.%d.nn.%d.0.weight' % (l, 2)].shape[0] == f
        assert sd['gpool_layers.%d.edge_pool.lin.weight' % l].shape == (f, f)
    assert enc.lin.in_features == 112


def test_pooling_features_keys():
    m = nb.EdgeConvPoolingFeatures(8)
    sd = m.state_dict()
    assert m.config == {'conv_depth': 3, 'n_features1': 32, 'n_features2': 128, 'n_features3': 256, 'k': 10}
    assert sd['conv1.nn.2.0.weight'].shape == (32, 64) and sd['pool1.edge_pool.lin.weight'].shape == (32, 32)
    assert sd['conv3.nn.0.0.weight'].shape == (256, 256) and sd['pool2.edge_pool.att.weight'].shape == (1, 256)
    assert sd['lin.weight'].shape == (8, 256)


def test_new_value_errors():
    with pytest.raises(ValueError, match='skip_connections'):
        nb.EdgeConvFeatures(16, {'graph_pooling': True, 'skip_connections': True})
    with pytest.raises(ValueError, match=r'\b4 points\b.*k_neighbors = 5'):
        nb._check_cloud(5, 4)
    from gpe_amd import configs, nets
    cfg = configs.att_model_config(graph_pooling=True, skip_connections=False)
    loss = dict(cfg['loss'], loss_components=['shape', 'loop', 'rotation', 'translation', 'segmentation'])
    with pytest.raises(ValueError, match="'segmentation'.*graph_pooling"):
        nets.GarmentSegmentPattern3D(configs.data_config(), copy.deepcopy(cfg), loss)


def test_pooling_features_model_keeps_raising_with_the_reason():
    from gpe_amd import configs, nets
    cfg = configs.lstm_model_config(feature_extractor='EdgeConvPoolingFeatures')
    with pytest.raises(NotImplementedError, match=r'nn/nets.py:136'):
        nets.GarmentFullPattern3D(configs.data_config(), copy.deepcopy(cfg), copy.deepcopy(cfg['loss']))


def test_pool_has_no_cpu_path():
    p = nb.DynamicASAPool(8, pool_ratio=0.5)
    with pytest.raises(RuntimeError, match='no CPU path'):
        p(torch.randn(2 * 16, 8), (2, 16))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.asap_pool(torch.randn(16, 8), 1, 16, [q.detach() for q in p.edge_pool.params()], 0.5)


def test_restatement_graph_is_reverse_knn_with_self_loops():
    torch.manual_seed(0)
    B, N, F = 2, 30, 5
    x = torch.randn(B * N, F, dtype=torch.float64)
    knn = R.pool_graph(x, B, N)
    assert knn.shape == (B * N, 10)
    src, dst = R._edges(knn, B, N)
    assert ((src != dst).sum() + B * N) == src.numel()
    for q, c in zip(src.tolist(), dst.tolist()):          # c receives from q: c is among q's neighbours (or q == c)
        assert q == c or (c - q // N * N) in knn[q].tolist()


def test_restatement_gradients_match_finite_differences():
    torch.manual_seed(1)
    B, N, F = 2, 24, 6
    x = torch.randn(B * N, F, dtype=torch.float64, requires_grad=True)
    pool = R._ASAPooling(F, 0.5).double()
    info = {}
    R.asap_pool(x, B, N, pool.params(), 0.5, info=info)
    dec = {'knn': info['knn'], 'winners': info['winners'], 'perm': info['perm']}
    fn = lambda xx, *ps: R.asap_pool(xx, B, N, list(ps), 0.5, **dec)[0]
    assert torch.autograd.gradcheck(fn, (x,) + tuple(p.detach().requires_grad_() for p in pool.params()), eps=1e-6, atol=1e-5)


# ---- fixtures made by the reference's own modules (scripts/make_asap_golden.py) ---------------------------------------------------
import os                                                  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = ('asap_encoder_d2.pt', 'asap_encoder_d3.pt', 'asap_pool.pt', 'asap_pooling_features.pt')


def _fixture(name):
    return torch.load(os.path.join(GOLDEN, name), weights_only=False)


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_matches_reference_fixture(name):
    """the fp64 restatement, wired by this project, computes what the reference's own modules computed"""
    fx = _fixture(name)
    if fx['kind'] == 'EdgeConvFeatures':
        m = R.PooledEdgeConvFeatures(fx['out_size'], fx['config'])
        m.load_state_dict(fx['state_dict'], strict=True)
        m = m.double().train()
        with torch.no_grad():
            enc, out, batch = m(fx['positions'])
        assert out.shape == fx['out'].shape and torch.equal(batch, fx['batch'])
        assert torch.allclose(enc, fx['encoding'], rtol=0, atol=1e-10) and torch.allclose(out, fx['out'], rtol=0, atol=1e-10)
    elif fx['kind'] == 'DynamicASAPool':
        m = R.DynamicASAPool(fx['F'], k=fx['k_given'], pool_ratio=fx['ratio'])
        m.load_state_dict(fx['state_dict'], strict=True)
        m = m.double()
        with torch.no_grad():
            out, M = m(fx['x'], fx['B'], fx['N'])
        assert torch.equal(torch.arange(fx['B']).repeat_interleave(M), fx['batch'])
        assert torch.allclose(out, fx['out'], rtol=0, atol=1e-10)
    else:
        m = R.PoolingFeatures(fx['out_size'], fx['config'])
        m.load_state_dict(fx['state_dict'], strict=True)
        m = m.double().train()
        with torch.no_grad():
            out = m(fx['positions'])
        assert torch.allclose(out, fx['out'], rtol=0, atol=1e-10)


@pytest.mark.parametrize('name', FIXTURES)
def test_drop_in_constructors_match_reference_fixture(name):
    """the drop-in modules have the reference's keys, shapes, merged config, k, kept counts and output shapes"""
    fx = _fixture(name)
    # every knn the reference's pools ran asked for k = 10, whatever k they were given (nn/net_blocks.py:204)
    assert fx['knn_calls'] and all(c['k'] == 10 == ops.ASAP_K for c in fx['knn_calls'])
    assert all(c['neighbours'] == min(10, c['n_points']) for c in fx['knn_calls'])
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    if fx['kind'] == 'EdgeConvFeatures':
        m = nb.EdgeConvFeatures(fx['out_size'], fx['config'])
        assert shapes(m) == fx['shapes'] and list(m.state_dict()) == list(fx['state_dict'])
        assert m.config == fx['merged_config']
        N = fx['N']
        for call in fx['knn_calls']:                       # one pool per conv, each on the previous pool's output
            assert call['n_points'] == N
            N = ops.asap_count(N, fx['config']['pool_ratio'])
        assert fx['out'].shape == (fx['B'] * N, m.lin.in_features) and fx['encoding'].shape == (fx['B'], fx['out_size'])
        assert torch.equal(fx['batch'], torch.arange(fx['B']).repeat_interleave(N))
    elif fx['kind'] == 'DynamicASAPool':
        m = nb.DynamicASAPool(fx['F'], k=fx['k_given'], pool_ratio=fx['ratio'])
        assert shapes(m) == fx['shapes'] and list(m.state_dict()) == list(fx['state_dict']) and m.k == 10
        M = ops.asap_count(fx['N'], fx['ratio'])
        assert fx['out'].shape == (fx['B'] * M, fx['F'])
        assert torch.equal(fx['batch'], torch.arange(fx['B']).repeat_interleave(M))
    else:
        m = nb.EdgeConvPoolingFeatures(fx['out_size'], fx['config'])
        assert shapes(m) == fx['shapes'] and list(m.state_dict()) == list(fx['state_dict'])
        assert m.config == fx['merged_config']
        assert shapes(nb.EdgeConvPoolingFeatures(fx['out_size'])) == fx['default_shapes']
        assert [c['n_points'] for c in fx['knn_calls']] == [fx['N'], ops.asap_count(fx['N'], 0.5)]
        assert fx['out'].shape == (fx['B'], fx['out_size'])

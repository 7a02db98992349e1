"""-m gpu: the encoder's prediction path (csrc/gpe_edge_predict.hip through ops.edge_conv_predict, DynamicEdgeConv.predict,
EdgeConvFeatures.predict, model.predict) against the CPU oracle in eval mode on the path's own graphs, and against today's eval-mode
forward.  Bars: those of the existing layer / fixture tests (test_gpu_kernels.TOL, test_gpu_model's max(1e-4, 20 x e32))."""
import copy
import os

import pytest
import torch

from test_gpu_kernels import TOL, relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


@pytest.fixture(params=['f32', 'f16x3'])
def mode(request, gpe):
    """the two arithmetics of the fused kernel, the f16x3 size gate lifted so that the small shapes run the fp16-pipe kernel"""
    prev = gpe.set_math(request.param)
    gate = gpe.set_f16x3_min_rows(0)
    yield request.param
    gpe.set_f16x3_min_rows(gate)
    gpe.set_math(prev)


def _convs(gpe, C, H, Fo, k, hidden, aggr='max', seed=0):
    """-> (oracle conv, product conv in eval mode) with the same weights: BatchNorm affine parameters and running statistics away from
    their defaults, every third scale of the last BatchNorm negative (the min branch of the max aggregation)"""
    from oracle import ref_path as O
    torch.manual_seed(seed)
    chans = [2 * C] + [H] * (hidden + 1) + [Fo]
    oconv = O.DynamicEdgeConv(O.MLP(chans), k=k, aggr=aggr)
    with torch.no_grad():
        for blk in oconv.nn:
            blk[2].weight.uniform_(0.5, 1.5)
            blk[2].bias.uniform_(-0.3, 0.3)
            blk[2].running_mean.uniform_(0.1, 0.4)
            blk[2].running_var.uniform_(0.5, 1.5)
        oconv.nn[-1][2].weight[::3] *= -1
    assert (oconv.nn[-1][2].weight < 0).sum().item() * 4 >= Fo
    pconv = gpe.net_blocks.DynamicEdgeConv(gpe.net_blocks.MLP(chans), k=k, aggr=aggr)
    pconv.load_state_dict(oconv.state_dict())
    return oconv, pconv.cuda().eval()


def _layer_bar(oconv, x, B, N, k, graph, out, mode):
    """test_edgeconv_layer_fwd_bwd's forward bar against the fp64 oracle in eval mode on `graph`"""
    batch = torch.arange(B).repeat_interleave(N)
    o64 = copy.deepcopy(oconv).double().eval()
    o64.knn_override = graph
    o32 = copy.deepcopy(oconv).eval()
    o32.knn_override = graph
    with torch.no_grad():
        ref = o64(x.double(), batch)
        err32 = relerr(o32(x.clone(), batch), ref)
    err = relerr(out, ref)
    print('edge predict %s relerr build=%.2e oracle-fp32=%.2e' % (mode, err, err32))
    assert out.shape == ref.shape
    assert err < max(TOL[mode]['fwd'], 20 * err32), (err, err32)


# (B, N, C, H, F, k, hidden H x H layers)
SHAPES = [(2, 50, 3, 200, 112, 5, 1),          # 12 points per tile, 4 padding rows, ragged last tile, a tile across the cloud boundary
          (1, 130, 150, 200, 150, 16, 1),      # full tiles + a 2-point tail, wide layer-2 input
          (2, 64, 112, 200, 112, 20, 1),       # 3 points per tile
          (1, 70, 3, 28, 12, 7, 1),            # widths below one K slab, the 4-block menu entry
          (1, 64, 3, 64, 128, 16, 1),          # F > H
          (1, 48, 3, 256, 256, 16, 1),         # the menu's upper edge (f16x3 lands on the exact kernel)
          (1, 64, 3, 200, 112, 16, 0),         # depth 1
          (1, 64, 3, 96, 64, 16, 2),           # depth 3
          (1, 80, 3, 200, 112, 64, 1)]         # k = 64: one point per tile
CASES = [s + ('max',) for s in SHAPES] + [SHAPES[0] + ('mean',), SHAPES[0] + ('add',)]


@pytest.mark.parametrize('B,N,C,H,Fo,k,hidden,aggr', CASES)
def test_fused_layer_vs_fp64_oracle(gpe, mode, B, N, C, H, Fo, k, hidden, aggr):
    from oracle import ref_path as O
    oconv, pconv = _convs(gpe, C, H, Fo, k, hidden, aggr, seed=B + N + C + hidden)
    assert gpe.ops.edge_predict_on_menu(pconv.nn, k)
    x = torch.randn(B * N, C, generator=torch.Generator().manual_seed(1))
    out = pconv.predict(x.cuda(), B, N, route='fused')
    assert not out.requires_grad and pconv.last_order is not None
    graph = pconv.last_knn.cpu().view(B * N, k).long()
    if C == 3:
        assert torch.equal(graph, O.knn_local(x, B, k))
    _layer_bar(oconv, x, B, N, k, graph, out, mode)


@pytest.mark.parametrize('B,N,C,H,Fo,k,hidden', [SHAPES[0], SHAPES[1], SHAPES[7]])
def test_layers_route_is_todays_eval_forward(gpe, mode, B, N, C, H, Fo, k, hidden):
    _, pconv = _convs(gpe, C, H, Fo, k, hidden, seed=3)
    x = torch.randn(B * N, C, generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        want = pconv(x, B, N)
    want_idx, want_order = pconv.last_knn, pconv.last_order
    got = pconv.predict(x, B, N, route='layers')
    assert torch.equal(got, want) and torch.equal(pconv.last_knn, want_idx) and torch.equal(pconv.last_order, want_order)
    pconv.predict(x, B, N, route='fused')
    assert torch.equal(pconv.last_knn, want_idx) and torch.equal(pconv.last_order, want_order)
    # 'auto' lands on one of the two
    auto = pconv.predict(x, B, N)
    assert torch.equal(auto, want) or torch.equal(auto, pconv.predict(x, B, N, route='fused'))


def test_fused_route_off_the_menu_raises(gpe):
    _, pconv = _convs(gpe, 3, 200, 112, 65, 1)                        # k = 65: refused before anything is launched
    with pytest.raises(ValueError, match="route='fused'"):
        pconv.predict(torch.randn(2 * 80, 3).cuda(), 2, 80, route='fused')
    # four hidden layers: off the fused menu, within what the layer kernels take; 'auto' is today's eval forward
    B, N, C, H, Fo, k = 2, 70, 6, 40, 28, 5
    _, pconv = _convs(gpe, C, H, Fo, k, 4)
    assert not gpe.ops.edge_predict_on_menu(pconv.nn, k)
    x = torch.randn(B * N, C, generator=torch.Generator().manual_seed(6)).cuda()
    with pytest.raises(ValueError, match="route='fused'"):
        pconv.predict(x, B, N, route='fused')
    with torch.no_grad():
        want = pconv(x, B, N)
    assert torch.equal(pconv.predict(x, B, N), want)


@pytest.mark.parametrize('tag', ['full3d_small', 'full3d_k16', 'segment3d_small', 'segment3d_k20'])
def test_model_predict_vs_oracle(gpe, mode, tag, golden_dir):
    from oracle import ref_path as O
    fx = torch.load(os.path.join(golden_dir, tag + '.pt'), weights_only=False)
    torch.manual_seed(fx['seed'])
    model = getattr(gpe.nets, fx['model'])(fx['data_config'], copy.deepcopy(fx['nn_config']), copy.deepcopy(fx['loss_config'])).cuda().train()
    feats = fx['features']
    for it in range(2):                                   # move the running statistics
        torch.manual_seed(fx['seed'] + it)
        model(feats.cuda(), log_step=0, epoch=fx.get('epoch', 0))
    model.eval()
    B, N = feats.shape[0], feats.shape[1]
    state = {n: v.detach().cpu() for n, v in model.state_dict().items()}
    for route in ('auto', 'fused'):
        torch.manual_seed(fx['seed'] + 2)                 # the decoders' random initial states are part of the contract
        preds = model.predict(feats.cuda()) if route == 'auto' else model.predict(feats.cuda(), route=route)
        convs = model.feature_extractor.conv_layers
        knn = [c.last_knn.cpu().view(-1, c.k).long() for c in convs]
        assert torch.equal(knn[0], O.knn_local(feats.reshape(B * N, -1), B, convs[0].k))
        outs = []
        for double in (True, False):
            torch.manual_seed(fx['seed'])
            om = getattr(O, fx['model'])(fx['data_config'], copy.deepcopy(fx['nn_config']), copy.deepcopy(fx['loss_config']))
            om.load_state_dict(state)
            om = (om.double() if double else om).eval()
            for conv, idx in zip(om.feature_extractor.conv_layers, knn):
                conv.knn_override = idx
            torch.manual_seed(fx['seed'] + 2)
            with torch.no_grad():
                outs.append(om(feats.double() if double else feats))
        ref, p32 = outs
        assert set(preds.keys()) == set(ref.keys())
        assert ('att_weights' in preds) == ('att_weights' in fx['preds'])
        for key, v in ref.items():
            assert preds[key].shape == v.shape and not preds[key].requires_grad
            err = (preds[key].cpu().double() - v).abs().max().item()
            e32 = (p32[key].double() - v).abs().max().item()
            print('%s %s route=%s %s: err %.2e (fp32 oracle %.2e)' % (tag, mode, route, key, err, e32))
            assert err < max(1e-4, 20 * e32), (route, key, err, e32)


def test_fused_route_stores_nothing_per_edge(gpe):
    B, N, k, H, Fo = 2, 512, 16, 200, 112
    _, pconv = _convs(gpe, 3, H, Fo, k, 1, seed=5)
    x = torch.randn(B * N, 3, generator=torch.Generator().manual_seed(4)).cuda()
    E = B * N * k

    def peak(route):
        pconv.predict(x, B, N, route=route)               # warm: workspaces, the library's one-time attribute calls
        torch.cuda.synchronize()
        rest = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = pconv.predict(x, B, N, route=route)
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - rest
        del out
        return p

    layers, fused = peak('layers'), peak('fused')
    print('peak bytes above rest: layers %d, fused %d (one [E, %d] fp32 activation = %d)' % (layers, fused, H, E * H * 4))
    # the layers route holds a_1 [E, 200] and a_2 [E, 112]; the fused route holds no [E, .] tensor
    assert fused <= layers - E * H * 4


@pytest.mark.parametrize('variant', ['skip', 'pool'])
def test_features_predict_skip_and_pooling(gpe, mode, variant):
    from oracle import ref_path as O
    cfg = {'k_neighbors': 4, 'EConv_hidden': 200, 'EConv_feature': 112}
    cfg.update({'skip_connections': True} if variant == 'skip' else {'graph_pooling': True, 'pool_ratio': 0.5})
    torch.manual_seed(7)
    ext = gpe.net_blocks.EdgeConvFeatures(40, cfg).cuda()
    B, N = 2, 64
    pos = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(8))
    ext.train()
    ext(pos.cuda())                                       # move the running statistics
    ext.eval()
    with torch.no_grad():
        want = ext(pos.cuda())
    want_graph = ext.conv_layers[0].last_knn.clone()
    got = ext.predict(pos.cuda(), route='fused')
    assert torch.equal(ext.conv_layers[0].last_knn, want_graph)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and not a.requires_grad
    assert got[1].shape[1] == 112 + (3 if variant == 'skip' else 0)
    assert got[1].shape[0] == (B * N if variant == 'skip' else B * 16)
    # the first conv's output against the fp64 oracle, the bar of the layer test
    conv = ext.conv_layers[0]
    H0, F0 = conv.nn[0][0].weight.shape[0], conv.nn[-1][0].weight.shape[0]
    oconv = O.DynamicEdgeConv(O.MLP([6] + [H0] * (len(conv.nn) - 1) + [F0]), k=conv.k, aggr=conv.aggr)
    oconv.load_state_dict({n: v.detach().cpu() for n, v in conv.state_dict().items()})
    x = pos.reshape(B * N, 3)
    out = conv.predict(x.cuda(), B, N, route='fused')
    _layer_bar(oconv, x, B, N, conv.k, conv.last_knn.cpu().view(B * N, conv.k).long(), out, mode)

"""DynamicASAPool on the device (csrc/gpe_asap.hip, ops.AsapPoolFn) against the fp64 restatement of tests/asap_restate.py, on the
build's own decisions (pool graph, channel-max winners, kept rows), which are themselves checked against the restatement's."""
import copy

import pytest
import torch

import asap_restate as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _cloud(kind, B, N, F, g):
    if kind == 'normal':
        return torch.randn(B * N, F, generator=g)
    if kind == 'hubs':
        # 4 centres per cloud, every other point on the unit sphere around one of them: the points of a sphere are ~sqrt(2) apart,
        # their centre 1 away, so each centre is in the kNN list of its whole sphere (in-degree ~ N / 4)
        x = torch.randn(B, N, F, generator=g)
        x = x / x.norm(dim=-1, keepdim=True)
        centres = 3 * torch.randn(B, 4, F, generator=g)
        lab = torch.arange(N) % 4
        x = x + centres[:, lab]
        x[:, :4] = centres[:, :4]
        return x.reshape(B * N, F)
    if kind == 'dups':
        x = torch.randn(B, N, F, generator=g)
        x[:, N // 2:N // 2 + N // 4] = x[:, :N // 4]                # a quarter of every cloud twice
        x[:, -3:] = x[:, 5:6]                                        # and one point four times
        return x.reshape(B * N, F)
    if kind == 'manydups':
        # 15 copies of one point (> k = 10), far from every other point: every copy's list holds the 10 lowest-numbered copies, so
        # the five highest-numbered copies are pushed out of their own lists, and the clusters of the ten others coincide (all 15
        # copies), which makes their fitness tie exactly
        x = torch.randn(B, N, F, generator=g)
        x[:, 7] += 50.0
        x[:, 20:34] = x[:, 7:8]
        return x.reshape(B * N, F)
    raise ValueError(kind)


def _run(gpe, F, N, B, ratio, kind='normal', seed=0):
    from gpe_amd import net_blocks as nb
    g = torch.Generator().manual_seed(seed)
    x = _cloud(kind, B, N, F, g)
    torch.manual_seed(seed + 1)
    pool = nb.DynamicASAPool(F, pool_ratio=ratio)
    pool.keep_decisions = True
    with torch.no_grad():                          # livelier scores than the default init (softmax and fitness away from flat)
        for p in pool.parameters():
            p.mul_(3.0)
    pool = pool.to(DEV)
    xd = x.to(DEV).requires_grad_()
    out, (_, M) = pool(xd, (B, N))
    gout = torch.randn(out.shape, generator=g)
    out.backward(gout.to(DEV))
    torch.cuda.synchronize()
    return pool, x, xd, out, gout, M


def _kept_in_fitness_order(pool, B, N):
    """the build's kept rows are ITS OWN fitness ranking with ties to the lower index: per cloud, the kept (fitness desc, index asc)
    keys rise strictly and no dropped node ranks before the last kept one"""
    fit = pool.last['fitness'].cpu().double().view(B, N)
    perm = pool.last['perm'].cpu().long().view(B, -1)
    for b in range(B):
        keys = [(-fit[b, c].item(), c) for c in (perm[b] - b * N).tolist()]
        assert all(a < z for a, z in zip(keys, keys[1:]))
        kept = set((perm[b] - b * N).tolist())
        assert all((-fit[b, c].item(), c) > keys[-1] for c in range(N) if c not in kept)


def _check(gpe, F, N, B, ratio, kind='normal', seed=0, layer_floor=1e-2, tol=1e-4, loose=None):
    """loose: {parameter name: (layer_floor, tol)} for the parameters of a case whose bar is set apart (reason at the call)"""
    pool, x, xd, out, gout, M = _run(gpe, F, N, B, ratio, kind, seed)
    assert M == R.pool_count(N, ratio) and out.shape == (B * M, F)
    dec = R.build_decisions(pool)
    params = [p.detach().cpu().double().requires_grad_() for p in pool.edge_pool.params()]
    xr = x.double().requires_grad_()
    info = {}
    ref, _ = R.asap_pool(xr, B, N, params, ratio, info=info, **dec)
    ref.backward(gout.double())
    # the build's decisions are the restatement's own: same graph rules, same tie rules; kept rows wherever the margin allows
    own_graph = R.pool_graph(x.double(), B, N)
    assert torch.equal(own_graph, dec['knn']), 'pool graph differs from oracle.ref_path.knn_local'
    assert info['winner_gap'] == 0.0 and torch.equal(dec['winners'], info['own_winners'])    # maxima, lowest source on ties
    _kept_in_fitness_order(pool, B, N)
    if info['perm_margin'] >= 5e-5:
        assert torch.equal(dec['perm'], info['own_perm'])
    else:
        assert info['perm_gap'] < 5e-5
    err = (out.detach().cpu().double() - ref.detach()).abs().max().item()
    assert err < 1e-4 * max(1.0, ref.abs().max().item()), err
    gx = xd.grad.cpu().double()
    assert (gx - xr.grad).abs().max().item() <= 1e-4 * xr.grad.abs().max().item() + 1e-12
    # the query-branch gradients (lin, att.bias, the w_q half of att) are sums of a softmax's gradients over each cluster; where
    # every score of a cluster has the same sign they cancel to zero exactly, and what is left in fp32 is rounding of terms of
    # the layer's scale — so a parameter's bar is relative to the largest gradient of the layer when its own is far smaller
    layer = max(r.grad.abs().max().item() for r in params)
    for (name, p), r in zip(pool.edge_pool.named_parameters(), params):
        e = (p.grad.cpu().double() - r.grad).abs().max().item()
        fl, tl = (loose or {}).get(name, (layer_floor, tol))
        assert e <= tl * max(r.grad.abs().max().item(), fl * layer) + 1e-12, (name, e, r.grad.abs().max().item(), layer)
    return pool, info


CASES = [(F, N, B, [0.1, 0.3, 0.5][(i + j + b) % 3]) for i, F in enumerate((32, 56, 112, 128))
         for j, N in enumerate((50, 205, 1000, 2048)) for b, B in enumerate((1, 4))]


@pytest.mark.parametrize('F,N,B,ratio', CASES + [(512, 2048, 1, 0.3), (56, 8192, 1, 0.1)])
@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
def test_asap_pool_matches_restatement(gpe, mode, F, N, B, ratio):
    prev = gpe.set_math(mode)
    try:
        _check(gpe, F, N, B, ratio, seed=F + N + B)
    finally:
        gpe.set_math(prev)


@pytest.mark.parametrize('ratio', [0.1, 0.3, 0.5])
@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
def test_asap_pool_every_math_mode(gpe, mode, ratio):
    prev = gpe.set_math(mode)
    try:
        _check(gpe, 56, 205, 4, ratio, seed=7)
    finally:
        gpe.set_math(prev)


def test_asap_pool_hubs(gpe):
    # clusters of ~250 sources whose scores share one sign: the query-branch gradients are a cancellation to zero, and their fp32
    # residue scales with the layer's largest gradient (~2e-6 of it here), not with their own (fp64: 1e-12); and a hub's fitness
    # pre-activation is a sum over ~250 sources far from zero, where sigmoid' turns its fp32 rounding into a relative error of
    # the same size (2.8e-4 on gnn_score.lin1 here)
    query = {n: (1.0, 1e-4) for n in ('lin.weight', 'lin.bias', 'att.weight', 'att.bias')}
    fitness = {n: (1e-2, 1e-3) for n in ('gnn_score.lin1.weight', 'gnn_score.lin1.bias', 'gnn_score.lin2.weight',
                                         'gnn_score.lin3.weight', 'gnn_score.lin3.bias')}
    pool, info = _check(gpe, 32, 1000, 2, 0.3, kind='hubs', seed=3, loose={**query, **fitness})
    indeg = torch.bincount(info['knn'].reshape(-1) + (torch.arange(2000) // 1000 * 1000).repeat_interleave(10), minlength=2000)
    assert indeg.max().item() >= 200


def test_asap_pool_duplicates(gpe):
    _check(gpe, 56, 205, 2, 0.5, kind='dups', seed=4)


def test_asap_pool_more_copies_than_k(gpe):
    pool, info = _check(gpe, 32, 205, 2, 0.5, kind='manydups', seed=6)
    knn = info['knn'].view(2, 205, 10)
    assert all(c not in knn[b, c].tolist() for b in range(2) for c in range(29, 34))     # pushed out of their own lists
    fit = pool.last['fitness'].cpu().view(2, 205)
    assert (fit[:, 7:8] == fit[:, 20:29]).all()                                           # exact ties among the copies


def test_asap_pool_small_cloud(gpe):
    _check(gpe, 32, 7, 3, 0.5, seed=5)                    # fewer than 10 points: min(10, N) neighbours


def test_asap_pool_is_reproducible(gpe):
    runs = []
    for _ in range(2):
        pool, x, xd, out, gout, M = _run(gpe, 112, 2048, 4, 0.1, seed=11)
        runs.append([out.detach().clone(), xd.grad.clone()] + [p.grad.clone() for p in pool.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_asap_pool_no_grad_keeps_nothing(gpe):
    from gpe_amd import net_blocks as nb
    pool = nb.DynamicASAPool(32, pool_ratio=0.5).to(DEV)
    x = torch.randn(2 * 64, 32, device=DEV)
    with torch.no_grad():
        out, (B, M) = pool(x, (2, 64))
    assert out.grad_fn is None and (B, M) == (2, 32) and pool.last == {}          # no decisions kept unless asked for
    out2, batch = pool(x, torch.arange(2, device=DEV).repeat_interleave(64))      # the reference's LongTensor batch
    assert torch.equal(out2, out) and torch.equal(batch.cpu(), torch.arange(2).repeat_interleave(32))


def _encoder_pair(gpe, cfg, seed=0):
    from gpe_amd import net_blocks as nb
    torch.manual_seed(seed)
    prod = nb.EdgeConvFeatures(32, dict(cfg, graph_pooling=True))
    orac = R.PooledEdgeConvFeatures(32, dict(cfg, graph_pooling=True))
    orac.load_state_dict(prod.state_dict(), strict=True)
    return prod.to(DEV).train(), orac.double().train()


def _grad_check(prod, orac, tol=2e-3):
    pn = dict(prod.named_parameters())
    for n, p in orac.named_parameters():
        if pn[n].grad is None or p.grad is None:          # a parameter the forward does not reach (e.g. an unused encoder lin)
            other = p.grad if pn[n].grad is None else pn[n].grad
            assert other is None or not other.abs().max().item(), n
            continue
        gerr = (pn[n].grad.cpu().double() - p.grad).abs().max().item() / (p.grad.abs().max().item() + 1e-12)
        assert gerr < tol, (n, gerr)


@pytest.mark.parametrize('depth,B,N,k,F', [(2, 2, 256, 5, 112), (3, 2, 256, 5, 112), (2, 32, 2048, 16, 112)])
def test_pooled_encoder_matches_fp64_composition(gpe, depth, B, N, k, F):
    cfg = {'conv_depth': depth, 'k_neighbors': k, 'EConv_feature': F, 'EConv_hidden': 200, 'pool_ratio': 0.1 if N > 1000 else 0.3}
    prod, orac = _encoder_pair(gpe, cfg)
    for p in prod.gpool_layers:
        p.keep_decisions = True
    g = torch.Generator().manual_seed(9)
    pos = torch.randn(B, N, 3, generator=g)
    enc, out, batch = prod(pos.to(DEV))
    ge = torch.randn(enc.shape, generator=g)
    (enc * ge.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    R.pin_to_build(orac, prod)
    renc, rout, rbatch = orac(pos.double())
    (renc * ge.double()).sum().backward()
    assert out.shape == rout.shape and torch.equal(batch.cpu(), rbatch)
    assert (enc.detach().cpu().double() - renc.detach()).abs().max().item() < 1e-4 * max(1.0, renc.abs().max().item())
    for pp, op in zip(prod.gpool_layers, orac.gpool_layers):
        # (the pooled features differ from fp64 by the conv's rounding: the build's winners may differ within it)
        assert op.info['winner_gap'] < 5e-5 and op.info['perm_gap'] < 5e-5
    _grad_check(prod, orac)


def _model_pair(gpe, kind):
    from gpe_amd import configs, nets
    from oracle import ref_path as O
    data_config = configs.data_config()
    if kind == 'full':
        cfg = configs.lstm_model_config(k_neighbors=5, graph_pooling=True, pool_ratio=0.3)
        cls, ocls = nets.GarmentFullPattern3D, O.GarmentFullPattern3D
    else:
        cfg = configs.att_model_config(k_neighbors=5, graph_pooling=True, pool_ratio=0.3, skip_connections=False)
        cls, ocls = nets.GarmentSegmentPattern3D, O.GarmentSegmentPattern3D
    torch.manual_seed(0)
    prod = cls(data_config, copy.deepcopy(cfg), copy.deepcopy(cfg['loss']))
    ocfg = dict(copy.deepcopy(cfg), graph_pooling=False)
    orac = ocls(data_config, ocfg, copy.deepcopy(cfg['loss']))
    orac.feature_extractor = R.PooledEdgeConvFeatures(prod.feature_extractor.lin.out_features, prod.feature_extractor.config)
    orac.load_state_dict(prod.state_dict(), strict=True)
    return data_config, prod.to(DEV).train(), orac.double().train()


@pytest.mark.parametrize('kind', ['full', 'segment'])
def test_pooled_models_match_fp64_composition(gpe, kind):
    import bench
    data_config, prod, orac = _model_pair(gpe, kind)
    prod.loss.with_quality_eval = False
    for p in prod.feature_extractor.gpool_layers:
        p.keep_decisions = True
    feats, gt = bench.synthetic(2, 256, data_config, seed=1000, device='cpu')
    torch.manual_seed(5)
    preds = prod(feats.to(DEV))
    loss = prod.loss(preds, {k: v.to(DEV) for k, v in gt.items()}, epoch=0)[0]
    loss.backward()
    torch.cuda.synchronize()
    R.pin_to_build(orac.feature_extractor, prod.feature_extractor)
    torch.manual_seed(5)
    ref = orac(feats.double())
    rloss = orac.loss(ref, {k: v.clone() for k, v in gt.items()}, epoch=0)[0]
    rloss.backward()
    for key in ref:
        if key in preds and torch.is_tensor(ref[key]) and ref[key].numel():
            assert (preds[key].detach().cpu().double() - ref[key]).abs().max().item() < 1e-4, key
    assert abs(loss.item() - rloss.item()) < 1e-4 * max(1.0, abs(rloss.item()))
    _grad_check(prod, orac)


def test_edge_conv_pooling_features_forward_backward(gpe):
    from gpe_amd import net_blocks as nb
    from oracle import ref_path as O
    torch.manual_seed(0)
    prod = nb.EdgeConvPoolingFeatures(16).to(DEV).train()
    prod.pool1.keep_decisions = prod.pool2.keep_decisions = True
    g = torch.Generator().manual_seed(2)
    pos = torch.randn(2, 200, 3, generator=g)
    out = prod(pos.to(DEV))
    assert out.shape == (2, 16)
    gy = torch.randn(2, 16, generator=g)
    (out * gy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    # fp64: conv1 -> pool1 -> conv2 -> pool2 -> conv3 -> global max -> lin on the build's decisions
    sd = {k: v.detach().cpu().double() for k, v in prod.state_dict().items()}
    c = prod.config
    convs = [O.DynamicEdgeConv(O.MLP([6, 64, 64, c['n_features1']]), k=10),
             O.DynamicEdgeConv(O.MLP([2 * c['n_features1']] + [c['n_features2']] * 3), k=10),
             O.DynamicEdgeConv(O.MLP([2 * c['n_features2']] + [c['n_features3']] * 3), k=10)]
    pools = [R.DynamicASAPool(c['n_features1']), R.DynamicASAPool(c['n_features2'])]
    lin = torch.nn.Linear(c['n_features3'], 16)
    holder = torch.nn.Module()
    for i, m in enumerate(convs):
        holder.add_module('conv%d' % (i + 1), m)
    for i, m in enumerate(pools):
        holder.add_module('pool%d' % (i + 1), m)
    holder.add_module('lin', lin)
    holder.load_state_dict(sd, strict=True)
    holder.double().train()
    for oc, pc in zip(convs, (prod.conv1, prod.conv2, prod.conv3)):
        oc.knn_override = pc.last_knn.cpu().view(-1, pc.k).long()
    for op, pp in zip(pools, (prod.pool1, prod.pool2)):
        op.overrides = R.build_decisions(pp)
    B, N = 2, 200
    h = pos.double().reshape(-1, 3)
    for conv, pool in zip(convs[:2], pools):
        h = conv(h, torch.arange(B).repeat_interleave(N))
        h, N = pool(h, B, N)
    h = convs[2](h, torch.arange(B).repeat_interleave(N))
    ref = lin(O.global_max_pool(h, torch.arange(B).repeat_interleave(N), B))
    (ref * gy.double()).sum().backward()
    assert (out.detach().cpu().double() - ref.detach()).abs().max().item() < 1e-4 * max(1.0, ref.abs().max().item())
    pn = dict(prod.named_parameters())
    for n, p in holder.named_parameters():
        gerr = (pn[n].grad.cpu().double() - p.grad).abs().max().item() / (p.grad.abs().max().item() + 1e-12)
        assert gerr < 2e-3, (n, gerr)


def test_pooled_model_step_graph_replays_eager(gpe):
    from gpe_amd import configs, nets, optim, graph
    import bench
    dev = torch.device(DEV)
    data_config = configs.data_config()
    cfg = configs.lstm_model_config(k_neighbors=5, graph_pooling=True, pool_ratio=0.3)
    torch.manual_seed(0)
    model_a = nets.GarmentFullPattern3D(data_config, copy.deepcopy(cfg), copy.deepcopy(cfg['loss'])).to(dev).train()
    model_a.loss.with_quality_eval = False
    model_b = copy.deepcopy(model_a)
    feats, gt = bench.synthetic(4, 256, data_config, seed=1000, device=dev)
    opt_a = optim.FusedAdam(optim.FlatArena(model_a), lr=2e-3, schedule=optim.OneCycle(2e-3, 40))
    opt_b = optim.FusedAdam(optim.FlatArena(model_b), lr=2e-3, schedule=optim.OneCycle(2e-3, 40))
    nsteps = 5
    la = []
    for i in range(nsteps):
        torch.manual_seed(100 + i)
        loss = model_a.loss(model_a(feats), gt, epoch=0)[0]
        loss.backward()
        opt_a.step()
        la.append(loss.detach().clone())
    sg = graph.StepGraph(lambda f, g: model_b.loss(model_b(f), g, epoch=0)[0], opt_b, warmup=2)
    lb = []
    for i in range(nsteps):
        torch.manual_seed(100 + i)
        lb.append(sg.step(feats, gt).detach().clone())
    sg.synchronize()
    torch.cuda.synchronize()
    assert sg.captures == 1 and sg.replays == nsteps - 2
    for a, b in zip(la, lb):
        assert torch.equal(a, b)
    for (n, p), q in zip(model_a.named_parameters(), model_b.parameters()):
        assert torch.equal(p, q), n


def test_pool_gradients_reach_the_arena_hooks_and_the_checkpoint(gpe):
    """The pool's nine gradients are written by the kernel straight into the FlatArena and announced through mark_written, the hook
    DistributedHotPath launches its bucket all-reduces from (parallel.py _on_written); FusedAdam's torch.optim.Adam-format
    checkpoint then carries their moments and loads into torch.optim.Adam over the same model."""
    from gpe_amd import configs, nets, optim
    import bench
    dev = torch.device(DEV)
    data_config = configs.data_config()
    cfg = configs.lstm_model_config(k_neighbors=5, graph_pooling=True, pool_ratio=0.3)
    torch.manual_seed(0)
    model = nets.GarmentFullPattern3D(data_config, copy.deepcopy(cfg), copy.deepcopy(cfg['loss'])).to(dev).train()
    model.loss.with_quality_eval = False
    arena = optim.FlatArena(model)
    heard = []
    arena.listeners.append(heard.append)
    opt = optim.FusedAdam(arena, lr=1e-3)
    feats, gt = bench.synthetic(2, 256, data_config, seed=1000, device=dev)
    model.loss(model(feats), gt, epoch=0)[0].backward()
    torch.cuda.synchronize()
    pool_params = [p for n, p in model.named_parameters() if '.gpool_layers.' in n]
    assert len(pool_params) == 2 * 9
    for p in pool_params:
        i = arena.index[p.data_ptr()]
        assert i in heard and i in arena.written and p.grad.abs().sum().item() > 0
    opt.step()
    sd = opt.state_dict()
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    for j, n in enumerate(names):
        if '.gpool_layers.' in n:
            assert j in sd['state'] and sd['state'][j]['exp_avg_sq'].abs().sum().item() > 0, n
    ref = torch.optim.Adam(model.parameters(), lr=1e-3)
    ref.load_state_dict(sd)
    msd = model.state_dict()
    assert all(k in msd for k in ('feature_extractor.gpool_layers.0.edge_pool.att.weight',
                                  'feature_extractor.gpool_layers.1.edge_pool.gnn_score.lin2.weight'))

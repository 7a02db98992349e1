"""Drop-in for the reference's nn/net_blocks.py (classes resolved by name from the YAML config,
nn/nets.py:100,106,116).  The torch modules below only HOLD parameters/buffers under the reference's names
(`conv_layers.{i}.nn.{j}.{0,2}.*`, `lstm.weight_ih_l0`, `lin.*` ...); every forward/backward runs the HIP
kernels through ops.py."""
import torch
import torch.nn as nn

from . import ops
from . import streams


def MLP(channels, batch_norm=True):
    """Parameter container with the reference layout [Linear -> ReLU -> BatchNorm1d] x n, BN after ReLU and on
    the last layer too (nn/net_blocks.py:43-47; `batch_norm` is ignored there as well)."""
    return nn.Sequential(*[
        nn.Sequential(nn.Linear(channels[i - 1], channels[i]), nn.ReLU(), nn.BatchNorm1d(channels[i]))
        for i in range(1, len(channels))])


class DynamicEdgeConv(nn.Module):
    """Holder with PyG's attribute name `.nn` (state-dict compatibility); the arithmetic is ops.EdgeConvFn.
    aggr: 'max' (shipped), 'mean', 'add'; the edge MLP may have any number of blocks >= 2 (EConv_hidden_depth >= 1)."""

    def __init__(self, nn_module, k, aggr='max'):
        super().__init__()
        if aggr not in ('max', 'mean', 'add'):
            raise ValueError("unsupported aggregation '%s' (PyG MessagePassing accepts max / mean / add here)" % aggr)
        if len(nn_module) < 2:
            raise NotImplementedError('EConv_hidden_depth must be >= 1 (edge MLP of at least 2 blocks), got %d block(s)'
                                      % len(nn_module))
        self.nn = nn_module
        self.k = k
        self.aggr = aggr
        self.last_knn = None
        self.last_order = None                               # the locality order the last graph search worked in (int32 [B, N])
        self.half_act_guard = ops.HalfActGuard()             # f16x3: watches the fp16-stored activation (ops.set_half_act_guard)

    def register_packs(self, plan):
        blocks = [self.nn[i] for i in range(len(self.nn))]
        plan.add_edge_first(blocks[0][0].weight, blocks[0][0].bias)
        for b in blocks[1:]:
            plan.add_linear(b[0].weight, fwd=False, bwd=True)     # forward packs carry the folded BatchNorm scale

    def forward(self, x, n_clouds, n_points, order=None):
        """order: the previous EdgeConv layer's `last_order` (a speed hint for this layer's graph search; results do not depend on it)"""
        eps, mom, nb, args = ops.mlp_tensors(self.nn)
        H0 = self.nn[0][0].weight.shape[0]
        if H0 % 4 or H0 > 256:
            # a first-block width the fused P|Q kernels do not take: the general (explicit-message) formulation
            out, idx = ops.edge_conv_general(x, n_clouds, n_points, self.k, self.training, eps, mom, nb, self.aggr, args)
            self.last_order = None
        else:
            out, idx, self.last_order = ops.EdgeConvFn.apply(x, n_clouds, n_points, self.k, self.training, eps, mom, nb, self.aggr,
                                                             self.half_act_guard, order, *args)
        self.last_knn = idx
        return out

    def predict(self, x, n_clouds, n_points, order=None, route='auto'):
        """forward at prediction time (an addition to the reference's class surface): eval mode, nothing recorded for autograd, and
        on route 'fused' no per-edge tensor (ops.edge_conv_predict; 'layers' = the kernels of forward, 'auto' chooses).  Sets
        last_knn / last_order as forward does."""
        if route not in ops.EDGE_PREDICT_ROUTES:
            raise ValueError('unknown route %r (choose from %s)' % (route, ops.EDGE_PREDICT_ROUTES))
        if self.training:
            raise RuntimeError('DynamicEdgeConv.predict is a prediction path: call .eval() first (BatchNorm running statistics)')
        eps, mom, nb, args = ops.mlp_tensors(self.nn)
        H0 = self.nn[0][0].weight.shape[0]
        if H0 % 4 or H0 > 256:
            # a first-block width off the P|Q menu: the general formulation, as in forward
            if route == 'fused':
                raise ValueError("route='fused' needs a first-block width <= 256 that is a multiple of 4 (got %d)" % H0)
            with torch.no_grad():
                out, idx = ops.edge_conv_general(x.detach(), n_clouds, n_points, self.k, False, eps, mom, nb, self.aggr, args)
            self.last_order = None
        else:
            out, idx, self.last_order = ops.edge_conv_predict(x, n_clouds, n_points, self.k, nb, self.aggr, args, order=order,
                                                              route=route, eps=eps)
        self.last_knn = idx
        return out


class EdgeConvFeatures(nn.Module):
    """nn/net_blocks.py:93-191: defaults, 2x DynamicEdgeConv, optional skip concat, global pool, Linear.
    forward(positions [B,N,3], global_pool=True) -> (encoding [B,out] | None, per-point [B*N,F(+3)], batch)."""

    def __init__(self, out_size, config={}):
        super().__init__()
        self.config = {
            'conv_depth': 2, 'k_neighbors': 5, 'EConv_hidden': 200, 'EConv_hidden_depth': 2,
            'EConv_feature': 112, 'EConv_aggr': 'max', 'global_pool': 'mean',
            'skip_connections': False, 'graph_pooling': False, 'pool_ratio': 0.1}
        self.config.update(config)
        depth = self.config['conv_depth']
        pooling = self.config['graph_pooling']
        if pooling and self.config['skip_connections']:
            # the reference concatenates the pooled features with ALL input positions and fails inside torch.cat at the first forward
            raise ValueError('skip_connections cannot be combined with graph_pooling: the pooled clouds keep %s of the points '
                             'the skip connection would concatenate' % self.config['pool_ratio'])
        if pooling:
            # nn/net_blocks.py:113-118: widths grow towards the last layer when the clouds shrink
            feat = [int(self.config['EConv_feature'] / d) for d in range(depth, 0, -1)]
            hid = [int(self.config['EConv_hidden'] / d) for d in range(depth, 0, -1)]
        else:
            feat = [self.config['EConv_feature']] * depth
            hid = [self.config['EConv_hidden']] * depth
        mlp_depth = self.config['EConv_hidden_depth']
        self.conv_layers = nn.ModuleList()
        self.conv_layers.append(DynamicEdgeConv(
            MLP([2 * 3] + [hid[0]] * mlp_depth + [feat[0]]),
            k=self.config['k_neighbors'], aggr=self.config['EConv_aggr']))
        for c in range(1, depth):
            self.conv_layers.append(DynamicEdgeConv(
                MLP([2 * feat[c - 1]] + [hid[c]] * mlp_depth + [feat[c]]),
                k=self.config['k_neighbors'], aggr=self.config['EConv_aggr']))
        if pooling:
            # nn/net_blocks.py:138-142: one pool after every conv, the last one included
            self.gpool_layers = nn.ModuleList()
            for c in range(depth):
                self.gpool_layers.append(DynamicASAPool(feat[c], k=self.config['k_neighbors'],
                                                        pool_ratio=self.config['pool_ratio']))
        if self.config['global_pool'] == 'max':
            self.global_pool = ops.segment_max
        elif self.config['global_pool'] == 'mean':
            self.global_pool = ops.segment_mean
        elif self.config['global_pool'] == 'add':
            self.global_pool = ops.segment_add
        else:
            raise ValueError('{} pooling is not supported'.format(self.config['global_pool']))
        out_features = self.config['EConv_feature'] + 3 if self.config['skip_connections'] \
            else self.config['EConv_feature']
        self.lin = nn.Linear(out_features, out_size)

    def register_packs(self, plan):
        for conv in self.conv_layers:
            conv.register_packs(plan)
        plan.add_linear(self.lin.weight)

    def predict(self, positions, global_pool=True, want_batch=True, route='auto'):
        """forward at prediction time (an addition to the reference's class surface): the same triple, computed in eval mode without
        autograd records, every DynamicEdgeConv on its prediction path (route: DynamicEdgeConv.predict)."""
        if route not in ops.EDGE_PREDICT_ROUTES:
            raise ValueError('unknown route %r (choose from %s)' % (route, ops.EDGE_PREDICT_ROUTES))
        if self.training:
            raise RuntimeError('EdgeConvFeatures.predict is a prediction path: call .eval() first (BatchNorm running statistics)')
        with torch.no_grad():
            B, N = positions.size(0), positions.size(1)
            pos_flat = positions.reshape(-1, positions.size(-1))
            if pos_flat.dtype != torch.float32:
                pos_flat = pos_flat.float()
            pos_flat = pos_flat.contiguous()
            batch = torch.arange(B, device=positions.device).repeat_interleave(N) if want_batch else None
            out = pos_flat
            order = None
            if self.config['graph_pooling']:
                for conv, pool in zip(self.conv_layers, self.gpool_layers):
                    _check_cloud(conv.k, N)
                    out = conv.predict(out, B, N, order=order, route=route)
                    out, (_, N) = pool(out, (B, N), order=conv.last_order)      # (the pool's existing forward)
                if want_batch:
                    batch = torch.arange(B, device=positions.device).repeat_interleave(N)
            else:
                for conv in self.conv_layers:
                    out = conv.predict(out, B, N, order=order, route=route)
                    order = conv.last_order
            if self.config['skip_connections']:
                out = torch.cat([out, pos_flat], dim=-1)
            if global_pool:
                pooled = self.global_pool(out.contiguous() if out.stride(1) != 1 else out, B, N)
                return ops.linear(pooled, self.lin.weight, self.lin.bias), out, batch
            return None, out, batch

    def forward(self, positions, global_pool=True, want_batch=True):
        B, N = positions.size(0), positions.size(1)
        pos_flat = positions.reshape(-1, positions.size(-1))
        if pos_flat.dtype != torch.float32:
            pos_flat = pos_flat.float()
        pos_flat = pos_flat.contiguous()
        # batch vector of the reference (nn/net_blocks.py:165-167); the kernels only need (B, N)
        # (want_batch=False: a caller that only takes the pooled encoding — nets.GarmentFullPattern3D — saves the two launches)
        batch = torch.arange(B, device=positions.device).repeat_interleave(N) if want_batch else None
        out = pos_flat
        order = None                                         # layer l + 1 searches its graph in layer l's locality order
        if self.config['graph_pooling']:
            for conv, pool in zip(self.conv_layers, self.gpool_layers):
                _check_cloud(conv.k, N)
                out = conv(out, B, N, order=order)
                # the pool's search may take the conv's order (same numbering); the next conv may not (a foreign numbering)
                out, (_, N) = pool(out, (B, N), order=conv.last_order)
                order = None
            if want_batch:
                batch = torch.arange(B, device=positions.device).repeat_interleave(N)
        else:
            for conv in self.conv_layers:
                out = conv(out, B, N, order=order)
                order = conv.last_order
        if self.config['skip_connections']:
            out = torch.cat([out, pos_flat], dim=-1)
        if global_pool:
            pooled = self.global_pool(out.contiguous() if out.stride(1) != 1 else out, B, N)
            return ops.linear(pooled, self.lin.weight, self.lin.bias), out, batch
        return None, out, batch


def _check_cloud(k, N):
    if N < k:
        # torch_cluster would quietly hand out fewer neighbours; the fused kernels need k of them
        raise ValueError('a pooled cloud of %d points is smaller than k_neighbors = %d: raise pool_ratio or lower k_neighbors'
                         % (N, k))


class _LEConvHolder(nn.Module):
    """parameter container with PyG 2.x LEConv's names (gnn_score.lin1 / lin2 / lin3; lin2 has no bias)."""

    def __init__(self, F):
        super().__init__()
        self.lin1 = nn.Linear(F, 1)
        self.lin2 = nn.Linear(F, 1, bias=False)
        self.lin3 = nn.Linear(F, 1)


class _ASAPoolingHolder(nn.Module):
    """parameter container with PyG 2.x ASAPooling's names (lin, att, gnn_score); the arithmetic is ops.AsapPoolFn."""

    def __init__(self, F, ratio):
        super().__init__()
        self.in_channels = F
        self.ratio = ratio
        self.lin = nn.Linear(F, F)
        self.att = nn.Linear(2 * F, 1)
        self.gnn_score = _LEConvHolder(F)

    def params(self):
        g = self.gnn_score
        return [self.lin.weight, self.lin.bias, self.att.weight, self.att.bias, g.lin1.weight, g.lin1.bias, g.lin2.weight,
                g.lin3.weight, g.lin3.bias]


class DynamicASAPool(nn.Module):
    """nn/net_blocks.py:194-218: ASAPooling on the kNN graph of the node features, parameters under `edge_pool.*`.

    Restated exactly (csrc/gpe_asap.hip, include/gpe_hip.h gpe_asap_fwd): the graph always uses k = 10 neighbours (the `k`
    argument is ignored, as in the reference; min(10, N) for smaller clouds) and is not flipped, so a node pools from every node
    that has it among its neighbours.  Fixed here where upstream leaves it open: equal fitness keeps the lower index; equal channel
    maxima route the gradient to the lowest-numbered source.  The parameters are drawn with torch.nn.Linear's initialisation in
    PyG 2.x's registration order (lin, att, gnn_score.lin1/2/3); same-seed equality with a model built by PyG itself is not
    claimed (its draw order depends on the version).

    forward(node_features [B*N, F], batch) -> (out [B*M, F], new_batch), M = ceil(fp32(pool_ratio) * N) per cloud.  batch is
    either the reference's LongTensor (clouds of equal size; B is read from it on the host once — a synchronising read) or a pair
    (B, N), in which case new_batch is the pair (B, M) and nothing is read back."""

    def __init__(self, feature_size, k=10, pool_ratio=0.5):
        super().__init__()
        self.k = ops.ASAP_K
        self.edge_pool = _ASAPoolingHolder(feature_size, pool_ratio)
        self.keep_decisions = False      # True: `last` receives the graph, kept rows, winners and fitness of every forward (tests)
        self.last = {}

    def forward(self, node_features, batch, order=None):
        if isinstance(batch, torch.Tensor):
            B = int(batch[-1].item()) + 1 if batch.numel() else 0
            N = node_features.shape[0] // max(B, 1)
            if B * N != node_features.shape[0]:
                raise ValueError('DynamicASAPool takes clouds of equal size (%d rows, %d clouds)' % (node_features.shape[0], B))
        else:
            B, N = batch
        x = node_features if node_features.dtype == torch.float32 else node_features.float()
        self.last = {}
        out, M = ops.asap_pool(x, B, N, self.edge_pool.params(), self.edge_pool.ratio, order=order,
                               trace=self.last if self.keep_decisions else None)
        if isinstance(batch, torch.Tensor):
            return out, torch.arange(B, device=batch.device).repeat_interleave(M)
        return out, (B, M)


class EdgeConvPoolingFeatures(nn.Module):
    """nn/net_blocks.py:221-268: conv1 -> pool1 -> conv2 -> pool2 -> conv3 -> global max pool -> Linear; forward(positions
    [B, N, 3]) -> [B, out_size].  Defaults n_features 32 / 128 / 256, k = 10; both pools keep half of the points."""

    def __init__(self, out_size, config={}):
        super().__init__()
        self.config = {'conv_depth': 3}
        self.config.update(n_features1=32, n_features2=128, n_features3=256, k=10)
        self.config.update(config)
        c = self.config
        self.conv1 = DynamicEdgeConv(MLP([2 * 3, 64, 64, c['n_features1']]), k=c['k'], aggr='max')
        self.pool1 = DynamicASAPool(c['n_features1'], k=c['k'])
        self.conv2 = DynamicEdgeConv(MLP([2 * c['n_features1'], c['n_features2'], c['n_features2'], c['n_features2']]),
                                     k=c['k'], aggr='max')
        self.pool2 = DynamicASAPool(c['n_features2'], k=c['k'])
        self.conv3 = DynamicEdgeConv(MLP([2 * c['n_features2'], c['n_features3'], c['n_features3'], c['n_features3']]),
                                     k=c['k'], aggr='max')
        self.lin = nn.Linear(c['n_features3'], out_size)

    def register_packs(self, plan):
        for conv in (self.conv1, self.conv2, self.conv3):
            conv.register_packs(plan)
        plan.add_linear(self.lin.weight)

    def forward(self, positions):
        B, N = positions.size(0), positions.size(1)
        out = positions.reshape(-1, positions.size(-1)).float().contiguous()
        for conv, pool in ((self.conv1, self.pool1), (self.conv2, self.pool2)):
            _check_cloud(conv.k, N)
            out = conv(out, B, N)
            out, (_, N) = pool(out, (B, N), order=conv.last_order)
        _check_cloud(self.conv3.k, N)
        out = self.conv3(out, B, N)
        return ops.linear(ops.segment_max(out, B, N), self.lin.weight, self.lin.bias)


class _PointConvHolder(nn.Module):
    """parameter container with PyG PointConv's attribute names (state-dict keys `conv.local_nn.*`)."""

    def __init__(self, local_nn):
        super().__init__()
        self.local_nn = local_nn
        self.global_nn = None


class _SetAbstractionModule(nn.Module):
    """nn/net_blocks.py:10-27: fps -> ball query (<= 25 neighbours) -> PointConv(MLP) with max aggregation, with PyG's defaults:
    fps(random_start=True) — the start points are drawn from torch's CPU generator (ops.fps_start; `fps_start` overrides) — and
    PointConv(add_self_loops=True), whose re-indexing of the bipartite edge list is restated in csrc/gpe_pointnet.hip."""

    def __init__(self, ratio, conv_radius, per_point_nn):
        super().__init__()
        self.ratio = ratio
        self.radius = conv_radius
        self.conv = _PointConvHolder(per_point_nn)
        self.fps_start = None              # int32 [B] tensor: fixed start points instead of the random draw
        self.add_self_loops = True         # PyG PointNetConv's default
        self.last = {}

    def forward(self, features, pos_flat, B, N):
        import math
        M = int(math.ceil(self.ratio * N))
        start = self.fps_start.to(pos_flat.device) if self.fps_start is not None else ops.fps_start(B, N, pos_flat.device)
        idx = ops.fps(pos_flat, B, N, M, start)
        nbr, cnt = ops.radius_neighbors(pos_flat, idx, B, N, self.radius, 25)
        ecnt, drop = ops.pointconv_self_loops(nbr, cnt, B, N, M) if self.add_self_loops else (cnt, None)
        off = torch.zeros(B * M + 1, device=pos_flat.device, dtype=torch.int64)
        torch.cumsum(ecnt, 0, out=off[1:])
        n_edges = int(off[-1].item())          # ragged edge list: the one host sync of this block (sizes the MLP rows)
        msg, seg = ops.ball_messages(pos_flat, features, idx, nbr, off, n_edges, B, N, drop)
        h = ops.dense_mlp(msg, self.conv.local_nn, self.training)
        out = ops.RaggedMaxFn.apply(h, off, seg, B * M)
        gidx = (idx.long() + (torch.arange(B, device=idx.device) * N)[:, None]).view(-1)
        self.last = {'idx': idx, 'nbr': nbr, 'cnt': cnt, 'edge_cnt': ecnt, 'drop': drop, 'seg': seg}
        return out, pos_flat[gidx], M


class _GlobalSetAbstractionModule(nn.Module):
    """nn/net_blocks.py:30-42: MLP on [features | pos] -> global max pool."""

    def __init__(self, per_point_net):
        super().__init__()
        self.nn = per_point_net

    def forward(self, features, pos, B, M):
        feats = torch.cat([features, pos], dim=1) if features is not None else pos
        return ops.segment_max(ops.dense_mlp(feats, self.nn, self.training), B, M)


class PointNetPlusPlus(nn.Module):
    """nn/net_blocks.py:50-88 (one set-abstraction level + the global level, as in the reference).  forward(positions [B,N,3])
    -> [B, out_size].  PyG's conventions (random fps start from torch's generator, PointConv's add_self_loops re-indexing) are
    restated in csrc/gpe_pointnet.hip; the two implementation-defined choices left (argmax ties, which neighbours survive the
    cap of 25) are fixed there for oracle and kernels alike."""

    def __init__(self, out_size, config={}):
        super().__init__()
        self.config = {'r1': 0.3, 'r2': 0.4, 'r3': 5, 'r4': 7}
        self.config.update(config)
        H, F = self.config['EConv_hidden'], self.config['EConv_feature']
        self.sa1_module = _SetAbstractionModule(0.2, self.config['r1'], MLP([3, H, H, F]))
        self.sa_last_module = _GlobalSetAbstractionModule(MLP([3 + F, H, H, F]))
        self.lin = nn.Linear(F, out_size)

    def forward(self, positions):
        B, N = positions.size(0), positions.size(1)
        pos_flat = positions.reshape(-1, positions.size(-1)).float().contiguous()
        feats, cpos, M = self.sa1_module(None, pos_flat, B, N)
        pooled = self.sa_last_module(feats, cpos, B, M)
        return ops.linear(pooled, self.lin.weight, self.lin.bias)


class _StateUploader(streams.Uploader):
    """Host-drawn tensors reach the GPU without draining the compute stream.

    The reference draws the LSTM start states on the CPU generator inside forward() (nn/net_blocks.py:391-392) and
    moves them with `.to(device)`.  From pageable memory that copy is stream-ordered AND blocks the host until it has
    run, i.e. until the whole encoder queued in front of it has finished — the GPU then idles while the host catches
    up (measured: 0.85 ms in front of each decoder, profiles/r01_e_gap_trace.md).  Here the draw lands in a pinned
    staging buffer (one per shape), the copy runs on a side stream, and the compute stream only waits on its event."""
    _per_device = {}

    @classmethod
    def get(cls, device):
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in cls._per_device:
            cls._per_device[key] = cls(device)
        return cls._per_device[key]


def _init_tenzor(*shape, device='cpu', init_type=''):
    """nn/net_blocks.py:302-315 — drawn on the CPU generator, then moved (keeps the reference's RNG stream)."""
    device = torch.device(device)
    zeros = not init_type or len(shape) == 1
    if not zeros and 'kaiming_normal' not in init_type:
        raise NotImplementedError('{} tenzor initialization is not implemented'.format(init_type))
    if zeros:
        return torch.zeros(shape, device=device)
    if device.type != 'cuda':
        t = torch.empty(shape)
        nn.init.kaiming_normal_(t)
        return t.to(device)
    if ops.HOST_DRAWN is not None:
        # a step driven by graph.StepGraph: a static device buffer, refilled from the same generator in front of every replay
        return ops.HOST_DRAWN.get(tuple(shape), nn.init.kaiming_normal_)
    # (same generator, same element order as torch.empty(shape))
    return _StateUploader.get(device).upload(tuple(shape), torch.Size(shape), nn.init.kaiming_normal_)


def _init_weights(module, init_type=''):
    """nn/net_blocks.py:318-333."""
    if not init_type:
        return
    for name, param in module.named_parameters():
        if 'weight' in name:
            if 'kaiming_normal' in init_type:
                if len(param.shape) > 1:
                    nn.init.kaiming_normal_(param)
            else:
                raise NotImplementedError('{} weight initialization is not implemented'.format(init_type))


def _rnn_params(rnn, n_layers):
    """the parameters of an nn.LSTM / nn.GRU as ops.rnn_stack takes them: flat, ops.RNN_PARAMS per layer (ops.rnn_layers is the inverse)"""
    return [getattr(rnn, '%s_l%d' % (name, l)) for l in range(n_layers) for name in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]


def _register_rnn_packs(plan, rnn, n_layers, hidden, gates):
    for l, ly in enumerate(ops.rnn_layers(_rnn_params(rnn, n_layers), n_layers)):
        plan.add_linear(ly.w_ih)
        plan.add_gates(ly.w_hh, hidden, gates)
        plan.add_linear(ly.w_hh, fwd=False, bwd=True)
        if l > 0:
            plan.add_gates(ly.w_ih, hidden, gates)     # layers > 0 project h_{l-1,t} inside the fused cell launch
        if gates == 4:
            plan.add_bias_sum(ly.b_ih, ly.b_hh)
        else:
            plan.add_gru_bias(ly.b_ih, ly.b_hh, hidden)


class LSTMEncoderModule(nn.Module):
    """nn/net_blocks.py:336-360: sequence -> final hidden state of the last LSTM layer."""

    def __init__(self, elem_len, encoding_size, n_layers, dropout=0, custom_init='kaiming_normal'):
        super().__init__()
        self.dropout = float(dropout)
        self.custom_init = custom_init
        self.n_layers = n_layers
        self.encoding_size = encoding_size
        self.lstm = nn.LSTM(elem_len, encoding_size, n_layers, dropout=dropout, batch_first=True)
        _init_weights(self.lstm, init_type=custom_init)

    def register_packs(self, plan):
        _register_rnn_packs(plan, self.lstm, self.n_layers, self.encoding_size, 4)

    def forward(self, batch_sequence):
        device = batch_sequence.device
        bs = batch_sequence.size(0)
        h0 = _init_tenzor(self.n_layers, bs, self.encoding_size, device=device, init_type=self.custom_init)
        c0 = _init_tenzor(self.n_layers, bs, self.encoding_size, device=device, init_type=self.custom_init)
        seq = batch_sequence if batch_sequence.stride(-1) == 1 else batch_sequence.contiguous()
        _, hN, _ = ops.rnn_stack(seq, h0, c0, seq.size(1), self.n_layers, 'lstm', _rnn_params(self.lstm, self.n_layers),
                                 want_state=True, dropout=self.dropout, training=self.training, h0_bounded=True)
        return hN[-1]


class LSTMDecoderModule(nn.Module):
    """nn/net_blocks.py:363-402.  `self.lstm` is a torch.nn.LSTM used ONLY as the parameter container
    (weight_ih_l*, weight_hh_l*, bias_ih_l*, bias_hh_l*); the recurrence runs in ops.RNNStackFn."""

    def __init__(self, encoding_size, hidden_size, out_elem_size, n_layers, dropout=0,
                 custom_init='kaiming_normal', **kwargs):
        super().__init__()
        self.dropout = float(dropout)
        self.custom_init = custom_init
        self.n_layers = n_layers
        self.encoding_size = encoding_size
        self.hidden_size = hidden_size
        self.out_elem_size = out_elem_size
        self.lstm = nn.LSTM(encoding_size, hidden_size, n_layers, dropout=dropout, batch_first=True)
        self.lin = nn.Linear(hidden_size, out_elem_size)
        _init_weights(self.lstm, init_type=custom_init)
        self.last_states = None

    def register_packs(self, plan):
        _register_rnn_packs(plan, self.lstm, self.n_layers, self.hidden_size, 4)
        plan.add_linear(self.lin.weight)

    def forward(self, batch_enc, out_len):
        device = batch_enc.device
        bs = batch_enc.size(0)
        # hidden first, then cell: the reference's draw order (nn/net_blocks.py:391-392)
        h0 = _init_tenzor(self.n_layers, bs, self.hidden_size, device=device, init_type=self.custom_init)
        c0 = _init_tenzor(self.n_layers, bs, self.hidden_size, device=device, init_type=self.custom_init)
        self.last_states = (h0, c0)
        enc = batch_enc if batch_enc.is_contiguous() else batch_enc.contiguous()
        top, _, _ = ops.rnn_stack(enc, h0, c0, out_len, self.n_layers, 'lstm', _rnn_params(self.lstm, self.n_layers),
                                  dropout=self.dropout, training=self.training, h0_bounded=True)
        return ops.linear(top, self.lin.weight, self.lin.bias).view(bs, out_len, -1)


class LSTMDoubleReverseDecoderModule(nn.Module):
    """nn/net_blocks.py:405-454: decode the sequence in reverse order, then refine it with a second LSTM that reads
    [flipped first pass | encoding] and starts from the first LSTM's final state."""

    def __init__(self, encoding_size, hidden_size, out_elem_size, n_layers, dropout=0,
                 custom_init='kaiming_normal', **kwargs):
        super().__init__()
        self.dropout = float(dropout)
        self.custom_init = custom_init
        self.n_layers = n_layers
        self.encoding_size = encoding_size
        self.hidden_size = hidden_size
        self.out_elem_size = out_elem_size
        self.lstm_reverse = nn.LSTM(encoding_size, hidden_size, n_layers, dropout=dropout, batch_first=True)
        self.lstm_forward = nn.LSTM(hidden_size + encoding_size, hidden_size, n_layers, dropout=dropout,
                                    batch_first=True)
        self.lin = nn.Linear(hidden_size, out_elem_size)
        _init_weights(self.lstm_reverse, init_type=custom_init)
        _init_weights(self.lstm_forward, init_type=custom_init)
        self.last_states = None

    def register_packs(self, plan):
        _register_rnn_packs(plan, self.lstm_reverse, self.n_layers, self.hidden_size, 4)
        _register_rnn_packs(plan, self.lstm_forward, self.n_layers, self.hidden_size, 4)
        plan.add_linear(self.lin.weight)

    def forward(self, batch_enc, out_len):
        device = batch_enc.device
        bs = batch_enc.size(0)
        h0 = _init_tenzor(self.n_layers, bs, self.hidden_size, device=device, init_type=self.custom_init)
        c0 = _init_tenzor(self.n_layers, bs, self.hidden_size, device=device, init_type=self.custom_init)
        self.last_states = (h0, c0)
        enc = batch_enc if batch_enc.is_contiguous() else batch_enc.contiguous()
        out, hN, cN = ops.rnn_stack(enc, h0, c0, out_len, self.n_layers, 'lstm',
                                    _rnn_params(self.lstm_reverse, self.n_layers), want_state=True,
                                    dropout=self.dropout, training=self.training, h0_bounded=True)
        dec_input = enc.unsqueeze(1).expand(-1, out_len, -1)
        seq = torch.cat([torch.flip(out, [1]), dec_input], -1)            # skip connection with the original input
        top, _, _ = ops.rnn_stack(seq, hN, cN, out_len, self.n_layers, 'lstm',
                                  _rnn_params(self.lstm_forward, self.n_layers), dropout=self.dropout,
                                  training=self.training, h0_bounded=True)      # (states of the first LSTM: |h| < 1)
        return ops.linear(top, self.lin.weight, self.lin.bias).view(bs, out_len, -1)


class GRUDecoderModule(nn.Module):
    """nn/net_blocks.py:457-497; `self.recurrent_cell` is the parameter container, ops.RNNStackFn the arithmetic."""

    def __init__(self, encoding_size, hidden_size, out_elem_size, n_layers, dropout=0,
                 custom_init='kaiming_normal', **kwargs):
        super().__init__()
        self.dropout = float(dropout)
        self.custom_init = custom_init
        self.n_layers = n_layers
        self.encoding_size = encoding_size
        self.hidden_size = hidden_size
        self.out_elem_size = out_elem_size
        self.recurrent_cell = nn.GRU(encoding_size, hidden_size, n_layers, dropout=dropout, batch_first=True)
        self.lin = nn.Linear(hidden_size, out_elem_size)
        _init_weights(self.recurrent_cell, init_type=custom_init)
        self.last_states = None

    def register_packs(self, plan):
        _register_rnn_packs(plan, self.recurrent_cell, self.n_layers, self.hidden_size, 3)
        plan.add_linear(self.lin.weight)

    def forward(self, batch_enc, out_len):
        device = batch_enc.device
        bs = batch_enc.size(0)
        h0 = _init_tenzor(self.n_layers, bs, self.hidden_size, device=device, init_type=self.custom_init)
        self.last_states = (h0,)
        enc = batch_enc if batch_enc.is_contiguous() else batch_enc.contiguous()
        top, _, _ = ops.rnn_stack(enc, h0, None, out_len, self.n_layers, 'gru',
                                  _rnn_params(self.recurrent_cell, self.n_layers), dropout=self.dropout,
                                  training=self.training, h0_bounded=True)
        return ops.linear(top, self.lin.weight, self.lin.bias).view(bs, out_len, -1)


class MLPDecoder(nn.Module):
    """nn/net_blocks.py:273-298: latent code -> MLP([enc, hid*out_len x n_layers, out_elem*out_len]) -> [B, out_len, out_elem].
    The arithmetic is ops.DenseMLPFn (wide layers run as several column blocks of the row GEMM)."""

    def __init__(self, encoding_size, hidden_size, out_elem_size, n_layers, out_len=1, dropout=0,
                 custom_init='kaiming_normal'):
        super().__init__()
        self.out_len = out_len
        self.mlp = MLP([encoding_size] + [hidden_size * out_len for _ in range(n_layers)] + [out_elem_size * out_len])
        _init_weights(self.mlp, init_type=custom_init)

    def register_packs(self, plan):
        blocks = [self.mlp[i] for i in range(len(self.mlp))]
        plan.add_linear(blocks[0][0].weight)                      # first block: nothing folded in
        for b in blocks[1:]:
            plan.add_linear(b[0].weight, fwd=False, bwd=True)

    def forward(self, batch_enc, *args):
        batch_size = batch_enc.size(0)
        out = ops.dense_mlp(batch_enc, self.mlp, self.training)
        return out.contiguous().view(batch_size, self.out_len, -1)


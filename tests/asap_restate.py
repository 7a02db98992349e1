"""Test infrastructure: an fp64 restatement of DynamicASAPool (nn/net_blocks.py:194-218 = PyG 2.x ASAPooling on knn(x, x, 10))
and of EdgeConvFeatures with graph_pooling (nn/net_blocks.py:113-118, 138-142, 172-176), written from the published definitions
with plain torch ops (autograd gives the gradients).

Three decisions of the pool are discontinuous, like the kNN graph and the ReLU masks of tests/relu_align.py: the pool's own kNN
graph (a distance tie in feature space), the winner of each channel max of the query branch (two sources within rounding of each
other) and the kept set / order of topk (two fitness values within rounding).  `asap_pool` takes the build's choice for each of
them as an override and reports in `info` how far the restatement's own choice is from it:
  info['winner_gap']  largest |x[own winner] - x[build's winner]| of a channel max (0 when the build's winners are the maxima)
  info['perm_gap']    largest fitness difference between the build's kept row and the restatement's own at any output slot
  info['perm_margin'] smallest fitness gap between neighbouring ranks up to the last kept one, per cloud (how close the
                      restatement's own choice is to a tie)
"""
import numpy as np
import torch
import torch.nn as nn

from oracle import ref_path as O

K = 10


def pool_count(N, ratio):
    """PyG topk: ceil(float(ratio) * N) with N as float32 (the fitness dtype), i.e. in fp32; a ratio >= 1 is a count."""
    if ratio >= 1:
        return min(int(ratio), N)
    return int(np.ceil(np.float32(ratio) * np.float32(N)))


def pool_graph(x, B, N):
    """The pool's kNN graph: LongTensor [B*N, min(10, N)] local indices (oracle.ref_path.knn_local: fp32 distances, ties to the
    lower index, as torch_cluster.knn)."""
    return O.knn_local(x.detach(), B, min(K, N))


def _edges(knn, B, N):
    """ASAPooling's edge list after add_remaining_self_loops: (src, dst) global rows, src = query q, dst = its neighbour c
    (torch_cluster's [query, neighbour] rows are not flipped), q == c dropped, one self-loop per node appended."""
    k = knn.shape[1]
    q = torch.arange(B * N).repeat_interleave(k)
    c = (knn + (torch.arange(B * N) // N * N)[:, None]).reshape(-1)
    keep = q != c
    loops = torch.arange(B * N)
    return torch.cat([q[keep], loops]), torch.cat([c[keep], loops])


def _scatter_add(v, idx, n):
    out = torch.zeros((n,) + tuple(v.shape[1:]), dtype=v.dtype)
    return out.index_add(0, idx, v)


def _edges_from_index(edge_index, BN):
    """add_remaining_self_loops on a general edge_index (messages flow from row 0 to row 1, as in PyG's MessagePassing)."""
    src, dst = edge_index[0].long(), edge_index[1].long()
    keep = src != dst
    loops = torch.arange(BN)
    return torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])


def asap_pool(x, B, N, params, ratio, knn=None, winners=None, perm=None, info=None, edge_index=None):
    """x [B*N, F] (fp64, may require grad); params: [lin.weight, lin.bias, att.weight, att.bias, gnn_score.lin1.weight, lin1.bias,
    lin2.weight, lin3.weight, lin3.bias].  Overrides: knn LongTensor [B*N, k] local; winners LongTensor [B*N, F] of GLOBAL source
    rows of each channel max; perm LongTensor [B*M] of kept GLOBAL rows.  edge_index (instead of knn): any [2, E] graph of GLOBAL
    rows in PyG's orientation (source row 0, target row 1), as ASAPooling receives it.  -> (out [B*M, F], perm [B*M])."""
    w_lin, b_lin, w_att, b_att, w1, b1, w2, w3, b3 = params
    BN, F = x.shape
    info = {} if info is None else info
    if edge_index is not None:
        info['knn'] = None
        src, dst = _edges_from_index(edge_index, BN)
    else:
        if knn is None:
            knn = pool_graph(x, B, N)
        info['knn'] = knn
        src, dst = _edges(knn, B, N)
    xs = x[src]
    # query branch: channel max over each cluster, lowest source index on ties
    with torch.no_grad():
        mx = torch.full((BN, F), float('-inf'), dtype=x.dtype).scatter_reduce(0, dst[:, None].expand(-1, F), xs, 'amax')
        big = torch.full_like(xs, BN, dtype=torch.long)
        cand = torch.where(xs == mx[dst], src[:, None].expand(-1, F), big)
        own = torch.full((BN, F), BN, dtype=torch.long).scatter_reduce(0, dst[:, None].expand(-1, F), cand, 'amin')
    if winners is None:
        winners = own
    winners = winners.long()
    info['own_winners'] = own
    info['winners'] = winners
    xq = torch.gather(x, 0, winners)
    info['winner_gap'] = (xq.detach() - mx).abs().max().item()
    xq = xq @ w_lin.t() + b_lin
    score = torch.cat([xq[dst], xs], dim=-1) @ w_att.t() + b_att
    score = torch.nn.functional.leaky_relu(score.view(-1), 0.2)
    smax = torch.full((BN,), float('-inf'), dtype=x.dtype).scatter_reduce(0, dst, score.detach(), 'amax')
    ex = (score - smax[dst]).exp()
    alpha = ex / (_scatter_add(ex, dst, BN) + 1e-16)[dst]
    xp = _scatter_add(xs * alpha[:, None], dst, BN)
    # LEConv fitness on the same graph: sum_j lin1(x'_j) - deg * lin2(x'_i) + lin3(x'_i)
    a = (xp @ w1.t() + b1).view(-1)
    bb = (xp @ w2.t()).view(-1)
    pre = _scatter_add(a[src] - bb[dst], dst, BN) + (xp @ w3.t() + b3).view(-1)
    fit = torch.sigmoid(pre)
    M = pool_count(N, ratio)
    f = fit.detach().view(B, N)
    own_perm, margin = [], float('inf')
    for b in range(B):
        order = sorted(range(N), key=lambda i: (-f[b, i].item(), i))
        own_perm += [b * N + i for i in order[:M]]
        vals = [f[b, i].item() for i in order[:min(M + 1, N)]]
        if len(vals) > 1:
            margin = min(margin, min(vals[i] - vals[i + 1] for i in range(len(vals) - 1)))
    own_perm = torch.tensor(own_perm, dtype=torch.long)
    info['own_perm'] = own_perm
    info['perm_margin'] = margin
    if perm is None:
        perm = own_perm
    perm = perm.long()
    info['perm'] = perm
    info['perm_gap'] = (fit.detach()[perm] - fit.detach()[own_perm]).abs().max().item()
    info['fitness'] = fit.detach()
    return xp[perm] * fit[perm][:, None], perm


class _LEConv(nn.Module):
    def __init__(self, F):
        super().__init__()
        self.lin1 = nn.Linear(F, 1)
        self.lin2 = nn.Linear(F, 1, bias=False)
        self.lin3 = nn.Linear(F, 1)


class _ASAPooling(nn.Module):
    def __init__(self, F, ratio):
        super().__init__()
        self.ratio = ratio
        self.lin = nn.Linear(F, F)
        self.att = nn.Linear(2 * F, 1)
        self.gnn_score = _LEConv(F)

    def params(self):
        g = self.gnn_score
        return [self.lin.weight, self.lin.bias, self.att.weight, self.att.bias, g.lin1.weight, g.lin1.bias, g.lin2.weight,
                g.lin3.weight, g.lin3.bias]


class DynamicASAPool(nn.Module):
    """nn/net_blocks.py:194-218 in fp64; `overrides` (dict with any of knn / winners / perm) pins the next forward's decisions,
    `info` holds what the last forward decided and the gaps."""

    def __init__(self, feature_size, k=10, pool_ratio=0.5):
        super().__init__()
        self.k = K
        self.edge_pool = _ASAPooling(feature_size, pool_ratio)
        self.overrides = {}
        self.info = {}

    def forward(self, x, B, N):
        self.info = {}
        out, perm = asap_pool(x, B, N, self.edge_pool.params(), self.edge_pool.ratio, info=self.info, **self.overrides)
        return out, pool_count(N, self.edge_pool.ratio)


class PooledEdgeConvFeatures(nn.Module):
    """EdgeConvFeatures with graph_pooling: True (oracle.ref_path.EdgeConvFeatures raises for it), composed from
    oracle.ref_path.DynamicEdgeConv + MLP and the pool above.  Same state-dict keys as the reference."""

    def __init__(self, out_size, config={}):
        super().__init__()
        self.config = {'conv_depth': 2, 'k_neighbors': 5, 'EConv_hidden': 200, 'EConv_hidden_depth': 2, 'EConv_feature': 112,
                       'EConv_aggr': 'max', 'global_pool': 'mean', 'skip_connections': False, 'graph_pooling': True,
                       'pool_ratio': 0.1}
        self.config.update(config)
        c = self.config
        depth = c['conv_depth']
        feat = [int(c['EConv_feature'] / d) for d in range(depth, 0, -1)]
        hid = [int(c['EConv_hidden'] / d) for d in range(depth, 0, -1)]
        md = c['EConv_hidden_depth']
        self.conv_layers = nn.ModuleList([O.DynamicEdgeConv(O.MLP([2 * 3] + [hid[0]] * md + [feat[0]]), k=c['k_neighbors'],
                                                            aggr=c['EConv_aggr'])])
        for i in range(1, depth):
            self.conv_layers.append(O.DynamicEdgeConv(O.MLP([2 * feat[i - 1]] + [hid[i]] * md + [feat[i]]), k=c['k_neighbors'],
                                                      aggr=c['EConv_aggr']))
        self.gpool_layers = nn.ModuleList([DynamicASAPool(feat[i], k=c['k_neighbors'], pool_ratio=c['pool_ratio'])
                                           for i in range(depth)])
        self.global_pool = {'max': O.global_max_pool, 'mean': O.global_mean_pool, 'add': O.global_add_pool}[c['global_pool']]
        self.lin = nn.Linear(c['EConv_feature'], out_size)

    def forward(self, positions, global_pool=True):
        B, N = positions.size(0), positions.size(1)
        out = positions.reshape(-1, positions.size(-1))
        for conv, pool in zip(self.conv_layers, self.gpool_layers):
            out = conv(out, torch.arange(B).repeat_interleave(N))
            out, N = pool(out, B, N)
        batch = torch.arange(B).repeat_interleave(N)
        if global_pool:
            return self.lin(self.global_pool(out, batch, B)), out, batch
        return None, out, batch


class PoolingFeatures(nn.Module):
    """EdgeConvPoolingFeatures (nn/net_blocks.py:221-268) in fp64: conv1 -> pool1 -> conv2 -> pool2 -> conv3 -> global max -> lin,
    from oracle.ref_path.DynamicEdgeConv + MLP and the pool above; same state-dict keys as the reference."""

    def __init__(self, out_size, config={}):
        super().__init__()
        self.config = {'conv_depth': 3}
        self.config.update(n_features1=32, n_features2=128, n_features3=256, k=10)
        self.config.update(config)
        c = self.config
        self.conv1 = O.DynamicEdgeConv(O.MLP([2 * 3, 64, 64, c['n_features1']]), k=c['k'], aggr='max')
        self.pool1 = DynamicASAPool(c['n_features1'], k=c['k'])
        self.conv2 = O.DynamicEdgeConv(O.MLP([2 * c['n_features1']] + [c['n_features2']] * 3), k=c['k'], aggr='max')
        self.pool2 = DynamicASAPool(c['n_features2'], k=c['k'])
        self.conv3 = O.DynamicEdgeConv(O.MLP([2 * c['n_features2']] + [c['n_features3']] * 3), k=c['k'], aggr='max')
        self.lin = nn.Linear(c['n_features3'], out_size)

    def forward(self, positions):
        B, N = positions.size(0), positions.size(1)
        out = positions.reshape(-1, positions.size(-1))
        for conv, pool in ((self.conv1, self.pool1), (self.conv2, self.pool2)):
            out = conv(out, torch.arange(B).repeat_interleave(N))
            out, N = pool(out, B, N)
        batch = torch.arange(B).repeat_interleave(N)
        out = self.conv3(out, batch)
        return self.lin(O.global_max_pool(out, batch, B))


def pin_to_build(oracle_enc, prod_enc):
    """Give the fp64 composition the build's decisions of the last forward: every conv's kNN graph and every pool's graph, winners
    and kept rows (net_blocks.DynamicASAPool keeps them in `.last`; the winners are read from the kernel state)."""
    for oc, pc in zip(oracle_enc.conv_layers, prod_enc.conv_layers):
        oc.knn_override = pc.last_knn.cpu().view(-1, pc.k).long()
    for op, pp in zip(oracle_enc.gpool_layers, prod_enc.gpool_layers):
        op.overrides = build_decisions(pp)


def build_decisions(pool):
    """{knn, winners, perm} of a net_blocks.DynamicASAPool's last forward, as LongTensors on the CPU."""
    last = pool.last
    k = last['knn'].shape[-1]
    return {'knn': last['knn'].cpu().view(-1, k).long(), 'winners': last['winners'].cpu().long(),
            'perm': last['perm'].cpu().long()}

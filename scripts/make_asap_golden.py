#!/usr/bin/env python3
"""Generates tests/golden/asap_*.pt: what the REFERENCE'S OWN EdgeConvFeatures(graph_pooling=True), DynamicASAPool and
EdgeConvPoolingFeatures (nn/net_blocks.py:93-268) compute, in fp64, on small clouds.

Only runnable where the reference checkout exists (like oracle/refgen/make_golden.py, whose stubs it puts on sys.path read-only).
PyG is not installed: the stub module torch_geometric.nn gets, at run time, a `knn` with torch_cluster's output layout
([query, neighbour] rows, min(k, N) neighbours per point: oracle.ref_path.knn_local) and an `ASAPooling` that takes whatever
edge_index the reference hands it in PyG's orientation (messages from row 0 to row 1) and evaluates tests/asap_restate.py on it.
Everything else — widths, where the pools sit, the k the pool asks for, that the graph is not flipped, the global pool on the
pooled batch, state-dict keys and shapes, output and batch shapes — is the reference's code.  The fixtures hold data only:
configs, the k of every knn call, inputs, state dicts, outputs.  Seeded: a re-run writes the same files.

    python scripts/make_asap_golden.py [REFERENCE_DIR]
"""
import os
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('GPE_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(REPO, 'oracle', 'refgen', 'stubs'), os.path.join(REF, 'nn'), REPO, os.path.join(REPO, 'tests')]

import torch_geometric.nn as stub_nn  # noqa: E402  (the stub package of oracle/refgen)
from oracle import ref_path as O  # noqa: E402
import asap_restate as R  # noqa: E402

KNN_CALLS = []


def knn(x, y, k, batch_x=None, batch_y=None):
    """torch_cluster.knn(x, y, k, batch_x, batch_y) for x is y: edge_index [2, B*N*min(k, N)], row 0 = query, row 1 = neighbour."""
    assert x is y or torch.equal(x, y)
    B = int(batch_x.max()) + 1
    N = x.shape[0] // B
    kk = min(k, N)
    KNN_CALLS.append({'k': k, 'n_points': N, 'neighbours': kk})
    local = O.knn_local(x.detach(), B, kk)
    row = torch.arange(B * N).repeat_interleave(kk)
    col = (local + (torch.arange(B * N) // N * N)[:, None]).reshape(-1)
    return torch.stack([row, col])


class _LEConv(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.lin1 = nn.Linear(in_channels, out_channels)
        self.lin2 = nn.Linear(in_channels, out_channels, bias=False)
        self.lin3 = nn.Linear(in_channels, out_channels)


class ASAPooling(nn.Module):
    """PyG 2.x ASAPooling(in_channels, ratio) without the optional GNN / dropout: parameters lin, att, gnn_score.lin1-3."""

    def __init__(self, in_channels, ratio=0.5, GNN=None, dropout=0.0, negative_slope=0.2, add_self_loops=False, **kw):
        super().__init__()
        assert GNN is None and dropout == 0.0 and negative_slope == 0.2
        self.ratio = ratio
        self.lin = nn.Linear(in_channels, in_channels)
        self.att = nn.Linear(2 * in_channels, 1)
        self.gnn_score = _LEConv(in_channels, 1)

    def forward(self, x, edge_index, edge_weight=None, batch=None):
        B = int(batch.max()) + 1
        N = x.shape[0] // B
        g = self.gnn_score
        params = [self.lin.weight, self.lin.bias, self.att.weight, self.att.bias, g.lin1.weight, g.lin1.bias, g.lin2.weight,
                  g.lin3.weight, g.lin3.bias]
        out, perm = R.asap_pool(x, B, N, params, self.ratio, edge_index=edge_index)
        return out, None, None, batch[perm], perm          # (the coarsened edge list: discarded by the reference)


stub_nn.knn = knn
stub_nn.ASAPooling = ASAPooling
import net_blocks as ref_blocks  # noqa: E402  (the reference's module, importing the patched stub)

torch.set_num_threads(1)


def _shapes(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def _save(name, fx):
    path = os.path.join(REPO, 'tests', 'golden', name)
    torch.save(fx, path)
    print('wrote', path, os.path.getsize(path), 'bytes')


def encoder(name, config, B, N, seed):
    del KNN_CALLS[:]
    torch.manual_seed(seed)
    model = ref_blocks.EdgeConvFeatures(16, config).double().train()
    pos = torch.randn(B, N, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 1))
    with torch.no_grad():
        enc, out, batch = model(pos)
    _save(name, {'kind': 'EdgeConvFeatures', 'out_size': 16, 'config': dict(config), 'merged_config': dict(model.config),
                 'B': B, 'N': N, 'positions': pos, 'state_dict': model.state_dict(), 'shapes': _shapes(model),
                 'knn_calls': list(KNN_CALLS), 'encoding': enc, 'out': out, 'batch': batch})


def pool(name, F, ratio, B, N, seed):
    del KNN_CALLS[:]
    torch.manual_seed(seed)
    model = ref_blocks.DynamicASAPool(F, k=5, pool_ratio=ratio).double().train()
    x = torch.randn(B * N, F, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 1))
    batch = torch.arange(B).repeat_interleave(N)
    with torch.no_grad():
        out, new_batch = model(x, batch)
    _save(name, {'kind': 'DynamicASAPool', 'F': F, 'k_given': 5, 'ratio': ratio, 'B': B, 'N': N, 'x': x,
                 'state_dict': model.state_dict(), 'shapes': _shapes(model), 'knn_calls': list(KNN_CALLS), 'out': out,
                 'batch': new_batch})


def pooling_features(name, config, B, N, seed):
    del KNN_CALLS[:]
    torch.manual_seed(seed)
    model = ref_blocks.EdgeConvPoolingFeatures(12, config).double().train()
    pos = torch.randn(B, N, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 1))
    with torch.no_grad():
        out = model(pos)
    _save(name, {'kind': 'EdgeConvPoolingFeatures', 'out_size': 12, 'config': dict(config), 'merged_config': dict(model.config),
                 'B': B, 'N': N, 'positions': pos, 'state_dict': model.state_dict(), 'shapes': _shapes(model),
                 'default_shapes': _shapes(ref_blocks.EdgeConvPoolingFeatures(12)), 'knn_calls': list(KNN_CALLS), 'out': out})


if __name__ == '__main__':
    encoder('asap_encoder_d2.pt', {'conv_depth': 2, 'graph_pooling': True, 'pool_ratio': 0.3, 'k_neighbors': 5,
                                   'EConv_feature': 16, 'EConv_hidden': 24, 'global_pool': 'max'}, 2, 96, 0)
    encoder('asap_encoder_d3.pt', {'conv_depth': 3, 'graph_pooling': True, 'pool_ratio': 0.5, 'k_neighbors': 4,
                                   'EConv_feature': 18, 'EConv_hidden': 21}, 2, 120, 1)
    pool('asap_pool.pt', 8, 0.3, 2, 50, 2)
    pooling_features('asap_pooling_features.pt', {'n_features1': 8, 'n_features2': 12, 'n_features3': 16}, 2, 80, 3)

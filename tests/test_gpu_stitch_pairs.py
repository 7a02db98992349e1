"""-m gpu: stitch recovery from the edge-pair classifier on the device (csrc/gpe_stitch_pairs.hip through ops.stitch_pairs /
StitchOnEdge3DPairs.predict_stitches) against the fp64 restatement (tests/stitch_pairs_restate.py), which
tests/test_stitch_pairs_host.py pins to the reference's recorded output.  Every test runs both routes (the fused store-free kernel
and the materialised rows through the dense-MLP kernels) in every arithmetic mode with the f16x3 size gate lifted.

The fixtures (tests/golden/stitch_pairs_*.pt) carry decision margins of 4 tol by construction (scripts/make_stitch_pairs_golden.py),
tol = 1e-4 * max(1, max |logit|), so stitches are compared exactly and nothing is excluded."""
import glob
import os

import numpy as np
import pytest
import torch

import stitch_pairs_restate as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(f for f in glob.glob(os.path.join(HERE, 'golden', 'stitch_pairs_*.pt')) if 'known_answer' not in f)
IDS = [os.path.basename(f)[len('stitch_pairs_'):-3] for f in FIXTURES]
ROUTES = ('fused', 'rows')


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


@pytest.fixture(scope='module')
def known():
    return torch.load(os.path.join(HERE, 'golden', 'stitch_pairs_known_answer.pt'), weights_only=False)


def _shipped(gpe, known):
    model = gpe.nets.StitchOnEdge3DPairs(known['data_config'], dict(known['nn_config']), {})
    model.load_state_dict(known['state_dict'])
    return model.cuda().eval()


def _random_model(gpe, hidden, layers, seed):
    """random weights with non-trivial BatchNorm running statistics (the folds must matter)"""
    torch.manual_seed(seed)
    model = gpe.nets.StitchOnEdge3DPairs({'element_size': 16}, {'stitch_hidden_size': hidden, 'stitch_mlp_n_layers': layers}, {})
    g = torch.Generator().manual_seed(seed + 1)
    for i in range(len(model.mlp)):
        bn = model.mlp[i][2]
        C = bn.weight.shape[0]
        bn.running_mean.copy_(torch.rand(C, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        bn.weight.data.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.data.copy_(torch.randn(C, generator=g) * 0.2)
    # both signs of the logit must occur: the output BatchNorm is centred on the mean of relu(z) over the pairs of one fixture,
    # computed by the fp64 restatement (an input of the test, not an output of the code under test)
    n = len(model.mlp) - 1
    last = model.mlp[n]
    last[0].bias.data.fill_(0.3)
    last[2].bias.data.fill_(0.0)
    fx = _load([f for f in FIXTURES if f.endswith('gaps.pt')][0])
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd['mlp.%d.2.running_mean' % n].zero_()
    sd['mlp.%d.2.running_var' % n].fill_(1.0 - 1e-5)
    sd['mlp.%d.2.weight' % n].fill_(1.0)
    sd['mlp.%d.2.bias' % n].zero_()
    r = R.logits64(sd, R.pair_rows(fx['edges'].numpy(), fx['pairs']), fx['f_shift'], fx['f_scale'])
    last[2].running_mean.fill_(float(r.mean()))
    return model.cuda().eval()


def _load(path):
    fx = torch.load(path, weights_only=False)
    fx['pairs'] = [tuple(int(v) for v in row) for row in fx['ref_order'].tolist()]
    fx['stats'] = {'f_shift': fx['f_shift'], 'f_scale': fx['f_scale']}
    return fx


def _padded(fx, P, L):
    e, n = fx['edges'], fx['num_edges']
    edges = torch.full((P, L, e.shape[-1]), 1e3)            # slots beyond the counts must be ignored, whatever they hold
    edges[:e.shape[0], :e.shape[1]] = e
    for p in range(e.shape[0]):
        edges[p, int(n[p]):] = 1e3
    ne = torch.zeros(P, dtype=torch.int64)
    ne[:n.shape[0]] = n
    return edges, ne


def _predict(model, edges, ne, stats, route, logits=True):
    out = model.predict_stitches(edges.cuda(), ne.cuda(), stats, route=route, return_logits=logits)
    return {k: v.cpu() for k, v in out.items()}


def _check_garment(out, b, fx, P, L, lg64, tol, exact_vs_fp64):
    """one garment of a call against the restatement; -> the product's logits in enumeration order"""
    pairs = fx['pairs']
    dense = out['logits'][b].numpy()
    assert dense.shape == (P * L, P * L)
    valid = np.zeros((P * L, P * L), dtype=bool)
    own = np.zeros(0, dtype=np.float32)
    if pairs:
        idx = np.asarray(pairs)
        valid[idx[:, 0] * L + idx[:, 2], idx[:, 1] * L + idx[:, 3]] = True
        own = R.dense_to_list(dense, pairs, L)
        err = np.abs(own.astype(np.float64) - lg64).max()
        print('garment %s: %d pairs, max |logit - fp64| = %.3g (tol %.3g)' % (fx['tag'], len(pairs), err, tol))
        assert err < tol
    assert np.isnan(dense[~valid]).all() and not np.isnan(dense[valid]).any()
    S = P * L // 2
    got_st, got_n, got_sc = out['stitches'][b].numpy(), int(out['num_stitches'][b]), out['scores'][b].numpy()
    assert got_st.shape == (2, S) and got_st.dtype == np.int32 and got_sc.shape == (S,)
    # (1) bit-exact against the selection fed with the product's own logits: epilogue + select kernels, whatever the arithmetic
    st, n, sc = R.as_tensors(R.stitches(pairs, own), P, L)
    assert got_n == n and np.array_equal(got_st, st)
    assert np.array_equal(got_sc, sc.astype(np.float32))
    # (2) the specification: fp64 logits, intended indexing
    if exact_vs_fp64:
        st, n, sc = R.as_tensors(R.stitches(pairs, lg64), P, L)
        assert got_n == n and np.array_equal(got_st, st)
        assert np.abs(got_sc - sc).max(initial=0.0) < tol
    return own


def _lg64(sd, fx):
    return R.logits64(sd, R.pair_rows(fx['edges'].numpy(), fx['pairs']), fx['f_shift'], fx['f_scale'])


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
def test_fixture_on_device(gpe, known, math_mode, path, route):
    fx = _load(path)
    model = _shipped(gpe, known)
    P, L = fx['edges'].shape[:2]
    out = _predict(model, fx['edges'][None], fx['num_edges'][None], fx['stats'], route)
    lg64 = _lg64(known['state_dict'], fx)
    assert abs(R.tol_of(lg64) - fx['tol']) < 1e-12
    _check_garment(out, 0, fx, P, L, lg64, fx['tol'], exact_vs_fp64=True)
    assert int(out['num_stitches'][0]) == len(R.stitches(fx['pairs'], lg64))
    if fx['positives'] < 2:
        assert int(out['num_stitches'][0]) == fx['positives']          # zero or one positives are ordinary results


@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
def test_routes_agree(gpe, known, math_mode, path):
    fx = _load(path)
    model = _shipped(gpe, known)
    a = _predict(model, fx['edges'][None], fx['num_edges'][None], fx['stats'], 'fused')
    b = _predict(model, fx['edges'][None], fx['num_edges'][None], fx['stats'], 'rows')
    assert torch.equal(a['stitches'], b['stitches']) and torch.equal(a['num_stitches'], b['num_stitches'])
    la, lb = a['logits'], b['logits']
    assert torch.equal(torch.isnan(la), torch.isnan(lb))
    d = (la - lb)[~torch.isnan(la)]
    assert d.numel() == len(fx['pairs']) and (d.numel() == 0 or d.abs().max().item() < 2 * fx['tol'])
    assert (a['scores'] - b['scores']).abs().max().item() < 2 * fx['tol']


@pytest.mark.parametrize('hidden,layers', [(64, 1), (100, 2), (200, 3), (256, 4), (36, 4)])
def test_fused_menu_shapes(gpe, math_mode, hidden, layers):
    """every accumulator width of the fused kernel (4 / 8 / 13 / 16 column blocks) and every depth, random weights"""
    model = _random_model(gpe, hidden, layers, 100 + hidden)
    assert gpe.ops.stitch_pairs_on_menu(model.mlp)
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    for path in FIXTURES[:]:
        fx = _load(path)
        if fx['tag'] not in ('gaps', 'claimed'):
            continue
        P, L = fx['edges'].shape[:2]
        lg64 = _lg64(sd, fx)
        outs = {}
        for route in ROUTES:
            outs[route] = _predict(model, fx['edges'][None], fx['num_edges'][None], fx['stats'], route)
            _check_garment(outs[route], 0, fx, P, L, lg64, R.tol_of(lg64), exact_vs_fp64=False)
        assert (lg64 > 0).any() and (lg64 < 0).any()


def test_off_menu_runs_through_auto(gpe, math_mode):
    model = _random_model(gpe, 30, 5, 77)
    assert not gpe.ops.stitch_pairs_on_menu(model.mlp)
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    fx = _load([f for f in FIXTURES if f.endswith('gaps.pt')][0])
    P, L = fx['edges'].shape[:2]
    lg64 = _lg64(sd, fx)
    out = _predict(model, fx['edges'][None], fx['num_edges'][None], fx['stats'], 'auto')
    _check_garment(out, 0, fx, P, L, lg64, R.tol_of(lg64), exact_vs_fp64=False)
    with pytest.raises(ValueError):
        model.predict_stitches(fx['edges'][None].cuda(), fx['num_edges'][None].cuda(), fx['stats'], route='fused')


@pytest.mark.parametrize('route', ROUTES)
def test_batched_equals_per_garment_and_repeats_bit_identically(gpe, known, math_mode, route):
    fxs = [_load(f) for f in FIXTURES]
    model = _shipped(gpe, known)
    P = max(fx['edges'].shape[0] for fx in fxs) + 1
    L = max(fx['edges'].shape[1] for fx in fxs) + 2
    padded = [_padded(fx, P, L) for fx in fxs]
    edges, ne = torch.stack([p[0] for p in padded]), torch.stack([p[1] for p in padded])
    stats = fxs[0]['stats']
    a = _predict(model, edges, ne, stats, route)
    b = _predict(model, edges, ne, stats, route)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k          # bit-identical, NaNs included
    for i, fx in enumerate(fxs):
        lg64 = _lg64(known['state_dict'], fx)
        _check_garment(a, i, fx, P, L, lg64, fx['tol'], exact_vs_fp64=True)
        one = _predict(model, edges[i:i + 1], ne[i:i + 1], stats, route)
        for k in one:
            assert torch.equal(one[k][0].view(torch.int32), a[k][i].view(torch.int32)), (fx['tag'], k)


def test_outputs_stay_on_the_device_without_logits(gpe, known):
    fx = _load(FIXTURES[0])
    model = _shipped(gpe, known)
    out = model.predict_stitches(fx['edges'][None].cuda(), fx['num_edges'][None].int().cuda(), fx['stats'])
    assert set(out) == {'stitches', 'num_stitches', 'scores'} and all(v.is_cuda for v in out.values())
    assert out['stitches'].dtype == torch.int32 and out['num_stitches'].dtype == torch.int32 and out['scores'].dtype == torch.float32
    with pytest.raises(RuntimeError, match='eval'):
        model.train().predict_stitches(fx['edges'][None].cuda(), fx['num_edges'][None].cuda(), fx['stats'])

"""Training the edge-pair classifier (nets.StitchOnEdge3DPairs) on the device, metrics on:
  (a) three training steps recorded from the reference's own classes (tests/golden/stitch_train_small.pt,
      scripts/make_stitch_train_golden.py) in every arithmetic mode, with the bars of test_stitch_model_known_answer;
  (b) six FusedAdam steps at the shipped architecture against an fp64 torch restatement stepped by torch.optim.Adam;
  (c) the same steps captured by graph.StepGraph with the loss dict as extras: bit-equal to the eager steps;
  (d) forward and backward of the device loss inside a stream capture: no host read.

Measured on one MI355X (worst over the three steps, as fractions of the bars of (a)): see DESIGN.md section 5.29."""
import copy
import os

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

METRICS = ('edge_pair_class_loss', 'edge_pair_class_acc', 'stitch_precision', 'stitch_recall')
COUNTS = ('pairs', 'correct', 'true_positives', 'predicted_positives', 'gt_positives')


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


@pytest.fixture(scope='module')
def recorded(golden_dir):
    return torch.load(os.path.join(golden_dir, 'stitch_train_small.pt'), weights_only=False)


def _labels_of(rows):
    """the generator's labels: a fixed function of the rows, about a quarter positives"""
    return rows[..., 0] + 0.5 * rows[..., 1] * rows[..., 2] > 0.75


def test_reference_pinned_training_steps(gpe, recorded, math_mode):
    fx = recorded
    pairs, labels = fx['pairs'].cuda(), fx['labels'].cuda()
    after = [s['state_before'] for s in fx['steps'][1:]] + [fx['state_after']]
    worst = {'logits': 0.0, 'loss': 0.0, 'grad': 0.0}
    for i, (s, nxt) in enumerate(zip(fx['steps'], after)):
        model = gpe.nets.StitchOnEdge3DPairs(fx['data_config'], dict(fx['nn_config']), {})
        model.load_state_dict(s['state_before'])
        model = model.cuda().train()
        assert model.loss.with_quality_eval
        out = model(pairs)
        loss, d, _ = model.loss(out, labels)
        counts = gpe.ops.pair_class_loss(out.detach(), labels, return_counts=True)[1]
        loss.backward()
        ref = s['logits']
        scale = max(1.0, ref.abs().max().item())
        e_logits = (out.detach().cpu() - ref).abs().max().item()
        e_loss = abs(loss.item() - s['full_loss'])
        worst['logits'] = max(worst['logits'], e_logits / (1e-4 * scale))
        worst['loss'] = max(worst['loss'], e_loss / 1e-5)
        assert e_logits < 1e-4 * scale, (i, e_logits)
        assert e_loss < 1e-5, (i, loss.item(), s['full_loss'])
        # the class decisions of the recorded logits are at least 1e-3 from a change: counts and ratios exactly
        assert counts.tolist() == [s['counts'][k] for k in COUNTS], i
        assert list(d) == list(METRICS) and d['edge_pair_class_loss'] is loss
        for k in METRICS[1:]:
            assert d[k].item() == s['loss_dict'][k], (i, k)
        for n, p in model.named_parameters():
            g = s['grads'][n]
            e = (p.grad.cpu() - g).abs().max().item() / (g.abs().max().item() + 1e-12)
            worst['grad'] = max(worst['grad'], e / 5e-3)
            assert e < 5e-3, (i, n, e)
        sd = model.state_dict()
        for k, v in nxt.items():
            if 'running_' in k:
                assert torch.allclose(sd[k].cpu(), v, rtol=1e-4, atol=1e-6), (i, k)
            elif 'num_batches_tracked' in k:
                assert sd[k].item() == v.item(), (i, k)
    print('%s: worst distance over the recorded steps, as a fraction of its bar: logits %.3g  loss %.3g  gradients %.3g'
          % (math_mode, worst['logits'], worst['loss'], worst['grad']))


def _shipped(gpe, seed=7):
    """the shipped architecture (16 pair features, 200 x 3) on rows [2, 406, 16] with the generator's labels"""
    torch.manual_seed(seed)
    model = gpe.nets.StitchOnEdge3DPairs({'element_size': 16}, {}, {})
    assert model.config['stitch_hidden_size'] == 200 and model.config['stitch_mlp_n_layers'] == 3
    rows = torch.randn(2, 406, 16, generator=torch.Generator().manual_seed(seed + 1))
    return model, rows, _labels_of(rows)


def test_training_trajectory_at_the_shipped_architecture(gpe):
    from gpe_amd import optim
    model, rows, labels = _shipped(gpe)
    # the same Sequential restated in torch, float64, from the same weights
    chans = [16, 200, 200, 200, 1]
    o64 = nn.Sequential(*[nn.Sequential(nn.Linear(chans[i - 1], chans[i]), nn.ReLU(), nn.BatchNorm1d(chans[i]))
                          for i in range(1, len(chans))])
    o64.load_state_dict(model.mlp.state_dict())
    o64 = o64.double().train()
    oopt = torch.optim.Adam(o64.parameters(), lr=2e-3)
    model = model.cuda().train()
    opt = optim.FusedAdam(optim.FlatArena(model), lr=2e-3)
    rd, ld = rows.cuda(), labels.cuda()
    losses, olosses = [], []
    for step in range(6):
        loss, d, _ = model.loss(model(rd), ld)
        loss.backward()
        opt.step()
        ol = nn.functional.binary_cross_entropy_with_logits(o64(rows.double().view(-1, 16)).view(-1), labels.double().view(-1))
        oopt.zero_grad(set_to_none=True)
        ol.backward()
        oopt.step()
        losses.append(loss.item()); olosses.append(ol.item())
        assert set(d) == set(METRICS)
    print('losses', ['%.6f' % v for v in losses], 'oracle', ['%.6f' % v for v in olosses],
          'worst |difference| %.3g' % max(abs(a - b) for a, b in zip(losses, olosses)))
    if olosses[-1] < olosses[0]:
        assert losses[-1] < losses[0]
    for a, b in zip(losses, olosses):
        assert abs(a - b) < 2e-3 * max(1.0, abs(b)), (losses, olosses)


@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
def test_captured_step_with_metrics_replays_the_eager_steps(gpe, mode):
    from gpe_amd import optim, graph
    prev = gpe.set_math(mode)
    prev_rows = gpe.set_f16x3_min_rows(0)
    try:
        model_a, rows, labels = _shipped(gpe)
        model_a = model_a.cuda().train()
        model_b = copy.deepcopy(model_a)
        assert model_a.loss.with_quality_eval and model_b.loss.with_quality_eval
        rd, ld = rows.cuda(), labels.cuda()
        sched = lambda: optim.OneCycle(2e-3, 40)
        opt_a = optim.FusedAdam(optim.FlatArena(model_a), lr=2e-3, schedule=sched())
        opt_b = optim.FusedAdam(optim.FlatArena(model_b), lr=2e-3, schedule=sched())
        nsteps = 7
        eager = []
        for i in range(nsteps):
            loss, d, _ = model_a.loss(model_a(rd), ld)
            loss.backward()
            opt_a.step()
            eager.append((loss.detach().clone(), {k: v.detach().clone() for k, v in d.items()}))
        sg = graph.StepGraph(lambda f, g: model_b.loss(model_b(f), g)[:2], opt_b, warmup=2)
        replayed = []
        for i in range(nsteps):
            loss = sg.step(rd, ld)
            assert isinstance(sg.extras, tuple) and len(sg.extras) == 1 and list(sg.extras[0]) == list(METRICS)
            replayed.append((loss.detach().clone(), {k: v.clone() for k, v in sg.extras[0].items()}))
        sg.synchronize()
        torch.cuda.synchronize()
        assert sg.captures == 1 and sg.replays == nsteps - 2
        for i, ((la, da), (lb, db)) in enumerate(zip(eager, replayed)):
            assert torch.equal(la, lb), (i, float(la), float(lb))
            for k in METRICS:
                assert torch.equal(da[k], db[k]), (i, k, float(da[k]), float(db[k]))
        assert len({float(l) for l, _ in eager}) == nsteps              # the steps differ: a replay that stood still would show
        for (n, p), q in zip(model_a.named_parameters(), model_b.parameters()):
            assert torch.equal(p, q), n
        for (n, p), q in zip(model_a.named_buffers(), model_b.buffers()):
            assert torch.equal(p, q), n
        assert opt_a.t == opt_b.t and opt_a.steps == opt_b.steps and opt_a.last_lr == opt_b.last_lr
    finally:
        gpe.set_f16x3_min_rows(prev_rows)
        gpe.set_math(prev)


def test_device_loss_reads_nothing_on_the_host(gpe):
    """forward and backward of the loss with metrics on inside a stream capture: a host read there is an error of the runtime"""
    loss_obj = gpe.metrics.ComposedLoss({'element_size': 16}, {'loss_components': ['edge_pair_class'],
                                                               'quality_components': ['edge_pair_class', 'edge_pair_stitch_recall']})
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(2, 406, generator=g) * 3).cuda().requires_grad_(True)
    y = (torch.rand(2, 406, generator=g) < 0.25).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        full, d, _ = loss_obj(x, y)                                # eager: the values to meet, and the stream's ticket word
        full.backward()
        want = ({k: v.detach().clone() for k, v in d.items()}, x.grad.clone())
        x.grad = None
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg, stream=side):
            full, d, _ = loss_obj(x, y)
            full.backward()
        static = (d, x.grad)
        static[1].zero_()
        cg.replay()
    side.synchronize()
    assert list(static[0]) == list(METRICS)
    for k in METRICS:
        assert torch.equal(static[0][k].detach(), want[0][k]), k
    assert torch.equal(static[1], want[1])

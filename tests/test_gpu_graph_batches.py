"""gpe_amd/graph.py StepGraph on FRESH batches and in every branch of the loss: the captured full-model step replayed on batches
other than the one it was captured on must be the eager step on that batch, bit for bit (tests/test_gpu_graph.py hands the same
two tensor objects to every step, at epoch 0, with the default loss).

Every case runs the same helper: three deep copies of one model, each with its own FusedAdam(FlatArena, lr 2e-3, OneCycle(2e-3, 40));
two run seven eager steps (the eager sequence must first equal itself), the third runs through StepGraph(warmup=2); all see the same
batches, torch.manual_seed(100 + i) in front of step i.  Three batches of bench.synthetic (seeds 1000, 1001, 1002) are cycled
b0 b1 b2 b0 b1 b2 b0, so the capture happens on b2 and the replays see all three.  The batches differ in structure: every pattern
has its own num_stitches in [1, S] (never 0: a pattern without stitches gives NaN by design), the clouds of b1 are scaled by 8 and
those of b2 by 0.1 (the model standardises nothing, so the amax words of the f16x3 kernels move).  Each step gets fresh clones: the
caller's tensors are never the static buffers.

Compared with torch.equal, no tolerance: the loss and the loss dict of every step; after the last step every parameter, buffer,
Adam's m and v, t / steps / last_lr; with a matching on, per step, last_permutation, last_leading_edges and both entries of
last_matched_stitch_gt.  The eager losses of steps 3, 4, 5 (b0, b1, b2) must differ pairwise, or the case would prove nothing.

epoch_with_order_matching stays 0: the pre-matching torch.randperm branch draws on the DEVICE generator, which a replay cannot
re-seed; it is out of scope here.  The captured step is single-stream; nothing here forks one.

Case 8 (the epoch crossing epoch_with_stitches in mid-run) is what graph.StepGraph got wrong: a non-tensor argument of step() was
frozen at the first call's value, so the stitch terms never started.  Its capture counts follow from StepGraph's rule (a changed
non-tensor argument or `key` value: one eager step, then a capture): with the epoch itself as the argument, the epochs
38 39 39 40 40 41 41 give eager eager CAPTURE eager CAPTURE eager CAPTURE (3 captures, 3 replays: 41 differs from 40 although the
loss does not); with the closure reading the epoch and key = (epoch >= epoch_with_stitches), eager eager CAPTURE eager CAPTURE
replay replay (2 captures, 4 replays)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

NSTEPS = 7
STITCH_EPOCH = 40


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _batches(data_config, B, N, dev):
    import bench
    S = data_config['max_num_stitches']
    out = []
    for j, scale in enumerate((1.0, 8.0, 0.1)):
        feats, gt = bench.synthetic(B, N, data_config, seed=1000 + j, device=dev)
        g = torch.Generator().manual_seed(2000 + j)
        gt['num_stitches'] = torch.randint(1, S + 1, (B,), generator=g).to(dev)
        out.append((feats * scale, gt))
    nums = [tuple(gt['num_stitches'].tolist()) for _, gt in out]
    assert len(set(nums)) == 3 and all(1 <= n <= S for t in nums for n in t)
    return out


def _fresh(batch):
    feats, gt = batch
    return feats.clone(), {k: v.clone() for k, v in gt.items()}


def _snapshot(loss, loss_dict, loss_obj, epoch, order, origin):
    """what one step left behind, cloned right after the step (a replay overwrites the tensors it returned)"""
    rec = {'loss': loss.detach().clone(), 'dict': {k: v.detach().clone() for k, v in loss_dict.items()}}
    if order:
        rec['perm'] = loss_obj.last_permutation.clone()
    if origin:
        rec['lead'] = loss_obj.last_leading_edges.clone()
    if loss_obj._stitch_terms_active(epoch):
        rec['stitches'] = loss_obj.last_matched_stitch_gt['stitches'].clone()
        rec['free'] = loss_obj.last_matched_stitch_gt['free_edges_mask'].clone()
    return rec


def _final(model, opt):
    state = {'param ' + n: p.detach() for n, p in model.named_parameters()}
    state.update({'buffer ' + n: b for n, b in model.named_buffers()})
    state.update(m=opt.m, v=opt.v)
    return state, (opt.t, list(opt.steps), opt.last_lr)


def _assert_same(what, recs_a, recs_b, end_a, end_b):
    for i, (a, b) in enumerate(zip(recs_a, recs_b)):
        assert torch.equal(a['loss'], b['loss']), (what, 'loss', i, float(a['loss']), float(b['loss']))
        assert list(a['dict']) == list(b['dict']), (what, 'loss dict keys', i, list(a['dict']), list(b['dict']))
        for k in a['dict']:
            assert torch.equal(a['dict'][k], b['dict'][k]), (what, k, i, float(a['dict'][k]), float(b['dict'][k]))
        assert set(a) == set(b), (what, i, sorted(a), sorted(b))
        for k in ('perm', 'lead', 'stitches', 'free'):
            if k in a:
                assert torch.equal(a[k], b[k]), (what, k, i)
    (sa, ha), (sb, hb) = end_a, end_b
    assert list(sa) == list(sb)
    for n in sa:
        assert torch.equal(sa[n], sb[n]), (what, n)
    assert ha == hb, (what, ha, hb)


def _run(gpe, mode, model_kind='lstm', B=4, N=256, k=5, nn_over=None, loss_over=None, epochs=(0,) * NSTEPS, variant='arg',
         expect=(1, NSTEPS - 2), want_neg=False, check_guards=False):
    """-> (eager records, StepGraph) after every assertion of the module docstring has held"""
    from gpe_amd import configs, nets, optim, graph
    dev = torch.device('cuda', 0)
    prev = gpe.set_math(mode)
    prev_rows = gpe.set_f16x3_min_rows(0)
    try:
        if check_guards:                 # (asked under the arithmetic of the case: the lazy dz3 exists in f16x3 only)
            assert gpe._lib.query('gpe_edge_lazy_dz3_ok', B, N, k, 150, 200) == 1
        data_config = configs.data_config()
        nn_cfg = (configs.att_model_config if model_kind == 'att' else configs.lstm_model_config)(k_neighbors=k, **(nn_over or {}))
        nn_cfg['loss'].update(loss_over or {})
        order, origin = nn_cfg['loss']['panel_order_inariant_loss'], nn_cfg['loss']['panel_origin_invariant_loss']
        torch.manual_seed(0)
        cls = nets.GarmentSegmentPattern3D if model_kind == 'att' else nets.GarmentFullPattern3D
        base = cls(data_config, dict(nn_cfg), dict(nn_cfg['loss'])).to(dev).train()
        base.loss.with_quality_eval = False
        models = [copy.deepcopy(base) for _ in range(3)]
        opts = [optim.FusedAdam(optim.FlatArena(m), lr=2e-3, schedule=optim.OneCycle(2e-3, 40)) for m in models]
        batches = _batches(data_config, B, N, dev)

        def eager(model, opt):
            recs = []
            for i in range(NSTEPS):
                feats, gt = _fresh(batches[i % 3])
                torch.manual_seed(100 + i)
                loss, loss_dict, _ = model.loss(model(feats), gt, epoch=epochs[i])
                loss.backward()
                opt.step()
                recs.append(_snapshot(loss, loss_dict, model.loss, epochs[i], order, origin))
            torch.cuda.synchronize()
            return recs

        recs_a = eager(models[0], opts[0])
        recs_a2 = eager(models[1], opts[1])
        # the reference of this file is the eager step: it has to be a function of its inputs before anything is compared with it
        _assert_same('eager against eager', recs_a, recs_a2, _final(models[0], opts[0]), _final(models[1], opts[1]))
        for i, r in enumerate(recs_a):
            print('step %d epoch %d: loss %.9g  %s' % (i, epochs[i], float(r['loss']),
                                                      '  '.join('%s %.6g' % (k_, float(v)) for k_, v in r['dict'].items())))
            assert bool(torch.isfinite(r['loss'])), i
        l3, l4, l5 = (float(recs_a[i]['loss']) for i in (3, 4, 5))
        assert l3 != l4 and l4 != l5 and l3 != l5, (l3, l4, l5)            # the three batches are told apart
        if want_neg:
            assert all('stitch_neg_loss' in r['dict'] for e, r in zip(epochs, recs_a) if e >= STITCH_EPOCH)
            assert any(float(r['dict'].get('stitch_neg_loss', 0.0)) > 0 for r in recs_a)

        model_b, opt_b = models[2], opts[2]
        state = {'epoch': epochs[0]}
        if variant == 'arg':
            sg = graph.StepGraph(lambda f, g, e: model_b.loss(model_b(f), g, epoch=e)[:2], opt_b, warmup=2)
        else:
            sg = graph.StepGraph(lambda f, g: model_b.loss(model_b(f), g, epoch=state['epoch'])[:2], opt_b, warmup=2,
                                 key=lambda: model_b.loss._stitch_terms_active(state['epoch']))
        recs_b, replayed = [], []
        for i in range(NSTEPS):
            feats, gt = _fresh(batches[i % 3])
            state['epoch'] = epochs[i]
            torch.manual_seed(100 + i)
            before = sg.replays
            loss = sg.step(feats, gt, epochs[i]) if variant == 'arg' else sg.step(feats, gt)
            assert feats.data_ptr() not in [t.data_ptr() for t in sg._flat(sg.static_in, [])]
            # the branch of the loss the step took (a frozen epoch shows here first: no stitch entries at epoch 40)
            assert list(sg.extras[0]) == list(recs_a[i]['dict']), (i, epochs[i], list(sg.extras[0]), list(recs_a[i]['dict']))
            recs_b.append(_snapshot(loss, sg.extras[0], model_b.loss, epochs[i], order, origin))
            replayed.append(sg.replays > before)
        sg.synchronize()
        torch.cuda.synchronize()
        print('captures %d replays %d, replayed steps %s' % (sg.captures, sg.replays, [i for i, r in enumerate(replayed) if r]))
        _assert_same('StepGraph against eager', recs_a, recs_b, _final(models[0], opts[0]), _final(model_b, opt_b))
        assert (sg.captures, sg.replays) == expect, (sg.captures, sg.replays)
        if order:
            identity = torch.arange(data_config['max_pattern_len'], device=dev).expand(B, -1)
            assert any(r and not torch.equal(rec['perm'], identity) for r, rec in zip(replayed, recs_b))
            assert not torch.equal(recs_b[3]['perm'], recs_b[4]['perm']) and not torch.equal(recs_b[4]['perm'], recs_b[5]['perm'])
            models[0].loss.check_order_match()
            model_b.loss.check_order_match()
        if check_guards:
            for m in (models[0], model_b):
                convs = [c for c in m.modules() if hasattr(c, 'half_act_guard')]
                assert convs and not any(c.half_act_guard.disabled for c in convs)
        return recs_a, sg
    finally:
        gpe.set_f16x3_min_rows(prev_rows)
        gpe.set_math(prev)


STITCH_RUN = dict(epochs=(STITCH_EPOCH,) * NSTEPS, want_neg=True)
MATCHING = dict(panel_order_inariant_loss=True, panel_origin_invariant_loss=True)


def test_fresh_batches_f32(gpe):
    """case 1: the plain captured step"""
    _run(gpe, 'f32')


def test_fresh_batches_f16x3_k16_lazy_dz3(gpe):
    """case 2: per-launch amax scale words, fp16 a3 rows and the lazily formed dz3 under clouds of changing magnitude"""
    _run(gpe, 'f16x3', B=8, N=512, k=16, check_guards=True)


def test_fresh_batches_attention_model_f16x3(gpe):
    """case 3: attention pooling and skip connections"""
    _run(gpe, 'f16x3', model_kind='att')


@pytest.mark.parametrize('hardnet', [False, True])
def test_stitch_terms_inside_a_capture(gpe, hardnet):
    """case 4: gpe_stitch_loss_fwd / bwd captured, num_stitches changing with the batch; the negative term is active"""
    _run(gpe, 'f32', loss_over=dict(stitch_hardnet_version=hardnet), **STITCH_RUN)


@pytest.mark.parametrize('order_by', ['shape_translation', 'stitches'])
@pytest.mark.parametrize('hardnet', [False, True])
def test_matchings_inside_a_capture(gpe, hardnet, order_by):
    """case 5: order_match, origin_match, stitch_renumber, panel_shift and the gathers under replay: the permutation and the
    leading edges are decided on the device from the batch and feed the launches behind them"""
    _run(gpe, 'f32', loss_over=dict(MATCHING, stitch_hardnet_version=hardnet, order_by=order_by), **STITCH_RUN)


def test_dropout_mask_between_recurrent_layers(gpe):
    """case 6: the HostDrawn mask consumes the CPU generator exactly as the eager step does"""
    _run(gpe, 'f32', nn_over=dict(dropout=0.3))


@pytest.mark.parametrize('decoder', ['GRUDecoderModule', 'LSTMDoubleReverseDecoderModule'])
def test_other_recurrence_stacks_f16x3(gpe, decoder):
    """case 7: the GRU and the double-reverse LSTM decoders in a capture"""
    _run(gpe, 'f16x3', nn_over=dict(panel_decoder=decoder, pattern_decoder=decoder))


@pytest.mark.parametrize('variant,expect', [('arg', (3, 3)), ('closure', (2, 4))])
def test_epoch_crossing_the_stitch_switch(gpe, variant, expect):
    """case 8: epochs 38 39 39 40 40 41 41 with the loss of case 5.  From the first epoch-40 step on the loss dict of the step —
    sg.extras[0] — carries the stitch entries (the module docstring derives the capture counts)."""
    epochs = (38, 39, 39, 40, 40, 41, 41)
    recs, sg = _run(gpe, 'f32', loss_over=dict(MATCHING, order_by='stitches'), epochs=epochs, variant=variant, expect=expect,
                    want_neg=True)
    main = ['pattern_loss', 'loop_loss', 'rotation_loss', 'translation_loss']
    stitch = ['stitch_similarity_loss', 'stitch_neg_loss', 'free_edges_loss']
    for e, r in zip(epochs, recs):
        assert list(r['dict']) == (main + stitch if e >= STITCH_EPOCH else main), (e, list(r['dict']))
    assert list(sg.extras[0]) == main + stitch

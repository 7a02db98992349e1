"""not-gpu: the drop-in surface — constructors, config merging, state-dict layout, error types — mirrors the reference
(SURVEY.md §8b), checked without touching the GPU."""
import copy
import json
import os

import pytest
import torch

import gpe_amd
from gpe_amd import configs, net_blocks, nets


def _full(**over):
    nn_cfg = configs.lstm_model_config(**over)
    return nets.GarmentFullPattern3D(configs.data_config(), nn_cfg, copy.deepcopy(nn_cfg['loss'])), nn_cfg


def test_state_dict_layout_and_param_count():
    model, _ = _full()
    sd = model.state_dict()
    assert len(sd) == 70
    assert sum(p.numel() for p in model.parameters()) == 2818765         # SURVEY.md §2.2 [probe]
    assert sd['feature_extractor.conv_layers.0.nn.0.0.weight'].shape == (200, 6)
    assert sd['feature_extractor.conv_layers.1.nn.0.0.weight'].shape == (200, 300)
    assert sd['feature_extractor.conv_layers.1.nn.2.2.running_var'].shape == (150,)
    assert sd['feature_extractor.conv_layers.0.nn.1.2.num_batches_tracked'].dtype == torch.int64
    assert sd['panel_decoder.lstm.weight_hh_l2'].shape == (1000, 250)
    assert sd['panel_decoder.lin.weight'].shape == (8, 250)
    assert sd['pattern_decoder.lin.weight'].shape == (250, 250)
    assert sd['placement_decoder.weight'].shape == (7, 250)


def test_fixture_state_keys_match(golden_dir):
    fx = torch.load(os.path.join(golden_dir, 'full3d_shipped.pt'), weights_only=False)
    torch.manual_seed(fx['seed'])
    model = nets.GarmentFullPattern3D(fx['data_config'], copy.deepcopy(fx['nn_config']),
                                      copy.deepcopy(fx['loss_config']))
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == [tuple(x) for x in fx['state_keys']]
    assert sorted(model.config.keys()) == fx['merged_config_keys']


ALL_FIXTURES = ['full3d_small', 'full3d_shipped', 'full3d_k16', 'segment3d_small', 'segment3d_shipped', 'segment3d_k20',
                'segment3d_globalatt', 'segment3d_globalatt_small', 'full3d_originmatch', 'full3d_ordermatch',
                'full3d_ordermatch_placement', 'full3d_poolmax', 'full3d_pooladd', 'full3d_aggrmean', 'full3d_aggradd',
                'full3d_depth1', 'full3d_depth3', 'full3d_mlpdec', 'full3d_gru', 'full3d_lstm2rev', 'segment3d_poolmax',
                'segment3d_pooladd']


@pytest.mark.parametrize('tag', ALL_FIXTURES)
def test_every_fixture_config_constructs_with_reference_layout(tag, golden_dir):
    """Every YAML variant the reference-generated fixtures cover (alternative decoders, pools, aggregations, depths,
    global attention) builds here with the reference's state-dict keys/shapes and, same seed, the same initial weights."""
    fx = torch.load(os.path.join(golden_dir, tag + '.pt'), weights_only=False)
    torch.manual_seed(fx['seed'])
    model = getattr(nets, fx['model'])(fx['data_config'], copy.deepcopy(fx['nn_config']),
                                       copy.deepcopy(fx['loss_config']))
    sd = model.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [tuple(x) for x in fx['state_keys']]
    assert sorted(model.config.keys()) == fx['merged_config_keys']
    if 'state_dict' in fx:
        for k, v in fx['state_dict'].items():
            assert torch.equal(sd[k], v), k
    plan = gpe_amd.ops.PackPlan()
    for m in model._pack_modules():
        m.register_packs(plan)
    model._register_own_packs(plan)
    assert len(plan.specs) > 0


def test_pack_plan_job_table():
    """the 64-byte job records gpe_pack_multi reads (include/gpe_hip.h): gpe_pack_job_blocks(kind, ..) 256-thread blocks per job (ABI 6:
    64 x 64 tiles for the row-major sources, 1024 outputs per block otherwise), jobs sorted by first_block, every output buffer sized
    to its job; one amax word per MATRIX, shared by its two plane packs; the table every arithmetic but f16x3 launches (table_noh3) is
    the full one without the plane jobs.  For the shipped LSTM decoders and for GRU decoders (three gates, no transposed planes)."""
    import numpy as np
    ops = gpe_amd.ops
    dc = configs.data_config()
    for gates, override in ((4, {}), (3, dict(panel_decoder='GRUDecoderModule', pattern_decoder='GRUDecoderModule'))):
        cfg = configs.lstm_model_config(k_neighbors=5, **override)
        model = nets.GarmentFullPattern3D(dc, dict(cfg), dict(cfg['loss']))
        plan = ops.PackPlan()
        for m in model._pack_modules():
            m.register_packs(plan)
        model._register_own_packs(plan)
        plan._build()
        tab = plan.table.numpy().view(ops._JOB)
        assert tab.dtype.itemsize == 64 and len(tab) == len(plan.specs)
        blk = 0
        for job, out in zip(tab, plan.outs):
            assert int(job['first_block']) == blk
            assert int(job['total']) == out.numel() and int(job['out']) == out.data_ptr()
            if int(job['kind']) < 5:
                assert int(job['total']) % 4 == 0                 # whole float4 quads
            kind, total, npad, K = int(job['kind']), int(job['total']), int(job['Npad']), int(job['K'])
            nb = gpe_amd._lib.query('gpe_pack_job_blocks', kind, total, npad, K)
            if kind in (0, 2):
                assert nb == -(-npad // 64) * -(-(total // npad) // 64)
            elif kind == 8:
                assert nb == -(-npad // 64) * -(-(-(-K // 32) * 32) // 64)
            else:
                assert nb == (total + 1023) // 1024
            blk += nb
        assert plan.blocks == blk
        pre = plan.pre_table.numpy().view(ops._JOB)
        assert len(set(int(j['w']) for j in pre)) == len(pre) == plan.words.numel()          # one amax job per matrix
        planes = [j for j in tab if int(j['kind']) in (8, 10)]
        assert all(int(j['w2']) in set(int(q['out']) for q in pre) for j in planes)
        if gates == 4:
            assert len(planes) > len(pre)
        else:
            assert len(planes) == len(pre) and not any(int(j['kind']) == 10 for j in tab)
        # the word of a plane job is the one whose address the job carries, and the one its matrix's amax job fills
        assert len(plan.word_of) == len(planes)
        for sp, job in zip(plan.specs, tab):
            assert int(job['kind']) == sp.kind and int(job['w']) == sp.p.data_ptr()
            if sp.kind in (8, 10):
                word = plan.word_of[(sp.p.data_ptr(), sp.kind)]
                assert word.numel() == 1 and word.data_ptr() == int(job['w2'])
                assert [int(q['w']) for q in pre if int(q['out']) == word.data_ptr()] == [sp.p.data_ptr()]
                at = (word.data_ptr() - plan.words.data_ptr()) // 4
                assert 0 <= at < plan.words.numel() and plan.words[at:at + 1].data_ptr() == word.data_ptr()
        # table_noh3: the rows of the full table that are no plane jobs, field by field, first_block running over them alone
        keep = [j for j in tab if int(j['kind']) not in (8, 10)]
        noh3 = plan.table_noh3.numpy().view(ops._JOB)
        assert plan.n_noh3 == len(noh3) == len(keep) < len(tab)
        blk = 0
        for job, full in zip(noh3, keep):
            for field in ops._JOB.names:
                assert int(job[field]) == (blk if field == 'first_block' else int(full[field])), field
            blk += gpe_amd._lib.query('gpe_pack_job_blocks', int(job['kind']), int(job['total']), int(job['Npad']), int(job['K']))
        assert plan.blocks_noh3 == blk < plan.blocks


def test_stitch_model_layout(golden_dir):
    fx = torch.load(os.path.join(golden_dir, 'stitch_pairs_known_answer.pt'), weights_only=False)
    model = nets.StitchOnEdge3DPairs(fx['data_config'], dict(fx['nn_config']), {})
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == \
        [(k, tuple(v.shape)) for k, v in fx['state_dict'].items()]
    model.load_state_dict(fx['state_dict'])
    assert model.config['loss']['loss_components'] == ['edge_pair_class']


def test_onecycle_matches_torch():
    from gpe_amd.optim import OneCycle
    net = torch.nn.Linear(2, 2)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=2e-3, epochs=7, steps_per_epoch=13, cycle_momentum=False)
    ours = OneCycle(2e-3, 7 * 13)
    for step in range(7 * 13):
        assert abs(ours.lr(step) - opt.param_groups[0]['lr']) < 1e-12, step
        opt.step()
        if step < 7 * 13 - 1:
            sch.step()
    with pytest.raises(ValueError):
        ours.lr(7 * 13)


def test_loss_has_no_cpu_path():
    """ComposedPatternLoss evaluates on the device through the HIP kernels or not at all: CPU predictions raise (the model
    path has no torch-math fallback either, tests/test_abi.py).  Value / gradient / matching parity vs the oracle's loop
    restatement is a GPU test (tests/test_gpu_kernels.py::test_pattern_loss_and_matching, ::test_stitch_losses_and_renumbering)."""
    dc = configs.data_config()
    g = torch.Generator().manual_seed(0)
    B, P, Lp = 3, 23, 14
    preds = {'outlines': torch.randn(B, P, Lp, 4, generator=g), 'rotations': torch.randn(B, P, 4, generator=g),
             'translations': torch.randn(B, P, 3, generator=g)}
    gt = {'outlines': torch.randn(B, P, Lp, 4, generator=g), 'rotations': torch.randn(B, P, 4, generator=g),
          'translations': torch.randn(B, P, 3, generator=g), 'num_edges': torch.randint(0, Lp + 1, (B, P), generator=g),
          'empty_panels_mask': torch.zeros(B, P, dtype=torch.bool)}
    for cfg in (dict(panel_origin_invariant_loss=True, panel_order_inariant_loss=True, order_by='shape_translation'),
                dict(panel_origin_invariant_loss=False, panel_order_inariant_loss=False)):
        cfg = dict(cfg, loss_components=['shape', 'loop', 'rotation', 'translation'], quality_components=[],
                   epoch_with_order_matching=0)
        loss = gpe_amd.metrics.ComposedPatternLoss(dc, cfg)
        with pytest.raises(RuntimeError, match='no CPU path'):
            loss(preds, {k: v.clone() for k, v in gt.items()}, epoch=0)


def test_config_merge_and_caller_mutation():
    cfg = {'panel_encoding_size': 64, 'pattern_encoding_size': 48, 'EConv_hidden': 32, 'EConv_feature': 24}
    loss_cfg = {'panel_origin_invariant_loss': False, 'panel_order_inariant_loss': False}
    model = nets.GarmentFullPattern3D(configs.data_config(), cfg, loss_cfg)
    # back-compat: the CALLER's dict gains the hidden sizes (nn/nets.py:75-78)
    assert cfg['panel_hidden_size'] == 64 and cfg['pattern_hidden_size'] == 48
    assert model.config['k_neighbors'] == 5 and model.config['EConv_aggr'] == 'max'      # extractor defaults merged
    assert model.config['loss'] is model.loss.config
    assert model.config['model'] == 'GarmentFullPattern3D'
    assert model.panel_decoder.lstm.weight_ih_l0.shape == (256, 64)


def test_error_types_match_reference():
    with pytest.raises(ValueError):
        net_blocks.EdgeConvFeatures(16, {'global_pool': 'median'})
    with pytest.raises(NotImplementedError):
        net_blocks._init_tenzor(2, 3, 4, init_type='xavier')
    with pytest.raises(AttributeError):
        _full(feature_extractor='NoSuchExtractor')
    with pytest.raises(NotImplementedError):        # selectable in the reference, no kernels yet: loud, not silent
        _full(feature_extractor='EdgeConvPoolingFeatures')


def test_train_eval_forward_to_loss():
    model, _ = _full()
    model.eval()
    assert model.loss.training is False and not model.feature_extractor.conv_layers[0].nn[0][2].training
    model.train()
    assert model.loss.training is True


def test_configs_equal_shipped_yamls(golden_dir):
    # the `NN` and `dataset` sections of the reference's shipped YAMLs, stored verbatim by oracle/refgen/make_golden.py
    with open(os.path.join(golden_dir, 'shipped_yaml_configs.json')) as f:
        shipped = json.load(f)
    for rel, fn in [('models/baseline/lstm_stitch_tags.yaml', configs.lstm_model_config),
                    ('models/att/att.yaml', configs.att_model_config)]:
        y = shipped[rel]
        ref_nn = y['NN']
        ref_nn.pop('pre-trained')
        assert fn() == ref_nn
        for k, v in configs.data_config().items():
            if k in y['dataset'] and k != 'max_pattern_len':
                assert y['dataset'][k] == v, k


def test_bench_workload_names():
    """bench.py labels the BASELINE.json configuration its arguments amount to, and nothing else as one."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(os.path.dirname(os.path.dirname(__file__)), 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    mk = lambda m, n, b, k: types.SimpleNamespace(model=m, points=n, batch=b, k=k)
    assert bench._workload_name(mk('lstm', 2048, 32, 16)).startswith('BASELINE cfg 2')
    assert bench._workload_name(mk('lstm', 1024, 8, 5)).startswith('BASELINE cfg 1')
    assert bench._workload_name(mk('att', 4096, 32, 20)).startswith('BASELINE cfg 4')
    assert bench._workload_name(mk('lstm', 8192, 64, 16)).startswith('BASELINE cfg 5')
    assert bench._workload_name(mk('lstm', 1000, 3, 10)).startswith('custom shape')
    assert 'N=1000, batch 3/GPU, k=10' in bench._workload_name(mk('lstm', 1000, 3, 10))


def test_bench_plain_run_and_output_dump(tmp_path, monkeypatch):
    """A plain bench.py run measures only the timed steps (--full is off by default); --dump-outputs writes fp32 / fp64 .npy files
    within the 64 MB budget, a larger array as a fixed, seeded sample of its elements."""
    import importlib.util
    import sys
    import numpy as np
    spec = importlib.util.spec_from_file_location('bench_mod_dump', os.path.join(os.path.dirname(os.path.dirname(__file__)), 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', str(tmp_path)])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == str(tmp_path)
    small = {'loss': torch.tensor(1.5), 'pred_x': torch.arange(12, dtype=torch.float16).view(3, 4), 'w': torch.ones(5, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / 'a'), small)
    got = {n: np.load(str(tmp_path / 'a' / (n + '.npy'))) for n in small}
    assert got['loss'].dtype == np.float32 and got['loss'].shape == () and got['loss'] == 1.5
    assert got['pred_x'].dtype == np.float32 and got['pred_x'].shape == (3, 4) and (got['pred_x'].ravel() == np.arange(12)).all()
    assert got['w'].dtype == np.float64
    big = {'params': torch.arange(4000, dtype=torch.float32), 'loss': torch.tensor(2.0)}
    for d in ('b1', 'b2'):
        bench.dump_outputs(str(tmp_path / d), big, budget=8000)
    p1, p2 = (np.load(str(tmp_path / d / 'params.npy')) for d in ('b1', 'b2'))
    assert p1.shape == (1000,) and (p1 == p2).all() and (np.diff(p1) > 0).all() and p1.max() < 4000
    assert sum(os.path.getsize(str(tmp_path / 'b1' / f)) for f in os.listdir(str(tmp_path / 'b1'))) < 8000 + 2 * 256


def test_bench_quotes_counter_traffic_only_for_what_it_measured(monkeypatch):
    """bench.py's `traffic` fields come from the committed PMC passes: refused when the kernel sources changed since (csrc hash)
    and — since round 4 — when the run is not the workload those passes measured (another shape / model / loss epoch / arithmetic),
    and the per-call work model follows the arguments the lazy-dz3 / fp16-activation paths add."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod2', os.path.join(os.path.dirname(os.path.dirname(__file__)), 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    doc, src, why = bench._pmc_doc()
    if doc is None:
        # kernel sources edited since the last committed PMC pass: the file must be REFUSED, naming both hashes — then the rest of
        # the logic is exercised on that file with this tree's hash stamped in (the state every round's final evidence call restores)
        import glob
        import json
        assert why.startswith('refused: profiles/') and bench.csrc_sha() in why, why
        assert bench.pmc_traffic('gpe_edge_mlp_bwd:inplace', 2.0) == (None, why) and bench.pmc_step_bytes() == (None, None)
        newest = sorted(glob.glob(os.path.join(bench.REPO, 'profiles', '*_hbm_traffic.json')))[-1]
        stamped = dict(json.load(open(newest)), csrc_sha=bench.csrc_sha())
        monkeypatch.setattr(bench.json, 'load', lambda f: stamped)
        doc, src, why = bench._pmc_doc()
    assert doc is not None and src.startswith('profiles/') and why is None, why     # the committed file matches this tree's csrc
    assert doc['csrc_sha'] == bench.csrc_sha()
    per_launch, _ = bench.pmc_traffic('gpe_edge_mlp_bwd:inplace', 2.0)
    assert 1.5e9 < per_launch < 3e9                           # the lazy B3: a3 (fp16) + a2 in, dz2 out
    assert bench.pmc_traffic('gpe_edge_dz3')[0] is None       # no such launch in the benched mode any more
    bench._PMC_APPLIES[0], bench._PMC_APPLIES[1] = False, 'not quoted: other workload'
    assert bench._pmc_doc() == (None, None, 'not quoted: other workload')
    assert bench.pmc_step_bytes() == (None, None)
    # algorithmic bytes: fp16 rows where the arguments say so (last int of the call: out_half / lz_ldagg)
    E = 32 * 2048 * 16
    fwd32 = bench.call_work('gpe_edge_mlp_fwd', (1, 0, 200, 32, 2048, 16, 200, 150, 152, 1, 152, 4096, 0))[1]
    fwd16 = bench.call_work('gpe_edge_mlp_fwd', (1, 0, 200, 32, 2048, 16, 200, 150, 152, 1, 152, 4096, 1))[1]
    assert fwd32 - fwd16 == E * 150 * 2
    b32 = bench.call_work('gpe_edge_mlp_bwd', (152, 0, 0, 32, 2048, 16, 150, 200, 200, 0, 4096, 0, 0))[1]
    b16 = bench.call_work('gpe_edge_mlp_bwd', (152, 0, 0, 32, 2048, 16, 150, 200, 200, 0, 4096, 150, 152))[1]
    assert b32 - b16 == E * 150 * 2


def test_bench_dominant_kernel_is_a_single_kernel_entry(monkeypatch):
    """bench.py's top-level `roofline` prices the dominant KERNEL (rocprof's average duration of that kernel must
    agree): sequences of dependent launches behind one C-ABI call (the recurrences: 40 / 80 launches) are priced in
    roofline_per_kernel and only NAMED in roofline.largest_sequence when they outweigh it; the w8 kernels' counter traffic is found
    in the committed PMC pass under their C-ABI entry."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location('bench_mod3', os.path.join(os.path.dirname(os.path.dirname(__file__)), 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    if bench._pmc_doc()[0] is None:
        # kernel sources edited since the last committed PMC pass (refused, see the test above): exercise the logic on that file with
        # this tree's hash stamped in
        import glob
        import json
        real = json.load
        monkeypatch.setattr(bench.json, 'load', lambda f: dict(real(f), csrc_sha=bench.csrc_sha()))

    class Ev:                                                  # stands in for a HIP event pair: elapsed_time in ms
        def __init__(self, ms):
            self.ms = ms

        def elapsed_time(self, other):
            return other.ms

    def launch(name, ints, ms):
        return (name, ints, Ev(0.0), Ev(ms))

    b2 = (200, 1, 400, 32, 2048, 16, 200, 200, 200, 400, 139520, 0, 0)
    b3 = (152, 0, 0, 32, 2048, 16, 150, 200, 200, 0, 139520, 150, 152)
    rnn = (4, 3, 14, 736, 250, 3500, 250, 2782080, 3780, 252, 2760000, 184000, 10304000, 736000, 10304000, 14000, 1000)
    rec = [launch('gpe_rnn_seq_bwd', rnn, 1.0), launch('gpe_edge_mlp_bwd', b2, 0.42), launch('gpe_edge_mlp_bwd', b2, 0.42),
           launch('gpe_edge_mlp_bwd', b3, 0.39), launch('gpe_edge_mlp_bwd', b3, 0.39)]
    args = types.SimpleNamespace(math='f16x3', batch=32, points=2048, k=16)
    roof, per_kernel, step = bench.roofline_tables(rec, 1, args, 10e-3, 32768)
    assert next(iter(per_kernel)) == 'gpe_rnn_seq_bwd'         # the sequence has the most time per step ...
    assert roof['kernel'] == 'gpe_edge_mlp_bwd:gather'          # ... the dominant KERNEL is the gathered backward
    assert roof['largest_sequence']['entry'] == 'gpe_rnn_seq_bwd'
    assert roof['bound'] == 'hbm' and roof['traffic_source'].startswith('profiles/') and 1.8e9 < roof['traffic'] < 2.3e9
    # frac prices the ALGORITHMIC bytes (dz2 in + dz1 out + the [P|Q] table + the indices), the counter traffic is
    # reported beside it as hbm_util / refetch
    alg = 32 * 2048 * 16 * (200 * 4 + 200 * 4 + 4) + 32 * 2048 * 2 * 200 * 4
    assert abs(roof['algorithmic_bytes_per_launch'] - alg) < 1 and abs(roof['frac'] - alg / 0.42e-3 / 8e12) < 1e-6
    assert abs(roof['achieved'] - alg / 0.42e-3 / 1e9) < 1e-3
    assert abs(roof['hbm_util'] - roof['traffic'] / 0.42e-3 / 8e12) < 1e-6 and abs(roof['refetch'] - roof['traffic'] / alg) < 1e-9
    assert 'rocprof_avg_launch_ms' in roof
    for fam in ('gpe_edge_mlp_fwd:gather', 'gpe_edge_mlp_fwd:dense', 'gpe_edge_mlp_bwd:inplace', 'gpe_edge_mlp_bwd:gather'):
        assert bench.pmc_traffic(fam, 2.0)[0] is not None, fam


def test_half_act_guard_host_side():
    """ops.HalfActGuard / set_half_act_guard without a GPU: mode switch, the amax bit pattern -> float conversion, copies and
    pickles of the owning module carry the decision and never the in-flight read."""
    import copy
    import pickle
    import numpy as np
    import torch
    from gpe_amd import ops, net_blocks
    prev = ops.set_half_act_guard('strict')
    try:
        assert ops.set_half_act_guard('off') == 'strict'
        g = ops.HalfActGuard()
        assert g.allow()                                        # 'off': never consulted
        ops.set_half_act_guard('fallback')
        assert g.allow() and not g.disabled                     # nothing pending
        with pytest.raises(ValueError):
            ops.set_half_act_guard('sometimes')
    finally:
        ops.set_half_act_guard(prev)
    bits = torch.tensor([int(np.array([70000.0], dtype=np.float32).view(np.int32)[0])], dtype=torch.int32)
    assert ops.HalfActGuard._value(bits) == 70000.0
    conv = net_blocks.DynamicEdgeConv(net_blocks.MLP([6, 8, 8, 8]), k=4)
    conv.half_act_guard.disabled = True
    conv.half_act_guard._pending = (object(), object())         # an in-flight read must not travel
    c2 = copy.deepcopy(conv)
    assert c2.half_act_guard.disabled and c2.half_act_guard._pending is None and c2.half_act_guard is not conv.half_act_guard
    g3 = pickle.loads(pickle.dumps(conv.half_act_guard))
    assert g3.disabled and g3._pending is None


def test_side_lanes_are_per_device():
    """streams.lane: one lane per device ordinal, sharing no flag and no job list — and building one touches no device (there is
    none here): the stream itself is created on first use."""
    from gpe_amd import streams
    a, b = streams.lane(0), streams.lane(1)
    assert a is streams.lane(0) and a is not b and (a.index, b.index) == (0, 1)
    assert a.stream is None and b.stream is None
    a.dirty = a.queued = True
    a.jobs.append('job')
    try:
        assert not b.dirty and not b.queued and b.jobs == [] and b.jobs is not a.jobs
    finally:
        a.dirty = a.queued = False
        del a.jobs[:]

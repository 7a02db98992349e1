"""Drop-in for the reference's nn/nets.py: same class names (resolved with getattr from the YAML, nn/train.py:120,
nn/experiment.py:232), constructor signature `(data_config, config={}, in_loss_config={})`, merged `.config`,
`forward(positions_batch, **kwargs) -> dict`, `.loss(preds, gt, epoch=)`, parameter/buffer names and shapes."""
import torch
import torch.nn as nn

from . import net_blocks as blocks
from . import ops
from .metrics import ComposedLoss, ComposedPatternLoss
from .patterns import DecodedPatterns


class BaseModule(nn.Module):
    """nn/nets.py:11-37."""

    def __init__(self):
        super().__init__()
        self.config = {'loss': 'MSELoss', 'model': self.__class__.__name__}
        self.regression_loss = nn.MSELoss()

    def loss(self, preds, ground_truth, **kwargs):
        ground_truth = ground_truth.to(preds.device)
        loss = self.regression_loss(preds, ground_truth)
        return loss, {'regression loss': loss}, False

    def train(self, mode=True):
        super().train(mode)
        if isinstance(self.loss, object):
            self.loss.train(mode)
        return self

    # ---- weight-derived kernel operands (ops.PackPlan): one refresh launch per optimizer step ----------------
    def _pack_modules(self):
        return [m for m in self.children() if hasattr(m, 'register_packs')]

    def _register_own_packs(self, plan):
        pass

    def refresh_packs(self):
        plan = self.__dict__.get('_pack_plan')
        if plan is None:
            plan = ops.PackPlan()
            for m in self._pack_modules():
                m.register_packs(plan)
            self._register_own_packs(plan)
            self.__dict__['_pack_plan'] = plan
        plan.refresh()

    def eval(self):
        super().eval()
        if isinstance(self.loss, object):
            self.loss.eval()
        return self

    def predict(self, positions_batch, route='auto', **kwargs):
        """forward's output dict at prediction time (an addition to the reference's class surface; its users call model.eval() and
        forward under no_grad: nn/evaluation_scripts/predict_per_example.py, on_test_set.py): nothing recorded for autograd, an
        EdgeConvFeatures encoder on its prediction path (route 'fused' / 'layers' / 'auto': ops.edge_conv_predict), everything
        behind the encoder on its existing forward kernels."""
        if route not in ops.EDGE_PREDICT_ROUTES:
            raise ValueError('unknown route %r (choose from %s)' % (route, ops.EDGE_PREDICT_ROUTES))
        if self.training:
            raise RuntimeError('%s.predict is a prediction path: call .eval() first (BatchNorm running statistics)'
                               % self.__class__.__name__)
        with torch.no_grad():
            return self._predict(positions_batch, route, **kwargs)

    def _predict(self, positions_batch, route, **kwargs):
        return self.forward(positions_batch, **kwargs)

    def predict_pattern(self, positions_batch, data_config, route='auto', stitches=None):
        """predict, then the step the reference runs on every prediction (Garment3DPatternFullDataset._pred_to_pattern,
        nn/data/datasets.py:731-767) on the device: ops.pattern_decode with data_config['standardize'] and
        data_config['explicit_stitch_tags'].  `stitches` [B,2,S] replace the pairing of the predicted stitch tags ("if somehow
        prediction already has an answer", :745).  -> patterns.DecodedPatterns; no host read before its as_spec / to_json."""
        if not self._predicts_patterns:
            raise NotImplementedError('%s.predict_pattern: the model predicts no panels (its stitches come from predict_stitches)'
                                      % self.__class__.__name__)
        return self._decode(self.predict(positions_batch, route=route), data_config, stitches)

    @staticmethod
    def _decode(preds, data_config, stitches=None):
        return DecodedPatterns(ops.pattern_decode(preds, data_config['standardize'],
                                                  bool(data_config.get('explicit_stitch_tags', False)), stitches=stitches))

    def predict_garment(self, positions_batch, data_config, stitch_model, stitch_data_stats, route='auto', **kw):
        """Both prediction stages on the device (the reference's evaluation_scripts/on_test_set.py and predict_per_example.py run the
        pattern model, build every pattern on the host and hand its 3D edges to the edge-pair classifier): predict_pattern, the
        panels placed in 3D (DecodedPatterns.place: ops.pattern_place), then stitch_model.predict_stitches on the placed edges
        (`stitch_model` a StitchOnEdge3DPairs in eval mode, `stitch_data_stats` its {'f_shift', 'f_scale'}; **kw are
        predict_stitches' keywords).  -> the DecodedPatterns with the classifier's answer attached as `pair_stitches`,
        `num_pair_stitches`, `pair_scores`; no host read before its as_spec(i, stitches='classifier') / to_json."""
        if stitch_model.training:
            raise RuntimeError('predict_garment runs the eval-mode stitch classifier: call .eval() on it first (the reference does, '
                               'pattern_converter.py:415)')
        d = self.predict_pattern(positions_batch, data_config, route=route).place()
        return d.attach_pair_stitches(stitch_model.predict_stitches(d.edges3d, d.num_edges, stitch_data_stats, **kw))

    def predict_scans(self, sampler, index, data_config, stitch_model=None, stitch_data_stats=None, route='auto', **kw):
        """Prediction from raw scans (the reference's evaluation_scripts/predict_per_example.py): sampler.sample(index) draws the
        model's clouds from the resident scans (`sampler` a staging.ScanSampler, `index` the scan of every batch slot), then
        predict_garment on them, or predict_pattern(...).place() without a stitch model.  -> the DecodedPatterns, with `scan_labels`
        (int32, resident-sized: the predicted panel of every point of the batch's scans, -1 elsewhere; sampler.labels) and
        `scan_picked` (int32 [B, N]: the drawn points) attached when the prediction carries `att_weights` (the attention model with
        the segmentation loss), both None otherwise.  No host read."""
        if not self._predicts_patterns:
            raise NotImplementedError('%s.predict_scans: the model predicts no panels' % self.__class__.__name__)
        if stitch_model is not None and stitch_model.training:
            raise RuntimeError('predict_scans runs the eval-mode stitch classifier: call .eval() on it first')
        features, picked = sampler.sample(index)
        preds = self.predict(features, route=route)
        d = self._decode(preds, data_config).place()
        if stitch_model is not None:
            d.attach_pair_stitches(stitch_model.predict_stitches(d.edges3d, d.num_edges, stitch_data_stats, **kw))
        att = preds.get('att_weights')
        d.scan_labels = sampler.labels(att) if att is not None else None
        d.scan_picked = picked if att is not None else None
        return d

    _predicts_patterns = False


# ---- GarmentFullPattern3D: what the reference's constructor fixes (nn/nets.py:49-130), as tables ------------------------------------
# attribute <- data_config key (nn/nets.py:53-57)
_DATA_FIELDS = (('panel_elem_len', 'element_size'), ('max_panel_len', 'max_panel_len'), ('max_pattern_size', 'max_pattern_len'),
                ('rotation_size', 'rotation_size'), ('translation_size', 'translation_size'))
# NN defaults (nn/nets.py:60-73); a *_hidden_size the caller left out falls back to the matching *_encoding_size IN THE CALLER'S DICT
# (nn/nets.py:75-78: configs saved before the hidden sizes existed)
_NN_DEFAULTS = {'panel_encoding_size': 250, 'panel_hidden_size': 250, 'panel_n_layers': 3,
                'pattern_encoding_size': 250, 'pattern_hidden_size': 250, 'pattern_n_layers': 2,
                'dropout': 0, 'lstm_init': 'kaiming_normal_', 'feature_extractor': 'EdgeConvFeatures',
                'panel_decoder': 'LSTMDecoderModule', 'pattern_decoder': 'LSTMDecoderModule', 'stitch_tag_dim': 3}
_HIDDEN_FALLBACK = (('panel_hidden_size', 'panel_encoding_size'), ('pattern_hidden_size', 'pattern_encoding_size'))
# loss defaults (nn/nets.py:83-92)
_LOSS_DEFAULTS = {'loss_components': ['shape', 'loop', 'rotation', 'translation'],
                  'quality_components': ['shape', 'discrete', 'rotation', 'translation'],
                  'loop_loss_weight': 1., 'stitch_tags_margin': 0.3, 'epoch_with_stitches': 40,
                  'stitch_supervised_weight': 0.1, 'stitch_hardnet_version': False, 'panel_origin_invariant_loss': True}


class GarmentFullPattern3D(BaseModule):
    """nn/nets.py:41-184: EdgeConv encoder -> pattern LSTM -> panel LSTM + placement Linear."""
    _predicts_patterns = True

    def __init__(self, data_config, config={}, in_loss_config={}):
        super().__init__()
        for attr, key in _DATA_FIELDS:
            setattr(self, attr, data_config[key])
        for hidden, enc in _HIDDEN_FALLBACK:                 # mutates the caller's dict (and raises KeyError when neither key is
            if hidden not in config:                         # given), like the reference
                config[hidden] = config[enc]
        self.config.update(_NN_DEFAULTS)
        self.config.update(config)
        self.loss = ComposedPatternLoss(data_config, {**{k: (list(v) if isinstance(v, list) else v) for k, v in _LOSS_DEFAULTS.items()},
                                                      **in_loss_config})
        self.config['loss'] = self.loss.config               # the loss object owns the merged dict from here on
        cfg = self.config
        extractor = getattr(blocks, cfg['feature_extractor'])
        if extractor is blocks.EdgeConvPoolingFeatures:
            # the block itself is usable (net_blocks.EdgeConvPoolingFeatures); the model is not: it returns one [B, out] tensor,
            # and the reference's forward_encode takes [0] of it (nn/nets.py:136) — the FIRST garment's encoding for the batch
            raise NotImplementedError('GarmentFullPattern3D with EdgeConvPoolingFeatures: the reference encodes every garment of '
                                      'a batch with the first garment\'s encoding (nn/nets.py:136 takes [0] of the block\'s '
                                      '[B, out] tensor); use EdgeConvFeatures with graph_pooling: True instead')
        self.feature_extractor = extractor(cfg['pattern_encoding_size'], cfg)
        cfg.update(getattr(self.feature_extractor, 'config', {}))
        # one row per sequence decoder: name, class key, output width, sequence length (`out_len` is swallowed by **kwargs in the
        # recurrent decoders and used by MLPDecoder: nn/net_blocks.py:273-298,365)
        for name, out_width, out_len in (('panel', self.panel_elem_len + cfg['stitch_tag_dim'] + 1, self.max_panel_len),
                                         ('pattern', cfg['panel_encoding_size'], self.max_pattern_size)):
            setattr(self, name + '_decoder', getattr(blocks, cfg[name + '_decoder'])(
                encoding_size=cfg[name + '_encoding_size'], hidden_size=cfg[name + '_hidden_size'], out_elem_size=out_width,
                n_layers=cfg[name + '_n_layers'], out_len=out_len, dropout=cfg['dropout'], custom_init=cfg['lstm_init']))
        self.placement_decoder = nn.Linear(cfg['panel_encoding_size'], self.rotation_size + self.translation_size)

    def forward_encode(self, positions_batch, route=None):
        """route (predict only): the EdgeConvFeatures encoder runs its prediction path"""
        if isinstance(self.feature_extractor, blocks.EdgeConvFeatures):
            if route is not None:
                return self.feature_extractor.predict(positions_batch, want_batch=False, route=route)[0]
            return self.feature_extractor(positions_batch, want_batch=False)[0]
        return self.feature_extractor(positions_batch)[0]

    def forward_pattern_decode(self, garment_encodings):
        panel_encodings = self.pattern_decoder(garment_encodings, self.max_pattern_size)
        return panel_encodings.contiguous().view(-1, panel_encodings.shape[-1])

    def _as_pattern(self, flat, last_dims):
        """[B * panels, ...] rows of a decoder -> [B, panels, *last_dims, -1] (views of ONE tensor per decoder, as in the reference)"""
        return flat.contiguous().view(-1, self.max_pattern_size, *last_dims, flat.shape[-1])

    def forward_panel_decode(self, flat_panel_encodings, batch_size):
        """nn/nets.py:143-169: per panel the edge sequence [edges][outline | stitch tag | free-edge logit] and the placement
        [rotation | translation]; the output dict slices those two tensors."""
        edges = self._as_pattern(self.panel_decoder(flat_panel_encodings, self.max_panel_len), (self.max_panel_len,))
        place = self._as_pattern(ops.linear(flat_panel_encodings, self.placement_decoder.weight, self.placement_decoder.bias), ())
        assert edges.shape[0] == batch_size
        e, r = self.panel_elem_len, self.rotation_size
        return {'outlines': edges[..., :e], 'rotations': place[..., :r], 'translations': place[..., r:],
                'stitch_tags': edges[..., e:-1], 'free_edges_mask': edges[..., -1]}

    def forward_decode(self, garment_encodings):
        flat_panel_encodings = self.forward_pattern_decode(garment_encodings)
        return self.forward_panel_decode(flat_panel_encodings, garment_encodings.size(0))

    def _register_own_packs(self, plan):
        plan.add_linear(self.placement_decoder.weight)

    def forward(self, positions_batch, **kwargs):
        self.refresh_packs()
        return self.forward_decode(self.forward_encode(positions_batch))

    def _predict(self, positions_batch, route, **kwargs):
        self.refresh_packs()
        return self.forward_decode(self.forward_encode(positions_batch, route=route))


class GarmentSegmentPattern3D(GarmentFullPattern3D):
    """nn/nets.py:187-299: per-point sparsemax attention over the EdgeConv features -> per-panel pooled encodings ->
    panel LSTM.  The per-panel Python loop of the reference is one reduce-GEMM per cloud here."""

    def __init__(self, data_config, config={}, in_loss_config={}):
        if 'loss_components' not in in_loss_config:     # mutates the caller's dict like the reference (:194-199)
            in_loss_config.update(loss_components=['shape', 'loop', 'rotation', 'translation'],
                                  quality_components=['shape', 'discrete', 'rotation', 'translation'])
        super().__init__(data_config, config, in_loss_config)
        self.save_att_weights = 'segmentation' in self.loss.config['loss_components']
        if self.save_att_weights and self.config.get('graph_pooling'):
            raise ValueError("the 'segmentation' loss term needs one attention weight per input point; graph_pooling: True "
                             "leaves the pooled points only — disable one of the two settings")
        if 'local_attention' not in self.config:
            self.config['local_attention'] = False
        attention_input_size = self.feature_extractor.config['EConv_feature']
        if not self.config['local_attention']:
            attention_input_size += self.config['pattern_encoding_size']
        if self.config['skip_connections']:
            attention_input_size += 3
        # parameter container with the reference's key layout: point_segment_mlp.0.{i}.{0,2}.* ; index 1 is the
        # parameter-free Sparsemax of the reference's Sequential
        self.point_segment_mlp = nn.Sequential(
            blocks.MLP([attention_input_size, attention_input_size, attention_input_size, self.max_pattern_size]),
            nn.Identity())
        panel_att_out_size = self.feature_extractor.config['EConv_feature']
        if self.config['skip_connections']:
            panel_att_out_size += 3
        self.panel_dec_lin = nn.Linear(panel_att_out_size, self.feature_extractor.config['panel_encoding_size'])
        del self.pattern_decoder

    def forward_panel_enc_from_3d(self, positions_batch, route=None):
        """route (predict only): the encoder runs its prediction path"""
        batch_size = positions_batch.shape[0]
        init_pattern_encodings, point_features_flat, batch = self.feature_extractor(
            positions_batch, not self.config['local_attention']) if route is None else self.feature_extractor.predict(
            positions_batch, not self.config['local_attention'], route=route)
        num_points = point_features_flat.shape[0] // batch_size
        point_features_flat = point_features_flat.contiguous()
        if self.config['local_attention']:
            att_in = point_features_flat
        else:
            glob = init_pattern_encodings.unsqueeze(1).repeat(1, num_points, 1).view(
                [-1, init_pattern_encodings.shape[-1]])
            att_in = torch.cat([glob, point_features_flat], dim=-1)
        logits = ops.dense_mlp(att_in, self.point_segment_mlp[0], self.training)
        points_weights = ops.SparsemaxFn.apply(logits)
        # "same pool as in initial extractor" (nn/nets.py:271-272): mean / max / add over the weighted features
        pooled = ops.AttentionPoolFn.apply(points_weights, point_features_flat, batch_size, num_points,
                                           self.feature_extractor.global_pool.pool_mode)
        panel_encodings = ops.linear(pooled, self.panel_dec_lin.weight, self.panel_dec_lin.bias)
        panel_encodings = panel_encodings.view(batch_size, -1, panel_encodings.shape[-1])
        points_weights = points_weights.view(batch_size, -1, points_weights.shape[-1]) \
            if self.save_att_weights else []
        return panel_encodings, points_weights

    def _register_own_packs(self, plan):
        plan.add_linear(self.placement_decoder.weight)
        plan.add_linear(self.panel_dec_lin.weight)
        blocks = [self.point_segment_mlp[0][i] for i in range(len(self.point_segment_mlp[0]))]
        plan.add_linear(blocks[0][0].weight)
        for b in blocks[1:]:
            plan.add_linear(b[0].weight, fwd=False, bwd=True)

    def forward(self, positions_batch, **kwargs):
        self.refresh_packs()
        batch_size = positions_batch.shape[0]
        panel_encodings, att_weights = self.forward_panel_enc_from_3d(positions_batch)
        panels = self.forward_panel_decode(panel_encodings.view(-1, panel_encodings.shape[-1]), batch_size)
        if len(att_weights) > 0:
            panels.update(att_weights=att_weights)
        return panels

    def _predict(self, positions_batch, route, **kwargs):
        self.refresh_packs()
        batch_size = positions_batch.shape[0]
        panel_encodings, att_weights = self.forward_panel_enc_from_3d(positions_batch, route=route)
        panels = self.forward_panel_decode(panel_encodings.view(-1, panel_encodings.shape[-1]), batch_size)
        if len(att_weights) > 0:
            panels.update(att_weights=att_weights)
        return panels


class StitchOnEdge3DPairs(BaseModule):
    """nn/nets.py:303-353: binary classifier on pairs of 3D edges — MLP([element_size, 200 x 3, 1]) on every pair row.
    The reference ships trained weights for it (models/att/neural_tailor_stitch_model.pth)."""

    def __init__(self, data_config, config={}, in_loss_config={}):
        super().__init__()
        self.pair_feature_len = data_config['element_size']
        self.config.update({'stitch_hidden_size': 200, 'stitch_mlp_n_layers': 3})
        self.config.update(config)
        self.config['loss'] = {
            'loss_components': ['edge_pair_class'],
            'quality_components': ['edge_pair_class', 'edge_pair_stitch_recall'],
            'panel_origin_invariant_loss': False, 'panel_order_inariant_loss': False}
        self.config['loss'].update(in_loss_config)
        self.loss = ComposedLoss(data_config, self.config['loss'])
        self.config['loss'] = self.loss.config
        mid_layers = [self.config['stitch_hidden_size']] * self.config['stitch_mlp_n_layers']
        self.mlp = blocks.MLP([self.pair_feature_len] + mid_layers + [1])

    def _register_own_packs(self, plan):
        mlp_blocks = [self.mlp[i] for i in range(len(self.mlp))]
        plan.add_linear(mlp_blocks[0][0].weight)
        for b in mlp_blocks[1:]:
            plan.add_linear(b[0].weight, fwd=False, bwd=True)

    def forward(self, pairs_batch, **kwargs):
        self.refresh_packs()
        self.device = pairs_batch.device
        self.batch_size = pairs_batch.size(0)
        return_shape = list(pairs_batch.shape)
        return_shape.pop(-1)
        out = ops.dense_mlp(pairs_batch.contiguous().view(-1, pairs_batch.shape[-1]), self.mlp, self.training)
        return out.view(return_shape)

    def predict_stitches(self, edges3d, num_edges, data_stats, **kw):
        """The model's prediction-time use (nn/data/pattern_converter.py:411-499: all_edge_pairs + stitches_from_pair_classifier):
        every cross-panel pair of the garments' 3D edges classified and, per edge, only the strongest positive kept — on the device,
        without materialising the pairs.  edges3d [B, P, L, element_size / 2] un-standardised edges per panel slot, num_edges [B, P];
        data_stats: {'f_shift', 'f_scale'} of the pair rows.  -> {'stitches', 'num_stitches', 'scores'[, 'logits']} (ops.stitch_pairs;
        keywords route=, return_logits=)."""
        if self.pair_feature_len % 2:
            raise ValueError('element_size must be even: a pair row is two edges (got %d)' % self.pair_feature_len)
        if self.training:
            raise RuntimeError('predict_stitches runs the eval-mode classifier: call .eval() first (the reference does, '
                               'pattern_converter.py:415)')
        return ops.stitch_pairs(edges3d, num_edges, self.mlp, data_stats['f_shift'], data_stats['f_scale'], **kw)

    def evaluate_stitches(self, edges3d, num_edges, gt_stitches, gt_num_stitches, data_stats, **kw):
        """predict_stitches scored against ground-truth stitches in the same pass: the reference's evaluation of this model over
        every edge pair of the garments (GarmentStitchPairsDataset with random_pairs_mode False -> self.loss), without the pair rows.
        gt_stitches integer [B, 2, S] edge ids panel * L + edge (either orientation), gt_num_stitches integer [B].
        -> (out, loss_dict): out = ops.stitch_pairs_eval's dict (keywords route=, return_logits=); loss_dict has the keys self.loss
        would produce for its configuration, pooled over the call, as fp32 device scalars (0 where a denominator is empty)."""
        if self.pair_feature_len % 2:
            raise ValueError('element_size must be even: a pair row is two edges (got %d)' % self.pair_feature_len)
        if self.training:
            raise RuntimeError('evaluate_stitches runs the eval-mode classifier: call .eval() first (the reference does, '
                               'pattern_converter.py:415)')
        out = ops.stitch_pairs_eval(edges3d, num_edges, self.mlp, data_stats['f_shift'], data_stats['f_scale'], gt_stitches,
                                    gt_num_stitches, **kw)
        m, loss_dict = out['metrics'], {}
        if 'edge_pair_class' in self.loss.l_components:
            loss_dict['edge_pair_class_loss'] = m['edge_pair_class_loss']
        if self.loss.with_quality_eval:
            if 'edge_pair_class' in self.loss.q_components:
                loss_dict['edge_pair_class_acc'] = m['edge_pair_class_acc']
            if 'edge_pair_stitch_recall' in self.loss.q_components:
                loss_dict['stitch_precision'] = m['stitch_precision']
                loss_dict['stitch_recall'] = m['stitch_recall']
        return out, loss_dict

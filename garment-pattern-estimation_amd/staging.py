"""Input side of a training step (reference: nn/trainer.py:93 `features = batch['features'].to(device)` from pageable
memory, after nn/data/transforms.py:35-50 standardised every sample on the CPU).

BatchStager keeps two pinned host buffers and a copy stream per device: batch i+1 is copied while step i computes, the
compute stream only waits on the copy's event, and the per-axis standardisation `(x - shift) / scale` runs as one kernel
on the device instead of per sample on the host.

StitchPairSampler is the input side of the edge-pair classifier's training (GarmentStitchPairsDataset with random_pairs_mode,
nn/data/datasets.py:985-1132): the data set's 3D edges and stitches stay in HBM and every step's pair rows are drawn there.

MeshPointSampler is the input side of the encoder / decoder step (Garment3DPatternFullDataset._get_sample_info): the data set's
meshes stay in HBM and every step's point clouds and segmentation labels are drawn there.

BalancedBatchSchedule and EpochFeeder make an epoch self-feeding (DatasetWrapper.new_loaders' BalancedBatchSampler,
nn/data/wrapper.py:78-89, nn/data/utils.py:16-92): which garments form every batch is drawn on the device once per epoch, the
garments' ground truth stays in HBM, and each step takes its index and ground-truth rows from there without a tensor from the host.

ScanSampler is the input side of prediction from raw scans (nn/evaluation_scripts/predict_per_example.py): point clouds of
arbitrary size stay in HBM and every call draws the model's clouds from them; its labels() hand the attention model's per-point panel
labels back to every point of a scan.

The statistics both training samplers standardise with are fitted on the device as well (fit_feature_stats of either sampler,
fit_pattern_standardization for the ground truth: the reference's standardize(training), nn/data/datasets.py:596-645, 1018-1041)."""
import numpy as np
import torch

from . import _lib as L
from . import ops
from . import streams


class BatchStager:
    def __init__(self, device, shift=None, scale=None, slots=2):
        self.device = torch.device(device)
        self.shift, self.scale = shift, scale
        self.up = streams.Uploader(self.device)
        self.slots, self.turn = slots, 0     # pinned slots, used round-robin

    def stage(self, features):
        """features: CPU tensor [B, N, C] (any float dtype) -> fp32 device tensor, standardised if stats were given."""
        if features.is_cuda:
            out = features.float()
        else:
            self.turn = (self.turn + 1) % self.slots
            out = self.up.upload(self.turn, features.shape, lambda buf: buf.copy_(features))
        if self.shift is not None:
            out = ops.standardize(out.view(-1, out.shape[-1]), self.shift, self.scale).view(out.shape)
        return out


def _fit_index(index, device):
    """the training garments of a statistics fit as an integer [G'] tensor on the device"""
    if not torch.is_tensor(index):
        index = torch.as_tensor(index)
    if index.dim() != 1 or index.numel() < 1 or index.is_floating_point() or index.is_complex() or index.dtype == torch.bool:
        raise ValueError('index must be an integer [G] tensor or sequence, G >= 1: the garments the statistics are fitted on')
    return index.to(device)


def _fit_chunk(chunk):
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError('chunk must be a positive integer: the garments drawn per launch (got %r)' % (chunk,))
    return chunk


def _fit_status_check(status, message):
    """the one host read of a fit's per-garment status words"""
    bad = (status.cpu() < 0).nonzero()
    if bad.numel():
        raise ValueError(message % int(bad[0]))


def fit_pattern_standardization(ground_truth, feature_stats):
    """The reference's config['standardize'] of a pattern-model experiment (Garment3DPatternFullDataset.standardize,
    nn/data/datasets.py:612-645), with the ground-truth statistics fitted on the device from the training garments' resident
    tensors: ground_truth = {'outlines' [G, P, L, E], 'rotations' [G, P, R], 'translations' [G, P, T], 'stitch_tags' [G, P, L, D]},
    fp32 on the device; feature_stats = {'f_shift', 'f_scale'} (MeshPointSampler.fit_feature_stats).
      outlines                                   mean / std over the un-padded edge rows, gt_shift['outlines'][0] = [1] = 0 (:618)
      rotations, translations, stitch_tags       min / norm_scale over all rows (zero is a valid value there)
    -> {'f_shift', 'f_scale', 'gt_shift': {...}, 'gt_scale': {...}} of fp32 numpy arrays, as MeshPointSampler.from_config,
    metrics.ComposedPatternLoss and ops.pattern_decode take it.  Four pairs of launches, then one host read per tensor."""
    keys = ('outlines', 'rotations', 'translations', 'stitch_tags')
    if not isinstance(ground_truth, dict) or any(k not in ground_truth for k in keys):
        raise ValueError('ground_truth must hold the device tensors %s' % (keys,))
    if not isinstance(feature_stats, dict) or any(k not in feature_stats for k in ('f_shift', 'f_scale')):
        raise ValueError("feature_stats must hold 'f_shift' and 'f_scale'")
    dims = {'outlines': 4, 'rotations': 3, 'translations': 3, 'stitch_tags': 4}
    G = None
    for k in keys:
        t = ground_truth[k]
        if not torch.is_tensor(t) or t.dim() != dims[k] or t.dtype != torch.float32 or not 1 <= t.shape[-1] <= ops.FIT_MAX_C or t.numel() < 1:
            raise ValueError('ground_truth[%r] must be an fp32 %d-dimensional tensor of 1 .. %d columns (got %s %s)'
                             % (k, dims[k], ops.FIT_MAX_C, getattr(t, 'dtype', type(t).__name__), tuple(getattr(t, 'shape', ()))))
        G = t.shape[0] if G is None else G
        if t.shape[0] != G:
            raise ValueError('the ground-truth tensors hold %d and %d garments' % (G, t.shape[0]))
    blocks = {}
    for k in keys:                                    # every launch first, the host reads after
        t = ground_truth[k].detach()
        x = t.reshape(G, -1, t.shape[-1])
        acc = ops.FitAccumulator(x.shape[2], G, x.shape[1], x.device, padded=(k == 'outlines'))
        acc.add(x)
        blocks[k] = acc.finish()
    f32 = lambda v: torch.as_tensor(v).detach().cpu().numpy().astype('float32')        # noqa: E731
    out = {'f_shift': f32(feature_stats['f_shift']), 'f_scale': f32(feature_stats['f_scale']), 'gt_shift': {}, 'gt_scale': {}}
    for k in keys:
        r = ops.fit_read(blocks[k])
        out['gt_shift'][k], out['gt_scale'][k] = (r['mean'], r['std']) if k == 'outlines' else (r['min'], r['norm_scale'])
    # the mean of the edge vectors is zero by the loop property, and shifting them would break it (:616-618)
    out['gt_shift']['outlines'][:2] = 0
    return out


class StitchPairSampler:
    """Fresh training pairs of the stitch classifier for every step, drawn on the device from a resident data set: what
    GarmentStitchPairsDataset._get_sample_info (nn/data/datasets.py:1119-1122: NNSewingPattern.stitches_as_3D_pairs, then
    FeatureStandartization) gives per garment, for a whole batch in one launch (ops.stitch_pairs_sample) and without host work.  The
    keyword names and defaults are those of the data set's config.

    edges3d [G, P, L, Fe] fp32, num_edges [G, P], gt_stitches [G, 2, S] (edge ids panel * L + edge), gt_num_stitches [G]: the layout
    StitchOnEdge3DPairs.evaluate_stitches takes; data_stats: {'f_shift', 'f_scale'} of the pair rows, or None for a new experiment:
    sample() then raises until fit_feature_stats(index) has fitted them on the device (or f_shift / f_scale are set).

        sampler = StitchPairSampler(edges3d, num_edges, gt_stitches, gt_num_stitches, stats)
        sg = graph.StepGraph(lambda idx: (lambda r, y: model.loss(model(r), y)[:2])(*sampler.sample(idx)), opt)
        loss = sg.step(index)               # index: the garments of the batch, an integer [B] tensor

    The sampler owns the resident tensors, the generator state {seed, draw} (`.state`, int64 [2] on the device: every call of
    sample() advances draw by one on the device, so a captured call draws new pairs on every replay) and the kernel's ticket word.
    `.status` is the int32 [B] status of the last call (>= 0 rows that gave up, -1 more stitches than stitched_edge_pairs_num, -2 an
    index outside the set).  reseed(seed, draw) restarts the sequence: the draws are a function of (seed, draw, batch slot, data)."""

    def __init__(self, edges3d, num_edges, gt_stitches, gt_num_stitches, data_stats, stitched_edge_pairs_num=200,
                 non_stitched_edge_pairs_num=200, shuffle_pairs=True, shuffle_pairs_order=True, seed=0):
        self.edges3d, self.num_edges, self.gt_stitches, self.gt_num_stitches = ops.stitch_sample_resident(
            edges3d, num_edges, gt_stitches, gt_num_stitches)
        self.f_shift = [float(v) for v in data_stats['f_shift']] if data_stats else None
        self.f_scale = [float(v) for v in data_stats['f_scale']] if data_stats else None
        self.stitched_edge_pairs_num = int(stitched_edge_pairs_num)
        self.non_stitched_edge_pairs_num = int(non_stitched_edge_pairs_num)
        self.shuffle_pairs, self.shuffle_pairs_order = bool(shuffle_pairs), bool(shuffle_pairs_order)
        self.device = self.edges3d.device
        self.state = ops.stitch_sample_state(seed, 0, self.device)
        self.ticket = torch.zeros(1, device=self.device, dtype=torch.int32)
        self.status = None

    @classmethod
    def from_config(cls, edges3d, num_edges, gt_stitches, gt_num_stitches, dataset_config, seed=0):
        """dataset_config: the 'dataset' dict of a stitch-model experiment (its 'standardize' statistics are required)"""
        keys = ('stitched_edge_pairs_num', 'non_stitched_edge_pairs_num', 'shuffle_pairs', 'shuffle_pairs_order')
        return cls(edges3d, num_edges, gt_stitches, gt_num_stitches, dataset_config['standardize'], seed=seed,
                   **{k: dataset_config[k] for k in keys if k in dataset_config})

    def reseed(self, seed, draw=0):
        """the next call draws with (seed, draw); a copy queued on the current stream, no device read"""
        self.state.copy_(ops.stitch_sample_state(seed, draw, 'cpu'), non_blocking=False)

    def sample(self, index):
        """index: integer [B] tensor on the device -> (rows fp32 [B, R, 2 Fe], labels bool [B, R])"""
        if self.f_shift is None:
            raise RuntimeError('StitchPairSampler was built without statistics (data_stats=None): call fit_feature_stats(index) '
                               'or set f_shift / f_scale before sample()')
        rows, labels, self.status = ops.stitch_pairs_sample(
            self.edges3d, self.num_edges, self.gt_stitches, self.gt_num_stitches, index, self.stitched_edge_pairs_num,
            self.non_stitched_edge_pairs_num, self.f_shift, self.f_scale, self.state, self.ticket, self.shuffle_pairs,
            self.shuffle_pairs_order)
        return rows, labels

    def fit_feature_stats(self, index, seed=0, chunk=256, install=True):
        """The pair rows' statistics of a new experiment, fitted on the device: what GarmentStitchPairsDataset.standardize(training)
        (nn/data/datasets.py:1034: _get_norm_stats of one sample per training garment) computes on the host.  Draws the rows of
        every garment of `index` (an integer [G'] tensor or sequence) with shift 0 / scale 1 and the sampler's own settings, `chunk`
        garments per launch, and accumulates them (ops.FitAccumulator).
        -> {'f_shift': min, 'f_scale': norm_scale} as fp32 numpy [2 Fe]; with `install` they become the sampler's own statistics.

        The draws come from a generator state of their own, (seed, 0) advanced once per chunk; the sampler's `.state` is left as it
        was.  The result is a function of (seed, chunk, index, data).  A garment whose status is negative (-1 more stitches than
        stitched_edge_pairs_num, -2 outside the set) raises after the last chunk: one host read at the end, none per chunk."""
        index, chunk = _fit_index(index, self.device), _fit_chunk(chunk)
        G, C = index.numel(), 2 * self.edges3d.shape[3]
        R = self.stitched_edge_pairs_num + self.non_stitched_edge_pairs_num
        acc = ops.FitAccumulator(C, G, R, self.device)
        state = ops.stitch_sample_state(seed, 0, self.device)
        status = []
        for g0 in range(0, G, chunk):
            rows, _, st = ops.stitch_pairs_sample(
                self.edges3d, self.num_edges, self.gt_stitches, self.gt_num_stitches, index[g0:g0 + chunk],
                self.stitched_edge_pairs_num, self.non_stitched_edge_pairs_num, [0.0] * C, [1.0] * C, state, self.ticket,
                self.shuffle_pairs, self.shuffle_pairs_order)
            acc.add(rows)
            status.append(st)
        result = acc.finish()
        _fit_status_check(torch.cat(status), 'fit_feature_stats: garment %d of the index has more stitches than '
                                             'stitched_edge_pairs_num or lies outside the set')
        r = ops.fit_read(result)
        stats = {'f_shift': r['min'], 'f_scale': r['norm_scale']}
        if install:
            self.f_shift, self.f_scale = [float(v) for v in stats['f_shift']], [float(v) for v in stats['f_scale']]
        return stats


class MeshPointSampler:
    """Fresh input point clouds of the pattern model for every step, drawn on the device from resident meshes: what
    Garment3DPatternFullDataset._get_sample_info (nn/data/datasets.py: _sample_points with its optional Gaussian noise,
    _point_classes_from_mesh, FeatureStandartization) gives per garment on the host, for a whole batch in at most two launches
    (ops.mesh_points_sample).  The reference keeps ONE cached sample per garment for a whole run; here every call is a new draw.
    The keyword names and defaults are those of the data set's config.

    meshes: a list of (verts [V, 3], faces [F, 3], labels [V]) per garment (labels: the class id of every vertex, -1 for a stitch /
    None vertex), or an ops.mesh_resident(...) built from one; data_stats: {'f_shift', 'f_scale'} of the points, or None.

        sampler = MeshPointSampler(meshes, stats, mesh_samples=2000)
        sg = graph.StepGraph(lambda idx, gt: model.loss(model(sampler.sample(idx)[0]), gt)[:2], opt)
        loss = sg.step(index, gt)           # index: the garments of the batch, an integer [B] tensor

    The sampler owns the resident set, the generator state {seed, draw} (`.state`, int64 [2] on the device: every call of sample()
    advances draw by one on the device, so a captured call draws new clouds on every replay) and the kernel's ticket word.
    `.status` is the int32 [B] status of the last call (>= 0 points that fell back to label 0 because their cloud has no labelled
    point, -1 a garment without a face of positive area, -2 an index outside the set).  reseed(seed, draw) restarts the sequence:
    the draws are a function of (seed, draw, batch slot, data)."""

    def __init__(self, meshes, data_stats=None, mesh_samples=2000, point_noise_w=0, seed=0):
        self.resident = ops.mesh_resident(meshes)
        self.f_shift = [float(v) for v in data_stats['f_shift']] if data_stats else None
        self.f_scale = [float(v) for v in data_stats['f_scale']] if data_stats else None
        self.mesh_samples, self.point_noise_w = int(mesh_samples), float(point_noise_w)
        self.device = self.resident.device
        if not self.resident.verts4.is_cuda:
            raise RuntimeError('gpe ops need tensors on the MI355X (got a %s resident set); there is no CPU path' % self.device)
        self.state = ops.stitch_sample_state(seed, 0, self.device)
        self.ticket = torch.zeros(1, device=self.device, dtype=torch.int32)
        self.status = None

    @classmethod
    def from_config(cls, meshes, dataset_config, seed=0):
        """dataset_config: the 'dataset' dict of a pattern-model experiment ('mesh_samples', 'point_noise_w', 'standardize')"""
        keys = ('mesh_samples', 'point_noise_w')
        return cls(meshes, dataset_config.get('standardize'), seed=seed, **{k: dataset_config[k] for k in keys if k in dataset_config})

    def reseed(self, seed, draw=0):
        """the next call draws with (seed, draw); a copy queued on the current stream, no device read"""
        self.state.copy_(ops.stitch_sample_state(seed, draw, 'cpu'), non_blocking=False)

    def sample(self, index):
        """index: integer [B] tensor on the device -> (features fp32 [B, mesh_samples, 3], segmentation int64 [B, mesh_samples])"""
        features, segmentation, self.status = ops.mesh_points_sample(
            self.resident, index, self.mesh_samples, self.state, self.ticket, self.point_noise_w, self.f_shift, self.f_scale)
        return features, segmentation

    def fit_feature_stats(self, index, seed=0, chunk=256, install=True):
        """The feature statistics of a new experiment, fitted on the device: what Garment3DPatternFullDataset.standardize(training)
        (nn/data/datasets.py:612: _get_distribution_stats of one sample per training garment) computes on the host.  Draws one
        unstandardised cloud (the sampler's mesh_samples and point_noise_w) per garment of `index` (an integer [G'] tensor or sequence:
        the training garments), `chunk` garments per launch into one reused buffer, and accumulates them (ops.FitAccumulator).
        -> {'f_shift': mean, 'f_scale': std} as fp32 numpy [3]; with `install` they become the sampler's own statistics.

        The draws come from a generator state of their own, (seed, 0) advanced once per chunk; the sampler's `.state` is left as it
        was.  The result is a function of (seed, chunk, index, data) — bit-identical for every grid size and CU reservation.  A
        garment whose status is negative (-1 no face of positive area, -2 outside the set) raises after the last chunk: there is
        one host read at the end and none per chunk."""
        index, chunk = _fit_index(index, self.device), _fit_chunk(chunk)
        G, N = index.numel(), self.mesh_samples
        acc = ops.FitAccumulator(3, G, N, self.device)
        state = ops.stitch_sample_state(seed, 0, self.device)
        buffers = ops.mesh_points_buffers(self.resident, min(chunk, G), N)
        status = torch.empty(G, device=self.device, dtype=torch.int32)
        for g0 in range(0, G, chunk):
            b = min(chunk, G - g0)
            out = tuple(t[:b] if t is not None else None for t in buffers[:2] + buffers[3:])
            out = (out[0], out[1], status[g0:g0 + b], out[2])
            ops.mesh_points_sample(self.resident, index[g0:g0 + b], N, state, self.ticket, self.point_noise_w, None, None, out=out)
            acc.add(out[0])
        result = acc.finish()
        _fit_status_check(status, 'fit_feature_stats: garment %d of the index has no face of positive area or lies outside the set')
        r = ops.fit_read(result)
        stats = {'f_shift': r['mean'], 'f_scale': r['std']}
        if install:
            self.f_shift, self.f_scale = [float(v) for v in stats['f_shift']], [float(v) for v in stats['f_scale']]
        return stats


def load_scan_points(path):
    """a scan from a .txt file: the first three numbers of every line are a point (load_points of the reference's
    nn/evaluation_scripts/predict_per_example.py; blank lines are skipped, a line with fewer than three numbers is a ValueError)
    -> float64 [n, 3]"""
    points = []
    with open(path, 'r') as f:
        for no, line in enumerate(f, 1):
            coords = [float(x) for x in line.split()]
            if not coords:
                continue
            if len(coords) < 3:
                raise ValueError('%s:%d: a point needs three numbers (got %d)' % (path, no, len(coords)))
            points.append(coords[:3])
    return np.asarray(points, dtype=np.float64).reshape(-1, 3)


class ScanSampler:
    """The pattern model's input clouds drawn on the device from raw scans that stay in HBM: what the reference's
    nn/evaluation_scripts/predict_per_example.py does per scan on the host (np.random.permutation(n)[:mesh_samples], :137-141,
    FeatureStandartization, :143-144, stack), for a whole batch in one call (ops.cloud_points_sample) and as often as the caller
    likes: several draws per scan show how stable a prediction is.  It mirrors MeshPointSampler.

    clouds: a list of [n, 3] arrays (load_scan_points reads the reference's .txt files), or an ops.cloud_resident(...) built from
    one; data_stats: {'f_shift', 'f_scale'} of the points, or None.

        sampler = ScanSampler([load_scan_points(p) for p in paths], stats, mesh_samples=2000)
        patterns = model.predict_scans(sampler, index, data_config, stitch_model, stitch_stats)

    The sampler owns the resident set, the generator state {seed, draw} (`.state`, int64 [2] on the device: every call of sample()
    advances draw by one on the device, so a captured call draws new clouds on every replay), the kernel's ticket word and its
    workspace.  `.status` is the int32 [B] status of the last call (N - n repeated rows of a scan of n < N points, 0 otherwise; -1 an
    empty scan, -2 an index outside the set).  reseed(seed, draw) restarts the sequence: the draws are a function of (seed, draw,
    batch slot, data).  labels(att_weights) hands the attention model's per-point panel labels of the last sample back to every
    point of its scans."""

    def __init__(self, clouds, data_stats=None, mesh_samples=2000, seed=0):
        self.resident = ops.cloud_resident(clouds)
        self.f_shift = [float(v) for v in data_stats['f_shift']] if data_stats else None
        self.f_scale = [float(v) for v in data_stats['f_scale']] if data_stats else None
        self.mesh_samples = int(mesh_samples)
        self.device = self.resident.device
        if not self.resident.points4.is_cuda:
            raise RuntimeError('gpe ops need tensors on the MI355X (got a %s resident set); there is no CPU path' % self.device)
        self.state = ops.stitch_sample_state(seed, 0, self.device)
        self.ticket = torch.zeros(1, device=self.device, dtype=torch.int32)
        self.status = self.index = self.picked = None

    @classmethod
    def from_config(cls, clouds, dataset_config, seed=0):
        """dataset_config: the 'dataset' dict of a pattern-model experiment ('mesh_samples', 'standardize')"""
        keys = ('mesh_samples',)
        return cls(clouds, dataset_config.get('standardize'), seed=seed, **{k: dataset_config[k] for k in keys if k in dataset_config})

    def reseed(self, seed, draw=0):
        """the next call draws with (seed, draw); a copy queued on the current stream, no device read"""
        self.state.copy_(ops.stitch_sample_state(seed, draw, 'cpu'), non_blocking=False)

    def sample(self, index):
        """index: integer [B] tensor on the device -> (features fp32 [B, mesh_samples, 3], picked int32 [B, mesh_samples])"""
        features, self.picked, self.status = ops.cloud_points_sample(
            self.resident, index, self.mesh_samples, self.state, self.ticket, self.f_shift, self.f_scale)
        self.index = index
        return features, self.picked

    def labels(self, att_weights, out=None):
        """att_weights fp32 [B, mesh_samples, P] of a prediction on the last sample -> int32 [T], resident-sized: the panel of every
        point of the scans of that batch (ops.cloud_labels), -1 on the scans outside it"""
        if self.picked is None:
            raise RuntimeError('ScanSampler.labels hands back the labels of the last sample: call sample(index) first')
        return ops.cloud_labels(self.resident, self.index, self.picked, att_weights, out=out)


def balanced_quotas(sizes, batch_size):
    """the garments of every type in a balanced batch, in the reference's own expression (nn/data/utils.py:48): int((len_c / G) *
    batch_size), evaluated in double.  It is not len_c * batch_size // G: 13 of 23 garments at batch_size = 23 give 12."""
    G = sum(sizes)
    return [int((n / G) * batch_size) for n in sizes]


class BalancedBatchSchedule:
    """The batches of a training epoch drawn on the device: what BalancedBatchSampler (nn/data/utils.py:16-92) yields, restated as
    a function of (seed, epoch, class lists, quotas, batch_size, drop_last) alone (include/gpe_hip_feed.h).  Every batch holds the
    quota of every garment type (balanced_quotas), the free slots take garments of types chosen uniformly among those that still
    have some, the slots of a batch are shuffled, and no garment appears twice in an epoch.

    ids_by_type: {type: integer sequence or tensor of garment ids}, as the reference's constructor takes it; more types than
    batch_size is the same NotImplementedError; len() is the same number of batches.

        schedule = BalancedBatchSchedule(ids_by_type, 30)
        schedule.draw()                     # three launches, no host read: the next epoch's table
        rows = schedule.host_table()        # the one host read, for logging and tests

    `.table` int32 [len(), batch_size] (a kept remainder is padded with -1), `.batch_len` int32 [len()], `.state` int64 [2] =
    {seed, epoch} (every draw() advances epoch by one on the device) and `.cursor` int64 [1] (the row ops.feed_next takes next) are
    static device tensors.  reseed(seed, epoch) restarts the sequence."""

    def __init__(self, ids_by_type, batch_size, drop_last=True, seed=0, device='cuda'):
        if len(ids_by_type) > batch_size:
            raise NotImplementedError('BalancedBatchSchedule: creating batches that are smaller than the number of garment types '
                                      'is not implemented (%d types, batch_size = %d)' % (len(ids_by_type), batch_size))
        lists = [np.asarray(v.detach().cpu() if torch.is_tensor(v) else v).reshape(-1) for v in ids_by_type.values()]
        if not lists or any(l.size and l.dtype.kind not in 'iu' for l in lists):
            raise ValueError('ids_by_type must map at least one type to integer garment ids')
        lists = [l.astype(np.int64) for l in lists]
        sizes = [int(l.size) for l in lists]
        G = sum(sizes)
        self.class_names = list(ids_by_type.keys())
        self.batch_size, self.data_size = int(batch_size), G
        rows = L.query('gpe_batch_schedule_rows', G, self.batch_size, 1 if drop_last else 0)
        if rows < 0:
            raise ValueError('BalancedBatchSchedule handles 1 .. 2^20 garments in batches of 1 .. 1024 (got %d, batch_size = %d)'
                             % (G, batch_size))
        if rows == 0:
            raise ValueError('the %d garments do not fill one batch of %d and drop_last leaves none' % (G, batch_size))
        ids = np.concatenate(lists)
        if ids.min() < 0 or ids.max() >= 1 << 31:
            raise ValueError('garment ids are integers in 0 .. 2^31 - 1')
        self.num_full_batches = G // self.batch_size
        self.drop_last = bool(drop_last) or G % self.batch_size == 0
        self.quotas = balanced_quotas(sizes, self.batch_size)
        if sum(self.quotas) > self.batch_size:
            raise ValueError('the per-type batch lengths %s exceed batch_size = %d' % (self.quotas, batch_size))
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('gpe ops need tensors on the MI355X (got device %s); there is no CPU path' % self.device)
        self._class_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self._quota = np.asarray(self.quotas, dtype=np.int32)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)          # noqa: E731
        self.class_off, self.ids, self.quota = to(self._class_off), to(ids.astype(np.int32)), to(self._quota)
        self.table = torch.full((rows, self.batch_size), -1, device=self.device, dtype=torch.int32)
        self.batch_len = torch.zeros(rows, device=self.device, dtype=torch.int32)
        self.state = ops.stitch_sample_state(seed, 0, self.device)
        self.cursor = torch.zeros(1, device=self.device, dtype=torch.int64)
        self.ws = torch.empty(L.query('gpe_batch_schedule_ws_bytes', G), device=self.device, dtype=torch.uint8)

    def __len__(self):
        return self.num_full_batches + (not self.drop_last)

    def reseed(self, seed, epoch=0):
        """the next draw() uses (seed, epoch); a copy queued on the current stream, no device read"""
        self.state.copy_(ops.stitch_sample_state(seed, epoch, 'cpu'), non_blocking=False)

    def draw(self):
        """queues the next epoch's table on the current stream (three launches); no host read"""
        ops.batch_schedule_draw(self.class_off, self.ids, self.quota, self._class_off, self._quota, self.batch_size, self.drop_last,
                                self.state, self.ws, self.table, self.batch_len)

    def host_table(self):
        """-> the table of the last draw() as a CPU int32 [len(), batch_size] tensor (-1 pads a kept remainder): the one host read"""
        return self.table.cpu()


class EpochFeeder:
    """The inputs of every step of an epoch taken from device memory: the next row of a BalancedBatchSchedule becomes the step's
    index, the ground truth of its garments is gathered from resident tables (ops.feed_next, two launches), and the sampler draws
    the batch's clouds or pair rows from that index.  Nothing comes from the host, so a captured step feeds itself at every replay:

        feeder = EpochFeeder(schedule, sampler, ground_truth)
        sg = graph.StepGraph(lambda: model.loss(model(feeder.next()[0]), feeder.last_gt)[0], opt)
        for epoch in ...:
            feeder.begin_epoch()
            for _ in range(len(feeder)):
                loss = sg.step()

    ground_truth: {name: tensor [G, ...]} whose leading dimension is the garment (outlines, num_edges, rotations, translations,
    num_panels, empty_panels_mask, num_stitches, stitches, free_edges_mask, stitch_tags, or whatever the caller's loss reads), 16
    at the most.  They are made resident and contiguous once and stored as given: whether to standardise them is the caller's
    choice.  A table whose rows are not a multiple of 4 bytes (a bool mask of 23 panels) is kept with padded rows, and its batch is a
    strided view of the padded output.

    next() -> (features, gt) for a MeshPointSampler, gt = the gathered batch with the sampler's `segmentation` added, or (rows,
    labels) for a StitchPairSampler; `.last_gt` is the gathered batch either way, `.index` the int32 [B] index (the dtype the
    samplers take without a conversion launch) and `.status` int32 [1] the entries of the last row outside 0 .. G - 1, whose
    ground-truth rows are zeros.  Every output of the feeder is a static buffer that the next call overwrites.
    begin_epoch() draws the schedule and zeroes the cursor on the current stream; len() is the steps per epoch.  A schedule that
    keeps a short last row is a ValueError: a captured step has one shape."""

    def __init__(self, schedule, sampler, ground_truth=None):
        if len(schedule) != schedule.num_full_batches:
            raise ValueError('EpochFeeder needs a schedule of full batches (drop_last=True): the last of these %d rows holds %d of '
                             '%d garments, and a captured step has one shape' % (len(schedule), schedule.data_size % schedule.batch_size,
                                                                                  schedule.batch_size))
        self.schedule, self.sampler = schedule, sampler
        self.device, B = schedule.device, schedule.batch_size
        ground_truth = dict(ground_truth or {})
        G = None
        for k, t in ground_truth.items():
            if not torch.is_tensor(t) or t.dim() < 1 or t.shape[0] < 1 or t[0].numel() < 1:
                raise ValueError('ground_truth[%r] must be a tensor whose leading dimension is the garment' % (k,))
            G = t.shape[0] if G is None else G
            if t.shape[0] != G:
                raise ValueError('the ground-truth tensors hold %d and %d garments' % (G, t.shape[0]))
        if G is None:                                     # no table: the set is the sampler's
            G = sampler.resident.G if hasattr(sampler, 'resident') else sampler.edges3d.shape[0]
        self.G = int(G)
        self.resident, self.gt, outputs = {}, {}, []
        for k, t in ground_truth.items():
            t = t.detach().to(self.device).contiguous()
            nb = t[0].numel() * t.element_size()
            if nb % 4 == 0:
                out = torch.zeros((B,) + tuple(t.shape[1:]), device=self.device, dtype=t.dtype)
                self.gt[k] = out
            else:                                         # rows padded to 4 bytes; the batch is a view of the padded output
                pad = torch.zeros(self.G, (nb + 3) // 4 * 4, device=self.device, dtype=torch.uint8)
                pad[:, :nb] = t.reshape(self.G, -1).view(torch.uint8)
                out = torch.zeros(B, pad.shape[1], device=self.device, dtype=torch.uint8)
                self.gt[k] = out[:, :nb].view(t.dtype).view((B,) + tuple(t.shape[1:]))
                t = pad
            self.resident[k] = t
            outputs.append(out)
        self.jobs, self.max_row_bytes = ops.feed_jobs(list(self.resident.values()), outputs) if outputs else (None, 0)
        self.outputs = outputs
        self.index = torch.full((B,), -1, device=self.device, dtype=torch.int32)
        self.status = torch.zeros(1, device=self.device, dtype=torch.int32)
        self.last_gt = self.gt

    def __len__(self):
        return self.schedule.num_full_batches

    def begin_epoch(self):
        """draws the next epoch's schedule and zeroes the cursor, on the current stream; no host read"""
        self.schedule.draw()
        self.schedule.cursor.zero_()

    def next(self):
        """the next batch: see the class"""
        ops.feed_next(self.schedule.table, self.schedule.cursor, self.G, self.jobs, self.max_row_bytes, self.index, self.status)
        out = self.sampler.sample(self.index)
        if isinstance(self.sampler, StitchPairSampler):
            self.last_gt = self.gt
            return out
        features, segmentation = out
        self.last_gt = dict(self.gt, segmentation=segmentation)
        return features, self.last_gt

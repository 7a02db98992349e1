"""Input side of a training step (reference: nn/trainer.py:93 `features = batch['features'].to(device)` from pageable
memory, after nn/data/transforms.py:35-50 standardised every sample on the CPU).

BatchStager keeps two pinned host buffers and a copy stream per device: batch i+1 is copied while step i computes, the
compute stream only waits on the copy's event, and the per-axis standardisation `(x - shift) / scale` runs as one kernel
on the device instead of per sample on the host.

StitchPairSampler is the input side of the edge-pair classifier's training (GarmentStitchPairsDataset with random_pairs_mode,
nn/data/datasets.py:985-1132): the data set's 3D edges and stitches stay in HBM and every step's pair rows are drawn there.

MeshPointSampler is the input side of the encoder / decoder step (Garment3DPatternFullDataset._get_sample_info): the data set's
meshes stay in HBM and every step's point clouds and segmentation labels are drawn there."""
import torch

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


class StitchPairSampler:
    """Fresh training pairs of the stitch classifier for every step, drawn on the device from a resident data set: what
    GarmentStitchPairsDataset._get_sample_info (nn/data/datasets.py:1119-1122: NNSewingPattern.stitches_as_3D_pairs, then
    FeatureStandartization) gives per garment, for a whole batch in one launch (ops.stitch_pairs_sample) and without host work.  The
    keyword names and defaults are those of the data set's config.

    edges3d [G, P, L, Fe] fp32, num_edges [G, P], gt_stitches [G, 2, S] (edge ids panel * L + edge), gt_num_stitches [G]: the layout
    StitchOnEdge3DPairs.evaluate_stitches takes; data_stats: {'f_shift', 'f_scale'} of the pair rows.

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
        self.f_shift = [float(v) for v in data_stats['f_shift']]
        self.f_scale = [float(v) for v in data_stats['f_scale']]
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
        rows, labels, self.status = ops.stitch_pairs_sample(
            self.edges3d, self.num_edges, self.gt_stitches, self.gt_num_stitches, index, self.stitched_edge_pairs_num,
            self.non_stitched_edge_pairs_num, self.f_shift, self.f_scale, self.state, self.ticket, self.shuffle_pairs,
            self.shuffle_pairs_order)
        return rows, labels


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

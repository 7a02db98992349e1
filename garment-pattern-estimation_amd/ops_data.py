"""Input data on the device: point clouds drawn from resident meshes (mesh_resident, mesh_points_sample), standardisation, the fit of
its statistics (fit_part .. FitAccumulator) and the epoch feed (batch_schedule_draw, feed_jobs, feed_next).  Reached as ops.X: ops.py
re-exports every name of __all__.  The sampler of the stitch classifier's training rows is in ops_stitch, with the classifier."""
import numpy as np
import torch

from . import _lib as L
from ._opbase import F32, F64, _dev_check, _int32

__all__ = ['MeshResident', 'mesh_face_thresholds', 'mesh_resident', 'MESH_SAMPLE_MAX_POINTS', 'MESH_SAMPLE_MAX_BATCH',
           'mesh_points_buffers', 'mesh_points_sample', 'standardize', 'FIT_LEAF', 'FIT_MAX_C', 'FIT_STATUS_EMPTY', 'FIT_STATUS_NONFINITE',
           'fit_leaves', 'fit_part', 'fit_finish', 'fit_read', 'FitAccumulator', 'batch_schedule_draw', 'feed_jobs', 'feed_next']


class MeshResident:
    """the meshes of a data set as mesh_points_sample reads them (built by mesh_resident), ragged over G garments: verts4 fp32
    [sum V, 4] = {x, y, z, the bits of the int32 class id}, faces int32 [sum F, 3] (indices local to the garment), vert_off / face_off
    int32 [G + 1], face_cdf int32 [sum F] holding the uint32 thresholds of the face choice; has_unlabelled: some vertex carries -1"""

    def __init__(self, verts4, faces, vert_off, face_off, face_cdf, has_unlabelled):
        self.verts4, self.faces, self.vert_off, self.face_off, self.face_cdf = verts4, faces, vert_off, face_off, face_cdf
        self.G = vert_off.numel() - 1
        self.has_unlabelled = bool(has_unlabelled)
        self.device = verts4.device

    @property
    def verts(self):
        return self.verts4[:, :3]

    @property
    def vert_label(self):
        return self.verts4.view(torch.int32)[:, 3]


def mesh_face_thresholds(verts, faces):
    """the integer thresholds of the area-proportional face choice of one garment (verts fp32 [V, 3], faces int [F, 3]) -> uint32
    [F]: T[f] = floor(2^31 C_f / C_total), C the sequential float64 cumulative sum of area = 0.5 |(B - A) x (C - A)| from the fp32
    vertices, and T[f] = 2^31 exactly from the last face of positive area onwards; all zeros for a garment without such a face"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64)
    a, e1, e2 = v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = 0.5 * np.sqrt(cx * cx + cy * cy + cz * cz)
    cum = np.cumsum(area)
    out = np.zeros(len(f), dtype=np.uint32)
    positive = np.nonzero(area > 0)[0]
    if len(positive):
        out[:] = np.floor(2.0 ** 31 * (cum / cum[-1])).astype(np.uint32)
        out[positive[-1]:] = 1 << 31
    return out


def mesh_resident(meshes, device='cuda'):
    """Packs the meshes of a data set for mesh_points_sample (setup, not per step): meshes is a list of (verts [V, 3] float, faces
    [F, 3] integer with indices into that garment's vertices, labels [V] integer: the class id of every vertex as the caller's
    PanelClasses map gives it, -1 for a `stitch` / `None` vertex) as arrays or CPU tensors -> MeshResident on `device`.  A face index
    outside 0 .. V - 1, a label below -1 and a coordinate that is not finite are ValueErrors."""
    if isinstance(meshes, MeshResident):
        return meshes
    meshes = list(meshes)
    if not meshes:
        raise ValueError('mesh_resident needs at least one mesh')
    v4, fs, cdf, voff, foff = [], [], [], [0], [0]
    for g, mesh in enumerate(meshes):
        if len(mesh) != 3:
            raise ValueError('mesh %d must be (verts, faces, labels)' % g)
        as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        verts, faces, labels = [as_np(t) for t in mesh]
        if verts.ndim != 2 or verts.shape[1] != 3 or verts.dtype.kind != 'f':
            raise ValueError('mesh %d: verts must be a float [V, 3] array (got %s %s)' % (g, verts.dtype, verts.shape))
        V = verts.shape[0]
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in 'iu':
            raise ValueError('mesh %d: faces must be an integer [F, 3] array (got %s %s)' % (g, faces.dtype, faces.shape))
        if labels.shape != (V,) or labels.dtype.kind not in 'iu':
            raise ValueError('mesh %d: labels must be an integer [%d] array (got %s %s)' % (g, V, labels.dtype, labels.shape))
        verts = verts.astype(np.float32)
        if not np.isfinite(verts).all():
            raise ValueError('mesh %d has a vertex coordinate that is not finite' % g)
        faces, labels = faces.astype(np.int64), labels.astype(np.int64)
        if faces.size and (faces.min() < 0 or faces.max() >= V):
            raise ValueError('mesh %d: a face names vertex %d, outside 0 .. %d' % (g, faces.min() if faces.min() < 0 else faces.max(), V - 1))
        if labels.size and (labels.min() < -1 or labels.max() >= 1 << 31):
            raise ValueError('mesh %d: labels are class ids >= 0, or -1 for a stitch / None vertex' % g)
        packed = np.empty((V, 4), dtype=np.float32)
        packed[:, :3] = verts
        packed.view(np.int32)[:, 3] = labels
        v4.append(packed)
        fs.append(faces.astype(np.int32))
        cdf.append(mesh_face_thresholds(verts, faces))
        voff.append(voff[-1] + V)
        foff.append(foff[-1] + faces.shape[0])
    if voff[-1] >= 1 << 31 or foff[-1] >= 1 << 31:
        raise ValueError('the resident set holds %d vertices and %d faces: the offsets are int32' % (voff[-1], foff[-1]))
    v4 = np.concatenate(v4)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return MeshResident(to(v4), to(np.concatenate(fs).reshape(-1, 3)), to(np.asarray(voff, dtype=np.int32)),
                        to(np.asarray(foff, dtype=np.int32)), to(np.concatenate(cdf).view(np.int32)),
                        bool((v4[:, 3].view(np.int32) < 0).any()))


MESH_SAMPLE_MAX_POINTS, MESH_SAMPLE_MAX_BATCH = (1 << 28) - 1, (1 << 24) - 1    # the counter fields of csrc/gpe_mesh_sample.hip


def mesh_points_buffers(resident, B, N):
    """the outputs and the workspace of mesh_points_sample for B garments of N points: (features, segmentation, status, ws or None).
    A caller that draws many batches into one place (the statistics fit) allocates them once and passes `out=`; the leading slices
    [t[:b] for t in ...] serve a smaller last batch."""
    dev = resident.device
    return (torch.empty(B, N, 3, device=dev, dtype=F32), torch.empty(B, N, device=dev, dtype=torch.int64),
            torch.empty(B, device=dev, dtype=torch.int32),
            torch.empty(B, N, 4, device=dev, dtype=F32) if resident.has_unlabelled else None)


def mesh_points_sample(resident, index, mesh_samples, state, ticket, point_noise_w=0.0, f_shift=None, f_scale=None, out=None):
    """The input point clouds of B garments and their segmentation labels drawn on the device: what
    Garment3DPatternFullDataset._get_sample_info (nn/data/datasets.py: _sample_points, _point_classes_from_mesh,
    FeatureStandartization) gives per garment, in at most two launches of csrc/gpe_mesh_sample.hip and with no host read (semantics
    and random numbers: include/gpe_hip.h).

    resident: mesh_resident(...) on the device; index integer [B]: the garment of every batch slot; f_shift / f_scale: 3 numbers
    each or both None; state int64 [2] = {seed, draw} on the device (stitch_sample_state), advanced by the call; ticket: one zeroed
    int32 of the caller's, left zero; out: mesh_points_buffers(resident, B, N) to draw into instead of new tensors.
    -> features fp32 [B, N, 3] (N = mesh_samples), segmentation int64 [B, N], status int32 [B]
    (>= 0 points that fell back to label 0 for want of a labelled point in their cloud, -1 a garment without a face of positive
    area, -2 index outside 0 .. G - 1; such a slot is all zeros)."""
    if not isinstance(resident, MeshResident):
        raise ValueError('resident must come from ops.mesh_resident (got %s)' % type(resident).__name__)
    dev = resident.device
    N = int(mesh_samples)
    if not 1 <= N <= MESH_SAMPLE_MAX_POINTS:
        raise ValueError('mesh_points_sample draws 1 .. 2^28 - 1 points per garment (got %d)' % N)
    if (f_shift is None) != (f_scale is None) or (f_shift is not None and (len(f_shift) != 3 or len(f_scale) != 3)):
        raise ValueError('the statistics are 3 shifts and 3 scales, or neither')
    if not torch.is_tensor(index) or index.dim() != 1 or not 1 <= index.numel() <= MESH_SAMPLE_MAX_BATCH:
        raise ValueError('index must be an integer [B] tensor, 1 <= B < 2^24')
    B = index.numel()
    if B * ((N + 511) // 512) >= 1 << 31:
        raise ValueError('B * ceil(N / 512) must stay below 2^31 (got B = %d, N = %d)' % (B, N))
    if index.is_floating_point() or index.is_complex() or index.dtype == torch.bool or index.device != dev:
        raise ValueError('index must be an integer [%d] tensor on the device of the resident set' % B)
    if (not torch.is_tensor(state) or state.dtype != torch.int64 or tuple(state.shape) != (2,) or state.device != dev
            or not state.is_contiguous()):
        raise ValueError('state must be a contiguous int64 [2] tensor {seed, draw} on the device of the resident set')
    if not torch.is_tensor(ticket) or ticket.dtype != torch.int32 or ticket.numel() != 1 or ticket.device != dev:
        raise ValueError('ticket must be one zeroed int32 on the device of the resident set')
    _dev_check(resident.verts4)
    import ctypes
    sh = (ctypes.c_float * 3)(*[float(v) for v in f_shift]) if f_shift is not None else None
    sc = (ctypes.c_float * 3)(*[float(v) for v in f_scale]) if f_scale is not None else None
    features, seg, status, ws = out if out is not None else mesh_points_buffers(resident, B, N)
    if out is not None and (
            features.shape != (B, N, 3) or features.dtype != F32 or seg.shape != (B, N) or seg.dtype != torch.int64
            or status.shape != (B,) or status.dtype != torch.int32 or (ws is None) != (not resident.has_unlabelled)
            or (ws is not None and (ws.shape != (B, N, 4) or ws.dtype != F32))
            or any(t.device != dev or not t.is_contiguous() for t in out if t is not None)):
        raise ValueError('out must be mesh_points_buffers(resident, %d, %d) (or leading slices of a larger set)' % (B, N))
    L.call('gpe_mesh_points_sample', resident.verts4, resident.faces, resident.vert_off, resident.face_off, resident.face_cdf,
           resident.G, _int32(index, -1, resident.G), B, N, float(point_noise_w), sh, sc, 1 if resident.has_unlabelled else 0, ws,
           state, ticket, features, seg, status)
    return features, seg, status


def standardize(x, shift, scale):
    """nn/data/transforms.py:35-50 FeatureStandartization on the device: (x - shift) / scale per column."""
    import ctypes
    _dev_check(x)
    x = x.contiguous()
    C = x.shape[-1]
    sh = (ctypes.c_float * C)(*[float(v) for v in shift])
    sc = (ctypes.c_float * C)(*[float(v) for v in scale])
    out = torch.empty_like(x)
    L.call('gpe_standardize', x, x.numel() // C, C, sh, sc, out)
    return out


# -------------------------------------------------------------------------------------------------
# Fitting the standardisation statistics (GarmentBaseDataset._get_distribution_stats / _get_norm_stats, nn/data/datasets.py:534-568)
# -------------------------------------------------------------------------------------------------
FIT_LEAF, FIT_MAX_C = 512, 16                    # rows per leaf and columns of csrc/gpe_fit_stats.hip
FIT_STATUS_EMPTY, FIT_STATUS_NONFINITE = 1, 2    # status bits of the result block (include/gpe_hip_fit.h)


def fit_leaves(sets, rows_per_set):
    """the records a part image of `sets` sets of `rows_per_set` rows holds (host only)"""
    n = L.query('gpe_fit_leaves', int(sets), int(rows_per_set))
    if n < 0:
        raise ValueError('fit_leaves: sets and rows_per_set must be positive and their leaves fit 63 bits (got %r, %r)'
                         % (sets, rows_per_set))
    return n


def _fit_columns(C):
    if isinstance(C, bool) or not isinstance(C, int) or not 1 <= C <= FIT_MAX_C:
        raise ValueError('the statistics fit handles 1 .. %d columns (got %r)' % (FIT_MAX_C, C))
    return C


def fit_part(x, part, leaf0=0, padded=False):
    """One record of 1 + 4 C doubles per leaf (512 rows of one set) of x fp32 [S, N, C], written into the caller's part image (fp64
    [leaves, 1 + 4 C]) from record leaf0 on: n, then per column mean, squared deviations, min, max over the rows kept (padded: rows
    with |x| <= 1e-5 in every column are dropped, the reference's _unpad).  One launch of csrc/gpe_fit_stats.hip, no host read."""
    if not torch.is_tensor(x) or x.dim() != 3:
        raise ValueError('fit_part: x must be [S, N, C] (got %s)' % (tuple(getattr(x, 'shape', ())),))
    _dev_check(x)
    S, N, C = x.shape
    _fit_columns(C)
    if not x.is_contiguous():
        raise ValueError('fit_part: x must be contiguous')
    if (not torch.is_tensor(part) or part.dtype != F64 or part.dim() != 2 or part.shape[1] != 1 + 4 * C or part.device != x.device
            or not part.is_contiguous()):
        raise ValueError('fit_part: part must be a contiguous fp64 [leaves, %d] tensor on the device of x' % (1 + 4 * C))
    leaves = fit_leaves(S, N)
    if not 0 <= int(leaf0) <= part.shape[0] - leaves:
        raise ValueError('fit_part: the %d leaves of x from record %d on do not fit a part image of %d' % (leaves, leaf0, part.shape[0]))
    L.call('gpe_fit_part', x.detach(), S, N, C, 1 if padded else 0, int(leaf0), part.shape[0], part)
    return part


def fit_finish(part, out=None):
    """Merges the records of a part image (fit_part) in a fixed order -> the result block, fp64 [2 + 5 C] on the device: n, status,
    mean [C], std [C], min [C], max [C], norm_scale [C] (include/gpe_hip_fit.h).  One launch, no host read."""
    if not torch.is_tensor(part) or part.dtype != F64 or part.dim() != 2 or part.shape[0] < 1 or (part.shape[1] - 1) % 4 or not part.is_contiguous():
        raise ValueError('fit_finish: part must be a contiguous fp64 [leaves, 1 + 4 C] tensor')
    if not part.is_cuda:
        raise RuntimeError('gpe ops need tensors on the MI355X (got a %s part image); there is no CPU path' % part.device)
    C = _fit_columns((part.shape[1] - 1) // 4)
    if out is None:
        out = torch.empty(2 + 5 * C, device=part.device, dtype=F64)
    elif out.dtype != F64 or tuple(out.shape) != (2 + 5 * C,) or out.device != part.device or not out.is_contiguous():
        raise ValueError('fit_finish: out must be a contiguous fp64 [%d] tensor on the device of part' % (2 + 5 * C))
    L.call('gpe_fit_finish', part, part.shape[0], C, out)
    return out


def fit_read(result):
    """the result block of fit_finish on the host (ONE device read), rounded to fp32 once like the reference's fp32 results ->
    {'n': int, 'status': int, 'mean' / 'std' / 'min' / 'max' / 'norm_scale': fp32 numpy [C]}; ValueError when no row was left"""
    r = result.detach().cpu().numpy()
    C = (r.size - 2) // 5
    status = int(r[1])
    if status & FIT_STATUS_EMPTY:
        raise ValueError('the statistics fit found no row (every row was dropped as padding)')
    keys = ('mean', 'std', 'min', 'max', 'norm_scale')
    out = {k: r[2 + i * C:2 + (i + 1) * C].astype(np.float32) for i, k in enumerate(keys)}
    out.update(n=int(r[0]), status=status)
    return out


class FitAccumulator:
    """The statistics of a data set that is handed in as chunks of whole sets:

        acc = FitAccumulator(3, G, 2000, 'cuda')
        for chunk in ...: acc.add(points)            # fp32 [g, 2000, 3] on the device, consecutive sets
        stats = acc.read()                           # {'n', 'mean', 'std', 'min', 'max', 'norm_scale', 'status'}

    The part image depends on (sets, rows_per_set) and the data alone, so the result is bit-identical for every chunking, grid size
    and CU reservation.  Nothing reads the host before read()."""

    def __init__(self, C, sets, rows_per_set, device, padded=False):
        self.C = _fit_columns(C)
        for name, v in (('sets', sets), ('rows_per_set', rows_per_set)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError('FitAccumulator: %s must be a positive integer (got %r)' % (name, v))
        self.sets, self.rows_per_set, self.padded = sets, rows_per_set, bool(padded)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('gpe ops need tensors on the MI355X (got device %s); there is no CPU path' % self.device)
        self.leaves = fit_leaves(sets, rows_per_set)
        self.part = torch.empty(self.leaves, 1 + 4 * self.C, device=self.device, dtype=F64)
        self.added, self.result = 0, None

    def add(self, x):
        """x: fp32 [g, rows_per_set, C] on the device: the next g sets"""
        if (not torch.is_tensor(x) or x.dim() != 3 or x.shape[0] < 1 or tuple(x.shape[1:]) != (self.rows_per_set, self.C)
                or x.dtype != F32):
            raise ValueError('FitAccumulator.add: fp32 [g >= 1, %d, %d] expected (got %s %s)'
                             % (self.rows_per_set, self.C, getattr(x, 'dtype', type(x).__name__), tuple(getattr(x, 'shape', ()))))
        if x.device != self.part.device:
            raise ValueError('FitAccumulator.add: x lives on %s, the accumulator on %s' % (x.device, self.part.device))
        if self.added + x.shape[0] > self.sets:
            raise ValueError('FitAccumulator.add: %d sets after %d, but %d were announced' % (x.shape[0], self.added, self.sets))
        fit_part(x.contiguous(), self.part, self.added * (self.leaves // self.sets), self.padded)
        self.added += x.shape[0]
        self.result = None

    def finish(self):
        """-> the result block on the device (fit_finish); every announced set must have been added"""
        if self.added != self.sets:
            raise ValueError('FitAccumulator.finish: %d of the %d announced sets were added' % (self.added, self.sets))
        if self.result is None:
            self.result = fit_finish(self.part)
        return self.result

    def read(self):
        """-> fit_read(finish()): the one host read"""
        return fit_read(self.finish())


def batch_schedule_draw(class_off, ids, quota, class_off_host, quota_host, B, drop_last, state, ws, table, batch_len):
    """One epoch's balanced batch schedule into table int32 [rows, B] and batch_len int32 [rows] (include/gpe_hip_feed.h): three launches,
    no host read.  class_off / quota: int32 on the device, with numpy int32 copies for the argument checks; state {seed, epoch} advances"""
    L.call('gpe_batch_schedule_draw', class_off, ids, quota, class_off_host.ctypes.data, quota_host.ctypes.data, quota.numel(),
           ids.numel(), int(B), 1 if drop_last else 0, state, ws, ws.numel(), table, batch_len)


def feed_jobs(tables, outputs):
    """the job array of feed_next: resident tables [G, ...] and their outputs [B, ...], contiguous device tensors whose rows are a
    multiple of 4 bytes, 16 at the most -> (jobs int64 [T, 3] on the device, the bytes of the widest row); checked by gpe_feed_jobs"""
    import ctypes
    T, nb = len(tables), [t[0].numel() * t.element_size() for t in tables]
    bad = any(not (t.is_contiguous() and o.is_contiguous() and o[0].numel() * o.element_size() == n) for t, o, n in zip(tables, outputs, nb))
    jobs, ptrs = np.zeros((T, 3), dtype=np.int64), lambda ts: (ctypes.c_void_p * T)(*[t.data_ptr() for t in ts])
    if bad or L.lib().gpe_feed_jobs(T, ptrs(tables), ptrs(outputs), (ctypes.c_long * T)(*nb), jobs.ctypes.data) != 0:
        raise ValueError('feed_jobs: 1 .. 16 contiguous tables, rows a multiple of 4 bytes and as wide as their outputs\' (%d: %s)' % (T, nb))
    return torch.from_numpy(jobs).to(tables[0].device), max(nb)


def feed_next(table, cursor, G, jobs, max_row_bytes, index_out, status):
    """The next batch (two launches, legal in a capture): index_out int32 [B] = row cursor % rows of table; every job's output row b =
    its resident row index_out[b]; cursor int64 [1] advanced; status int32 [1] = the entries outside 0 .. G - 1 (zero rows)"""
    L.call('gpe_feed_next', table, table.shape[0], table.shape[1], cursor, int(G), jobs, 0 if jobs is None else jobs.shape[0],
           int(max_row_bytes), index_out, status)

"""Prediction from raw scans on the device: point clouds of arbitrary size kept resident (cloud_resident), the model's clouds drawn
from them (cloud_points_sample) and the predicted per-point panel labels handed back to every point of a scan (cloud_labels):
csrc/gpe_scan_sample.hip, include/gpe_hip_scan.h.  Reached as ops.X: ops.py re-exports every name of __all__.  A leaf of its own
beside ops_data, whose mesh sampler it mirrors: the leaves that ops.py was cut into keep their combined size."""
import numpy as np
import torch

from . import _lib as L
from ._opbase import F32, _dev_check, _int32

__all__ = ['CloudResident', 'cloud_resident', 'CLOUD_SAMPLE_MAX_SAMPLES', 'CLOUD_SAMPLE_MAX_POINTS', 'CLOUD_SAMPLE_MAX_BATCH',
           'cloud_points_buffers', 'cloud_points_sample', 'cloud_labels']

# N, the points of one cloud and B: GPE_SCAN_MAX_SAMPLES / _POINTS / _BATCH of include/gpe_hip_scan.h
CLOUD_SAMPLE_MAX_SAMPLES, CLOUD_SAMPLE_MAX_POINTS, CLOUD_SAMPLE_MAX_BATCH = 2048, (1 << 28) - 1, (1 << 24) - 1


class CloudResident:
    """the scans of a batch of users as cloud_points_sample reads them (built by cloud_resident), ragged over G clouds: points4 fp32
    [T, 4] = {x, y, z, 0}, off int32 [G + 1]; sizes: the n_g on the host (a tuple), n_max their maximum (at least 1)"""

    def __init__(self, points4, off, sizes):
        self.points4, self.off, self.sizes = points4, off, tuple(int(n) for n in sizes)
        self.G, self.T = len(self.sizes), int(sum(self.sizes))
        self.n_max = max(max(self.sizes), 1)
        self.device = points4.device

    @property
    def points(self):
        return self.points4[:, :3]


def cloud_resident(clouds, device='cuda'):
    """Packs raw scans for cloud_points_sample (setup, not per call): clouds is a list of [n, 3] float arrays or CPU tensors (n = 0 is
    kept: its slot reports status -1) -> CloudResident on `device`.  A cloud that is not [n, 3], has a coordinate that is not finite or
    more than 2^28 - 1 points is a ValueError."""
    if isinstance(clouds, CloudResident):
        return clouds
    clouds = list(clouds)
    if not clouds:
        raise ValueError('cloud_resident needs at least one cloud')
    parts, off = [], [0]
    for g, c in enumerate(clouds):
        c = c.detach().cpu().numpy() if torch.is_tensor(c) else np.asarray(c)
        if c.ndim != 2 or c.shape[1] != 3 or c.dtype.kind not in 'fiu':
            raise ValueError('cloud %d must be a numeric [n, 3] array (got %s %s)' % (g, c.dtype, c.shape))
        if c.shape[0] > CLOUD_SAMPLE_MAX_POINTS:
            raise ValueError('cloud %d holds %d points: the limit is 2^28 - 1' % (g, c.shape[0]))
        c = c.astype(np.float32)
        if not np.isfinite(c).all():
            raise ValueError('cloud %d has a coordinate that is not finite' % g)
        packed = np.zeros((c.shape[0], 4), dtype=np.float32)
        packed[:, :3] = c
        parts.append(packed)
        off.append(off[-1] + c.shape[0])
    if off[-1] >= 1 << 31:
        raise ValueError('the resident set holds %d points: the offsets are int32' % off[-1])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)               # noqa: E731
    # (one row of padding keeps an all-empty set a real allocation)
    return CloudResident(to(np.concatenate(parts + [np.zeros((1, 4), dtype=np.float32)])), to(np.asarray(off, dtype=np.int32)),
                         np.diff(off))


def _ws_bytes(B, N, n_max):
    n = L.query('gpe_scan_sample_ws_bytes', B, N, n_max)
    if n < 0:
        raise ValueError('gpe_scan_sample_ws_bytes(%d, %d, %d) failed with code %d' % (B, N, n_max, n))
    return n


def cloud_points_buffers(resident, B, N):
    """the outputs and the workspace of cloud_points_sample for B slots of N points: (features, picked, status, ws).  A caller that
    draws many batches into one place allocates them once and passes `out=`."""
    dev = resident.device
    return (torch.empty(B, N, 3, device=dev, dtype=F32), torch.empty(B, N, device=dev, dtype=torch.int32),
            torch.empty(B, device=dev, dtype=torch.int32),
            torch.empty(_ws_bytes(B, N, resident.n_max), device=dev, dtype=torch.uint8))


def _slots(resident, index):
    if not isinstance(resident, CloudResident):
        raise ValueError('resident must come from ops.cloud_resident (got %s)' % type(resident).__name__)
    if not torch.is_tensor(index) or index.dim() != 1 or not 1 <= index.numel() <= CLOUD_SAMPLE_MAX_BATCH:
        raise ValueError('index must be an integer [B] tensor, 1 <= B < 2^24')
    _dev_check(resident.points4)
    if index.is_floating_point() or index.is_complex() or index.dtype == torch.bool or index.device != resident.device:
        raise ValueError('index must be an integer [%d] tensor on the device of the resident set' % index.numel())
    return _int32(index, -1, resident.G)


def cloud_points_sample(resident, index, samples, state, ticket, f_shift=None, f_scale=None, out=None, narrow_above=0):
    """The model's input clouds of B scans drawn on the device: per slot what predict_per_example.py:137-144 does on the host
    (np.random.permutation(n)[:samples], (p - f_shift) / f_scale), in three launches of csrc/gpe_scan_sample.hip and with no host
    read (the rule and the random numbers: include/gpe_hip_scan.h).

    resident: cloud_resident(...) on the device; index integer [B]: the scan of every batch slot; f_shift / f_scale: 3 numbers each or
    both None; state int64 [2] = {seed, draw} on the device (stitch_sample_state), advanced by the call; ticket: one zeroed int32 of
    the caller's, left zero; out: cloud_points_buffers(resident, B, samples) to draw into; narrow_above: see the header (tests).
    -> features fp32 [B, N, 3], picked int32 [B, N] (the point's index inside its scan), status int32 [B] (N - n repeated rows of a
    scan of n < N points, 0 otherwise; -1 an empty scan, -2 index outside 0 .. G - 1: such a slot is zeros and picked -1)."""
    idx = _slots(resident, index)
    dev, B, N = resident.device, index.numel(), int(samples)
    if not 1 <= N <= CLOUD_SAMPLE_MAX_SAMPLES:
        raise ValueError('cloud_points_sample draws 1 .. %d points per scan (got %d)' % (CLOUD_SAMPLE_MAX_SAMPLES, N))
    if (f_shift is None) != (f_scale is None) or (f_shift is not None and (len(f_shift) != 3 or len(f_scale) != 3)):
        raise ValueError('the statistics are 3 shifts and 3 scales, or neither')
    if (not torch.is_tensor(state) or state.dtype != torch.int64 or tuple(state.shape) != (2,) or state.device != dev
            or not state.is_contiguous()):
        raise ValueError('state must be a contiguous int64 [2] tensor {seed, draw} on the device of the resident set')
    if not torch.is_tensor(ticket) or ticket.dtype != torch.int32 or ticket.numel() != 1 or ticket.device != dev:
        raise ValueError('ticket must be one zeroed int32 on the device of the resident set')
    import ctypes
    sh = (ctypes.c_float * 3)(*[float(v) for v in f_shift]) if f_shift is not None else None
    sc = (ctypes.c_float * 3)(*[float(v) for v in f_scale]) if f_scale is not None else None
    features, picked, status, ws = out if out is not None else cloud_points_buffers(resident, B, N)
    if out is not None and (
            features.shape != (B, N, 3) or features.dtype != F32 or picked.shape != (B, N) or picked.dtype != torch.int32
            or status.shape != (B,) or status.dtype != torch.int32 or ws.dtype != torch.uint8
            or ws.numel() < _ws_bytes(B, N, resident.n_max) or any(t.device != dev or not t.is_contiguous() for t in out)):
        raise ValueError('out must be cloud_points_buffers(resident, %d, %d)' % (B, N))
    L.call('gpe_scan_sample', resident.points4, resident.off, resident.G, resident.n_max, idx, B, N, sh, sc, int(narrow_above), ws,
           ws.numel(), state, ticket, features, picked, status)
    return features, picked, status


def cloud_labels(resident, index, picked, att_weights, out=None):
    """The panel label of every point of the scans of a batch: the arg-max of the attention weights (att_weights fp32 [B, N, P], the
    model's `att_weights`) of the nearest of the slot's N drawn points (picked int32 [B, N], cloud_points_sample's for the same
    index), one launch (include/gpe_hip_scan.h gpe_scan_labels: ties, bad slots, a scan in two slots).  out: a resident-sized
    int32 [T] tensor to write into — rows of scans outside the batch keep what they hold; a new one starts at -1.  -> labels int32 [T]"""
    idx = _slots(resident, index)
    dev, B = resident.device, index.numel()
    if (not torch.is_tensor(picked) or picked.dtype != torch.int32 or picked.dim() != 2 or picked.shape[0] != B or picked.shape[1] < 1
            or picked.device != dev):
        raise ValueError('picked must be the int32 [%d, N] tensor of cloud_points_sample' % B)
    N = picked.shape[1]
    if not torch.is_tensor(att_weights) or att_weights.dim() != 3 or tuple(att_weights.shape[:2]) != (B, N) or not 1 <= att_weights.shape[2] <= 4096:
        raise ValueError('att_weights must be an fp32 [%d, %d, P] tensor, 1 <= P <= 4096' % (B, N))
    _dev_check(att_weights)
    if out is None:
        out = torch.full((max(resident.T, 1),), -1, device=dev, dtype=torch.int32)[:resident.T]
    elif out.dtype != torch.int32 or tuple(out.shape) != (resident.T,) or out.device != dev or not out.is_contiguous():
        raise ValueError('out must be a contiguous int32 [%d] tensor on the device of the resident set' % resident.T)
    if resident.T:
        L.call('gpe_scan_labels', resident.points4, resident.off, resident.G, resident.n_max, idx, B, N, picked.contiguous(),
               att_weights.detach().contiguous(), att_weights.shape[2], out)
    return out

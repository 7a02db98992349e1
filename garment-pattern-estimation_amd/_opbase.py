"""What every ops module shares and nothing rebinds: dtypes, the device check, row descriptors, the per-stream scratch of the
C-ABI calls (workspace, edge workspace, amax words, tickets) and the small argument helpers that more than one domain uses
(_int32, _int_tensor of the samplers; _view_strides, _row_stride of the losses and the quality metrics; _stitch_ldw, the weight
pitch the stitch classifier shares with the edge predictor).

Imports _lib and streams and nothing else from the package, so every other module may import it.  No name here is assigned after
import: the dicts are caches, mutated in place.  State that callers rebind lives in ops.py alone (DESIGN.md "ops modules")."""
import torch

from . import _lib as L
from . import streams


F32 = torch.float32
F64 = torch.float64


def _dev_check(t):
    if not t.is_cuda:
        raise RuntimeError('gpe ops need tensors on the MI355X (got a %s tensor); there is no CPU path' % t.device)
    if t.dtype != F32:
        raise RuntimeError('gpe ops are fp32 (got %s)' % t.dtype)


def _rows2d(t):
    """(tensor, stride_outer, stride_inner, inner) descriptor of a [M, K] tensor with unit inner stride."""
    assert t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), (t.shape, t.stride())
    return (t, t.stride(0), 0, 0)


def _rows3d(t):
    """descriptor of a [R, T, K] tensor flattened to R*T logical rows (row r*T+t)."""
    assert t.dim() == 3 and (t.shape[2] == 1 or t.stride(2) == 1), (t.shape, t.stride())
    return (t, t.stride(0), t.stride(1), t.shape[1])


def round_up(a, b):
    return (a + b - 1) // b * b


_WS = {}                   # (device index, stream handle) -> uint8 tensor: the scratch of that stream's C-ABI calls


def _workspace(nbytes, device):
    """caller-owned scratch of a C-ABI call (include/gpe_hip.h: `ws`).  One grow-only buffer per (device, stream): launches of one
    stream are ordered, so consecutive calls may share it, and two streams never do (the library's only rule for workspaces).
    Re-allocation goes through torch's caching allocator, which keeps the old block alive until the stream has passed it."""
    key = streams.stream_key(device)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), device=torch.device('cuda', key[0]), dtype=torch.uint8)
        _WS[key] = buf
    return buf


_EDGE_WS_BYTES = {}


def edge_workspace(B, N, k, ldmax, device):
    """-> (ws, bytes) for gpe_edge_mlp_fwd / _bwd / gpe_edge_redgemm / gpe_edge_pq_amax calls on B clouds of N points, k
    neighbours, per-point output pitches <= ldmax floats."""
    key = (B, N, k, ldmax)
    n = _EDGE_WS_BYTES.get(key)
    if n is None:
        n = L.query('gpe_edge_ws_bytes', B, N, k, ldmax)
        if n < 0:
            raise RuntimeError('gpe_edge_ws_bytes failed with code %d' % n)
        _EDGE_WS_BYTES[key] = n
    return _workspace(n, device), n


def f16x3_words(n, rows, device):
    """n caller-owned "amax words" (include/gpe_hip.h) when the f16x3 arithmetic will run on `rows`-row edge launches, else None:
    one uint32 per tensor whose largest magnitude a kernel measures while storing it and a later kernel scales by."""
    if L.get_math() != 'f16x3' or rows < L.query('gpe_f16x3_min_rows'):
        return None
    return torch.zeros(n, device=device, dtype=torch.int32)


def _word(words, i):
    return None if words is None else words[i:i + 1]


_TICKETS = {}


def _ticket(device):
    """the last-arriver ticket of gpe_pack_fold: one zeroed uint32 per (device, stream), left zero by every launch."""
    key = streams.stream_key(device)
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS[key] = torch.zeros(1, device=torch.device('cuda', key[0]), dtype=torch.int32)
    return t


def _stitch_ldw(H):
    nb = (H + 15) // 16
    nb = 4 if nb <= 4 else 8 if nb <= 8 else 13 if nb <= 13 else 16
    return nb * 16 if (nb * 16) % 32 == 16 else nb * 16 + 16


def _view_strides(ol):
    """(sb, sp, sl) of an outlines view [B,P,L,4] whose last dim is unit-stride (a slice of the [B,P,L,8] output)."""
    assert ol.dim() == 4 and ol.stride(3) == 1, (ol.shape, ol.stride())
    return ol.stride(0), ol.stride(1), ol.stride(2)


def _row_stride(t, P):
    """row pitch of a [B,P,c] view of a [B*P, ld] tensor."""
    assert t.dim() == 3 and t.stride(2) == 1 and t.stride(0) == P * t.stride(1), (t.shape, t.stride())
    return t.stride(1)


def _int_tensor(t, shape, name, dev):
    if (not torch.is_tensor(t) or tuple(t.shape) != shape or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool
            or t.device != dev):
        raise ValueError('%s must be an integer %s tensor on the device of edges3d' % (name, list(shape)))


def _int32(t, lo, hi):
    """an integer tensor as the kernels read it: int32 as it is (they clamp themselves), wider ones brought into range first"""
    t = t.detach()
    if t.dtype != torch.int32:
        t = t.to(torch.int64).clamp(lo, hi).to(torch.int32)
    return t.contiguous()

"""Host-side orchestration of the gfx950 kernels (C ABI in include/gpe_hip.h) + the autograd glue.

torch is used here for device memory, streams, parameter storage and the CPU RNG of the reference's random
LSTM states — every arithmetic step of the path is a call into libgpe_hip.so.  Nothing in this file falls back
to torch math: a missing library or a failing launch raises.

Reference lines restated by each Function are cited in its docstring (paths relative to /root/reference).

This module is the training hot path and the facade: the stitch classifier, the losses, the data samplers and the evaluation live
in ops_stitch / ops_losses / ops_data / ops_eval and are re-exported at the end of this file, so callers spell everything ops.X.
Every module-level name that callers REBIND through ops (SIDE_GRADS, SIDE_MIN_EDGES, CAPTURE, HOST_DRAWN, RNN_WS_HOOK, ...) is
defined here and read only by functions defined here (DESIGN.md "ops modules", tests/test_ops_layout_host.py).

Two per-model services live here as well (both optional; without them every Function behaves like a plain autograd op):
  * PackPlan  — all weight-derived kernel operands of a model (MFMA-packed / transposed / gate-interleaved weights, the
                P|Q split of the first edge Linear, b_ih + b_hh) are rebuilt by ONE launch when the weights changed,
                instead of ~45 small launches per training step;
  * grad sink — when a model's parameters live in a flat arena (optim.FlatArena), backward kernels write weight gradients
                straight into the arena's gradient buffer (no per-parameter tensors, no cat/copy for the all-reduce
                buckets, one fused Adam launch).
"""
import collections
import contextlib
import math
import os
import warnings
import weakref

import numpy as np
import torch

from . import _lib as L
from . import streams
from ._opbase import (F32, F64, _WS, _dev_check, _rows2d, _rows3d, _stitch_ldw, _ticket, _word, _workspace,  # noqa: F401
                      edge_workspace, f16x3_words, round_up)


def pack_fold(W, bias, stats, ews, ews_n, clear_word):
    """-> (packed W diag(s), b + W t) of the BatchNorm fold in one launch; ews given (f16x3): the packed weight's amax lands in the
    edge workspace and the coming gpe_edge_mlp_fwd is told so (bit 1 of its out_half)."""
    N, K = W.shape
    wp = torch.empty(L.query('gpe_packed_size', N, K), device=W.device, dtype=F32)
    bf = torch.empty(N, device=W.device, dtype=F32)
    L.call('gpe_pack_fold', W, W.stride(0), N, K, stats[2], stats[3], bias, wp, bf, ews, ews_n if ews is not None else 0, clear_word,
           _ticket(W.device) if ews is not None else None)
    return wp, bf


# -------------------------------------------------------------------------------------------------
# Leaf weight-gradient launches on a side stream
# -------------------------------------------------------------------------------------------------
# The weight-gradient reduce-GEMMs of a recurrent stack are LEAVES of the backward pass (nothing downstream reads them before the
# optimizer), and what follows the panel decoder's backward on the critical path is the pattern decoder's persistent backward
# launch, which occupies a few CUs for 0.2 ms.  `side_grads(...)` moves the launches issued inside it to one side stream per device
# (forked behind everything the current stream has queued, joined back by an autograd callback when the backward pass ends), so
# that the two overlap.  Only when every gradient involved lands in a flat arena (optim.FlatArena: nothing is returned to autograd),
# and outside stream captures (measured: no gain inside a captured step).  With more than one rank a gradient bucket leaves for the
# all-reduce when the arena is told its last gradient is written = queued: parallel.DistributedHotPath joins the side stream in front
# of a collective issued from the main stream.  GPE_DEBUG=1 GPE_SIDE_GRADS=0 keeps everything on one stream (A/B).
# Only for steps the GPU bounds: the fork / join / record_stream bookkeeping costs the host ~0.3 ms per step, which a host-bound shape
# (BASELINE cfg 1 with eager launches: 3.6 -> 4.0 ms) cannot hide.  The proxy is the size of the step's last EdgeConv graph (edges).
SIDE_GRADS = not (os.environ.get('GPE_DEBUG') == '1' and os.environ.get('GPE_SIDE_GRADS') == '0')
SIDE_MIN_EDGES = 1 << 17
SIDE_PQ = not (os.environ.get('GPE_DEBUG') == '1' and os.environ.get('GPE_SIDE_PQ') == '0')     # the forward fork of EdgeConvFn (A/B)
# The fork / join mechanics, the lane's state and the idle-stretch jobs live in streams.py (one lane per device); this file decides
# what goes there.  _LAST_EDGES stays process-global on purpose: it is a size proxy for "is this step GPU-bound", not stream state.
_LAST_EDGES = [0]


def _side_ok(edges):
    """May a step whose EdgeConv graph has `edges` edges fork onto the side lane now?  (the switches are read at call time)"""
    return bool(SIDE_GRADS and edges >= SIDE_MIN_EDGES and not torch.cuda.is_current_stream_capturing())


def side_grads(params, tensors):
    """with side_grads(params, tensors) as on_side: ...  — the launches inside run on the side stream when that is legal (see above);
    `tensors` = every main-stream tensor the launches read (kept away from the allocator until the side stream has passed them)."""
    if params and _side_ok(_LAST_EDGES[0]) and all(_SINK.get(p.data_ptr()) is not None and _SINK[p.data_ptr()][0]() is not None for p in params):
        return streams.lane(params[0].device.index).fork(tensors, leaf=True)
    return contextlib.nullcontext(False)


# -------------------------------------------------------------------------------------------------
# PackPlan: weight-derived operands refreshed by one launch
# -------------------------------------------------------------------------------------------------
WEIGHTS_EPOCH = 0          # bumped by optimizers that update parameters through raw pointers (optim.FusedAdam)
_PACKS = {}                # (param data_ptr, kind) -> (weakref to the plan, output tensor, index of the job in plan.specs); a plan's
#                            entries die with the plan (weakref.finalize)

K_PLAIN, K_TRANS, K_GATES, K_PQ, K_PQT, K_VADD, K_BPQ, K_GRUB = 0, 1, 2, 3, 4, 5, 6, 7
K_GATES_H3, K_AMAX, K_TRANS_H3 = 8, 9, 10      # f16x3 operands of the recurrences: fp16 plane packs + the amax job they depend on
PLANE_KINDS = (K_GATES_H3, K_TRANS_H3)
_JOB = np.dtype([('w', '<u8'), ('w2', '<u8'), ('out', '<u8'), ('total', '<i8'), ('first_block', '<i8'),
                 ('ldw', '<i4'), ('N', '<i4'), ('K', '<i4'), ('kind', '<i4'), ('Npad', '<i4'), ('aux', '<i4')])
assert _JOB.itemsize == 64
# one job of a PackPlan: source parameter, second source (a bias pair) or None, K_* kind, output rows and columns, the kind's own
# number (units per gate, width of a half), length of a vector output or None
PackSpec = collections.namedtuple('PackSpec', 'p p2 kind N K aux out_numel')


def _pack_geometry(sp):
    """-> (Npad, total) of a PackSpec: the padded row count its job record carries and the floats of its output"""
    if sp.kind in (K_VADD, K_BPQ, K_GRUB):
        return 0, sp.out_numel
    if sp.kind in (K_GATES, K_GATES_H3):
        npad = 16 * (sp.N // sp.aux) * ((sp.aux + 15) // 16)      # gate-interleaved: each gate's units filled up to whole blocks of 16
    else:
        npad = round_up(sp.N, 16)
    if sp.kind == K_GATES:
        return npad, npad * round_up(sp.K, 16)
    if sp.kind in PLANE_KINDS:
        return npad, L.query('gpe_packed_planes_size', npad, sp.K)
    return npad, L.query('gpe_packed_size', sp.N, sp.K)           # K filled up to the edge kernels' resident chunk count


def _job_table(rows, dev):
    """rows: per job the fields of _JOB without first_block -> (the records gpe_pack_multi reads, as bytes on `dev`; blocks of the launch)"""
    tab = np.zeros(len(rows), dtype=_JOB)
    blk = 0
    for i, (w, w2, out, total, ldw, N, K, kind, npad, aux) in enumerate(rows):
        tab[i] = (w, w2, out, total, blk, ldw, N, K, kind, npad, aux)
        blk += L.query('gpe_pack_job_blocks', kind, total, npad, K)
    return torch.from_numpy(tab.view(np.uint8).copy()).to(dev), blk


# (PackPlan.refresh on a side stream under the layer-1 kNN search was built in round 5 and MEASURED SLOWER — cfg 2, one session, twice
# each: 10.19 / 10.17 ms per step without, 10.34 / 10.34 with: the stream fork / join costs more than the 0.09 ms of pack launches it
# hides — and removed in round 6: profiles/r05_c_reverted_experiments.md.)


def bump_weights_epoch():
    global WEIGHTS_EPOCH
    WEIGHTS_EPOCH += 1


class PackPlan:
    """Collects the static pack jobs of a model (net_blocks modules call `add_*` from their `register_packs`) and re-runs them
    all with ONE gpe_pack_multi launch at the start of every model forward (40 us at the shipped sizes).  Outputs are
    persistent buffers, so backward reads what forward used.

    Why every forward and not "when a parameter changed": torch's version counters do not see an update made through
    `p.data` (an EMA of the weights, a hand-written `p.data.copy_()`, a foreign optimizer working on raw storage), and a stale
    pack gives silently wrong numbers.  In training the weights change every step anyway.  A caller whose weights are truly
    constant (inference loops) may set `plan.frozen = True` after the first forward: the launch is then skipped while the
    version counters and WEIGHTS_EPOCH stand still — that caller vouches for not touching `p.data`.

    A plan — and therefore the module that owns it — is SINGLE-STREAM: its outputs and amax words are rewritten by every refresh,
    so two streams driving the same module at the same time would race (the C library itself is stream-safe: all state is the
    caller's).  Use one module copy per stream (tests/test_gpu_kernels.py::test_two_streams_one_device).  A module that moves from
    one stream to another between forwards is handled: refresh() makes the new stream wait for the previous one."""

    def __init__(self):
        self.specs = []        # PackSpec records, one per job
        self.outs = []
        self.table = None
        self.blocks = 0
        self.vers = None
        self.epoch = -1
        self.home = None
        self.keys = []
        self.frozen = False
        self.h3_current = False
        self._stream = None
        self._keys_box = box = []              # shared with the finalizer: the keys this plan currently owns in _PACKS
        me = weakref.ref(self)
        # pop only entries that are still THIS plan's: a newer plan over the same parameters may have re-registered the keys
        weakref.finalize(self, lambda: [_PACKS.pop(k, None) for k in box if (_PACKS.get(k) or (None,))[0] is me])
        self._me = me

    def _add(self, p, kind, N, K, aux=0, p2=None, out_numel=None):
        self.specs.append(PackSpec(p, p2, kind, N, K, aux, out_numel))

    def add_linear(self, w, fwd=True, bwd=True):
        if fwd:
            self._add(w, K_PLAIN, w.shape[0], w.shape[1])
        if bwd:
            self._add(w, K_TRANS, w.shape[1], w.shape[0])

    def add_gates(self, w, H, G=4):
        """gate-interleaved pack of a recurrent weight [G*H, K] (LSTM G = 4, GRU G = 3) — and, for the f16x3 arithmetic, its two
        fp16 planes + the amax word they are normalised by (a kind-9 job of the plan's FIRST launch)."""
        self._add(w, K_GATES, G * H, w.shape[1], aux=H)
        self._add(w, K_GATES_H3, G * H, w.shape[1], aux=H)
        if G == 4:
            # the persistent backward launch (csrc/gpe_rnn_persist.hip) reads W^T through the fp16 pipe
            self._add(w, K_TRANS_H3, w.shape[1], G * H)

    def add_edge_first(self, w1, b1):
        H, C2 = w1.shape
        C = C2 // 2
        self._add(w1, K_PQ, 2 * H, C, aux=H)
        self._add(w1, K_PQT, C, 2 * H, aux=H)
        self._add(b1, K_BPQ, 2 * H, 0, aux=H, out_numel=2 * H)

    def add_bias_sum(self, b_ih, b_hh):
        self._add(b_ih, K_VADD, b_ih.numel(), 0, p2=b_hh, out_numel=b_ih.numel())

    def add_gru_bias(self, b_ih, b_hh, H):
        """b_ih + [b_hr | b_hz | 0]: nn.GRU keeps b_hn inside the r-gated term."""
        self._add(b_ih, K_GRUB, b_ih.numel(), 0, aux=2 * H, p2=b_hh, out_numel=b_ih.numel())

    def _versions(self):
        return [sp.p._version + (sp.p2._version if sp.p2 is not None else 0) for sp in self.specs]

    def _build(self):
        for k in self.keys:
            if (_PACKS.get(k) or (None,))[0] is self._me:
                _PACKS.pop(k, None)
        self.keys, self.outs = [], []
        del self._keys_box[:]
        dev = self.specs[0].p.device
        # f16x3 plane packs are normalised by their tensor's largest magnitude: one amax word per MATRIX (its gate-interleaved and
        # its transposed planes share it), numbered by first appearance and filled by a kind-9 job of an EARLIER launch
        # (self.pre_table) into self.words (zeroed before every refresh)
        mats = {id(sp.p): sp.p for sp in self.specs if sp.kind in PLANE_KINDS}       # (a dict keeps the order of first insertion)
        self.words = torch.zeros(max(len(mats), 1), device=dev, dtype=torch.int32)
        word = {m: self.words[wi:wi + 1] for wi, m in enumerate(mats)}
        pre = [(p.data_ptr(), 0, word[m].data_ptr(), p.numel(), p.stride(0), p.shape[0], p.shape[1], K_AMAX, 0, 0) for m, p in mats.items()]
        self.pre_table, self.pre_blocks = _job_table(pre, dev) if mats else (None, 0)
        rows, self.word_of = [], {}
        for i, sp in enumerate(self.specs):
            npad, total = _pack_geometry(sp)
            out = torch.empty(total, device=dev, dtype=F32)
            self.outs.append(out)
            key = (sp.p.data_ptr(), sp.kind)
            w2 = sp.p2.data_ptr() if sp.p2 is not None else 0
            if sp.kind in PLANE_KINDS:
                self.word_of[key] = word[id(sp.p)]
                w2 = word[id(sp.p)].data_ptr()
            rows.append((sp.p.data_ptr(), w2, out.data_ptr(), total, sp.p.stride(0) if sp.p.dim() == 2 else 0, sp.N, sp.K, sp.kind, npad, sp.aux))
            _PACKS[key] = (self._me, out, i)
            self.keys.append(key)
            self._keys_box.append(key)
        self.table, self.blocks = _job_table(rows, dev)
        # the same table without the fp16-plane jobs, for every arithmetic mode but f16x3 (their outputs and amax words are only
        # read by the f16x3 recurrences: ADVICE r4 — two launches and the plane arithmetic per step for nothing)
        noh3 = [row for row, sp in zip(rows, self.specs) if sp.kind not in PLANE_KINDS]
        self.table_noh3, self.blocks_noh3 = _job_table(noh3, dev) if mats else (self.table, self.blocks)
        self.n_noh3 = len(noh3)
        self.home = self._home()

    def _home(self):
        """where every source parameter lives right now: the job table holds raw pointers, so ANY parameter that moved
        (a partial re-homing, `p.data = ...` on a subset) must rebuild it"""
        return tuple((sp.p.data_ptr(), sp.p2.data_ptr() if sp.p2 is not None else 0, sp.p.device) for sp in self.specs)

    def refresh(self):
        """Called at the start of a model forward: one gpe_pack_multi launch (skipped only by a `frozen` plan whose parameters'
        version counters and WEIGHTS_EPOCH did not move)."""
        if not self.specs:
            return
        vers = self._versions()
        first = self.specs[0].p
        if first.is_cuda:
            st = torch.cuda.current_stream(first.device)
            if self._stream is not None and st != self._stream:
                st.wait_stream(self._stream)     # the packs / words the previous stream's launches still read are about to change
            self._stream = st
        rebuilt = self.table is None or self.home != self._home()
        if rebuilt:
            self._build()                      # first use, or a parameter moved (.to(device), arena re-homing)
        h3 = self.pre_table is not None and L.get_math() == 'f16x3'        # the planes are wanted now
        if not rebuilt and self.frozen and self.vers == vers and self.epoch == WEIGHTS_EPOCH and self.h3_current == h3:
            return                             # (a mode change re-runs the packs)
        self.h3_current = h3
        if h3:
            self.words.zero_()
            L.call('gpe_pack_multi', self.pre_table, self.pre_table.numel() // 64, self.pre_blocks)
            L.call('gpe_pack_multi', self.table, len(self.specs), self.blocks)
        else:
            L.call('gpe_pack_multi', self.table_noh3, self.n_noh3, self.blocks_noh3)
        self.vers, self.epoch = vers, WEIGHTS_EPOCH


def _current(t, kind, t2=None):
    """-> (plan, its persistent packed operand of parameter `t`) if a PackPlan owns one that is still current, else (None, None)"""
    hit = _PACKS.get((t.data_ptr(), kind))
    if hit is None:
        return None, None
    ref, out, i = hit
    plan = ref()
    if plan is None or plan.vers is None or plan.epoch != WEIGHTS_EPOCH:
        return None, None
    if plan.vers[i] != t._version + (t2._version if t2 is not None else 0):
        return None, None
    return plan, out


def _planned(t, kind, t2=None):
    """The persistent packed operand of parameter `t` if a PackPlan owns one that is still current, else None."""
    return _current(t, kind, t2)[1]


# -------------------------------------------------------------------------------------------------
# gradient sink (optim.FlatArena): weight gradients are written straight into the arena
# -------------------------------------------------------------------------------------------------
_SINK = {}                 # param data_ptr -> (weakref to the arena, flat gradient view shaped like the parameter)


def _gbuf(param, shape=None):
    """Output buffer for the gradient of `param`: the arena view if the parameter is registered, else a new tensor."""
    hit = _SINK.get(param.data_ptr())
    if hit is not None and hit[0]() is not None:
        return hit[1]
    return torch.empty(param.shape if shape is None else shape, device=param.device, dtype=F32)


def _gret(param, buf):
    """What backward returns for `param`: None when the gradient already sits in the arena (and the arena is told, so that
    a gradient bucket can leave for the all-reduce), else the tensor itself."""
    hit = _SINK.get(param.data_ptr())
    arena = hit[0]() if hit is not None else None
    if arena is None:
        return buf
    arena.mark_written(param)
    return None


# -------------------------------------------------------------------------------------------------
# raw wrappers
# -------------------------------------------------------------------------------------------------
def pack_weight(w, transpose=False, col_scale=None):
    """w: [N,K] (nn.Linear layout).  transpose=True packs w^T (operand [K_src_cols][K_src_rows])."""
    _dev_check(w)
    assert w.dim() == 2 and w.stride(1) == 1
    if col_scale is None:
        hit = _planned(w, K_TRANS if transpose else K_PLAIN)
        if hit is not None:
            return hit
    N, K = (w.shape[1], w.shape[0]) if transpose else (w.shape[0], w.shape[1])
    wp = torch.empty(L.query('gpe_packed_size', N, K), device=w.device, dtype=F32)
    L.call('gpe_pack_weight', w, w.stride(0), N, K, int(transpose), col_scale, wp)
    return wp


def pack_gates(w, H, G=4):
    """gate-interleaved pack of a recurrent weight [G*H, K]: one column block = the G gates of 16 units."""
    hit = _planned(w, K_GATES)
    if hit is not None:
        return hit
    wp = torch.empty(L.query('gpe_packed_ngates_size', H, G, w.shape[1]), device=w.device, dtype=F32)
    L.call('gpe_pack_weight_ngates', w, w.stride(0), H, G, w.shape[1], wp)
    return wp


def planned_planes(w, kind):
    """(fp16 plane pack, amax word) of a recurrent weight when a PackPlan owns them (f16x3 arithmetic of the recurrences), else
    (None, None): the wavefront kernels then run the exact fp32 instruction."""
    plan, out = _current(w, kind)
    if plan is None or not plan.h3_current:                  # (planes are only rebuilt by a refresh that ran in f16x3 mode)
        return None, None
    return out, plan.word_of.get((w.data_ptr(), kind))


def bias_sum(b_ih, b_hh):
    hit = _planned(b_ih, K_VADD, b_hh)
    if hit is not None:
        return hit
    out = torch.empty_like(b_ih)
    L.call('gpe_add', b_ih, b_hh, out, b_ih.numel())
    return out


def gru_bias(b_ih, b_hh, H):
    hit = _planned(b_ih, K_GRUB, b_hh)
    if hit is not None:
        return hit
    out = b_ih.detach().clone()
    L.call('gpe_add', b_ih, b_hh, out, 2 * H)
    return out


def _ptr_array(tensors):
    """host array of device pointers (the `const void* const*` arguments of the wavefront recurrences)."""
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def edge_first_operands(W1, b1):
    """-> (packed [W1a-W1b ; W1b], its packed transpose, bias [b1 | 0]) for the per-point P|Q projection."""
    H, C = W1.shape[0], W1.shape[1] // 2
    a, b, c = _planned(W1, K_PQ), _planned(W1, K_PQT), _planned(b1, K_BPQ)
    if a is not None and b is not None and c is not None:
        return a, b, c
    wpq = torch.empty(2 * H, C, device=W1.device, dtype=F32)
    bpq = torch.empty(2 * H, device=W1.device, dtype=F32)
    L.call('gpe_w1_split', W1, W1.stride(0), b1, H, C, wpq, C, bpq)
    return pack_weight(wpq), pack_weight(wpq, transpose=True), bpq


def fold_bias(w, bias, t):
    out = torch.empty(w.shape[0], device=w.device, dtype=F32)
    L.call('gpe_fold_bias', w, w.stride(0), w.shape[0], w.shape[1], bias, t, out)
    return out


def linear_raw(a_desc, wp, bias, M, N, K, y_desc, act=0, addend_desc=None):
    ad = addend_desc if addend_desc is not None else (None, 0, 0, 0)
    L.call('gpe_linear', a_desc[0], a_desc[1], a_desc[2], a_desc[3], wp, bias,
           ad[0], ad[1], ad[2], ad[3], y_desc[0], y_desc[1], y_desc[2], y_desc[3], M, N, K, act)


def redgemm_raw(u_desc, v_desc, rows, Mg, Ng, want_colsum=True, accumulate_into=None, v_shift=None, out=None):
    """G[Mg,Ng] = sum_r U[r,:]^T (V[r,:] - v_shift), colsum[Mg] = sum_r U[r,:].  `out` = (G, colsum) buffers to fill."""
    dev = u_desc[0].device
    if accumulate_into is not None:
        G, cs = accumulate_into
    elif out is not None:
        G, cs = out
    else:
        G = torch.empty(Mg, Ng, device=dev, dtype=F32)
        cs = torch.empty(Mg, device=dev, dtype=F32) if want_colsum else None
    acc = int(accumulate_into is not None)
    for n0 in range(0, Ng, 256):          # the kernel keeps <= 256 V columns resident per pass
        nb = min(256, Ng - n0)
        ws = torch.empty(L.query('gpe_redgemm_ws', Mg, nb), device=dev, dtype=F32)
        L.call('gpe_redgemm', u_desc[0], u_desc[1], u_desc[2], u_desc[3],
               v_desc[0][..., n0:], v_desc[1], v_desc[2], v_desc[3], None if v_shift is None else v_shift[n0:],
               rows, Mg, nb, G[:, n0:], G.stride(0), cs if n0 == 0 else None, ws, acc)
    return G, cs


def knn(x, B, N, k, want_global=False, order=None, want_order=False):
    """x: [B*N, C] rows (ld = x.stride(0)).  -> int32 [B, N, k] local neighbour indices (and, optionally, the same
    graph as global row numbers b*N + idx, the form the gather kernels consume).
    Replaces torch_cluster.knn under DynamicEdgeConv (nn/net_blocks.py:127-135,174).
    order (int32 [B, N], optional): a locality order of the points, a speed hint for the wide-feature search (include/gpe_hip.h
    gpe_knn); want_order: also return the order this search worked in (the xyz search's Morton-curve order; else the identity)."""
    _dev_check(x)
    idx = torch.empty(B, N, k, device=x.device, dtype=torch.int32)
    jg = torch.empty(B, N, k, device=x.device, dtype=torch.int32) if want_global else None
    oo = torch.empty(B, N, device=x.device, dtype=torch.int32) if want_order else None
    if order is not None:
        assert order.dtype == torch.int32 and order.shape == (B, N) and order.is_contiguous() and order.device == x.device
    nws = L.query('gpe_knn_ws_bytes', B, N, x.shape[1], k)
    L.call('gpe_knn', x, B, N, x.shape[1], x.stride(0), k, idx, jg, order, oo, _workspace(nws, x.device), nws)
    out = (idx, jg) if want_global else (idx,)
    if want_order:
        out = out + (oo,)
    return out if len(out) > 1 else out[0]


def knn_reverse(idx):
    B, N, k = idx.shape
    off = torch.empty(B, N + 1, device=idx.device, dtype=torch.int32)
    edge = torch.empty(B, N * k, device=idx.device, dtype=torch.int32)
    L.call('gpe_knn_reverse', idx, B, N, k, off, edge)
    return off, edge


def bn_finalize(part, nblk, C, count, gamma, beta, eps, momentum, rm, rv, nbt):
    stats = torch.empty(4, C, device=gamma.device, dtype=F32)
    L.call('gpe_bn_finalize', part, nblk, C, float(count), gamma, beta, float(eps), float(momentum), rm, rv, nbt,
           stats)
    return stats


def bn_from_running(rm, rv, gamma, beta, eps):
    C = gamma.shape[0]
    stats = torch.empty(4, C, device=gamma.device, dtype=F32)
    L.call('gpe_bn_from_running', rm, rv, C, gamma, beta, float(eps), stats)
    return stats


def bn_bwd_coef(part, nblk, stats, C, count, gamma=None, beta=None, training=True):
    """-> coef [4][C] = {s, c1, k2, mean}, dgamma, dbeta (written into the parameters' gradient buffers).  In eval mode the
    statistics are constants, so the projection terms c1 / k2 vanish (dz = s * dy under the ReLU mask)."""
    dev = stats.device
    coef = torch.empty(4, C, device=dev, dtype=F32)
    dg = _gbuf(gamma) if gamma is not None else torch.empty(C, device=dev, dtype=F32)
    db = _gbuf(beta) if beta is not None else torch.empty(C, device=dev, dtype=F32)
    L.call('gpe_bn_bwd_coef', part, nblk, stats, C, float(count), coef, dg, db)
    if not training:
        coef[1:3].zero_()
    return coef, dg, db


def bn_stats(blk, eps, training=False, momentum=None, part=None, nblk=0, count=0):
    """-> the BatchNorm stat block of the MLPBlock `blk`: from this batch's partial sums, or in eval mode from the running statistics"""
    if training:
        return bn_finalize(part, nblk, blk.W.shape[0], count, blk.gamma, blk.beta, eps, momentum, blk.running_mean, blk.running_var,
                           blk.num_batches_tracked)
    return bn_from_running(blk.running_mean, blk.running_var, blk.gamma, blk.beta, eps)


# -------------------------------------------------------------------------------------------------
# the tensors of a net_blocks.MLP as autograd takes them: flat, 4 parameters per block, then 3 buffers per block
# -------------------------------------------------------------------------------------------------
MLP_PARAMS, MLP_BUFFERS = ('W', 'b', 'gamma', 'beta'), ('running_mean', 'running_var', 'num_batches_tracked')
MLPBlock = collections.namedtuple('MLPBlock', MLP_PARAMS + MLP_BUFFERS, defaults=(None,) * len(MLP_BUFFERS))


def mlp_tensors(mlp):
    """mlp: the nn.Sequential parameter container built by net_blocks.MLP -> (eps, momentum, nb, the flat tuple of its tensors)"""
    blocks = [mlp[i] for i in range(len(mlp))]
    flat = [t for lin, _, bn in blocks for t in (lin.weight, lin.bias, bn.weight, bn.bias)]
    flat += [t for _, _, bn in blocks for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    return blocks[0][2].eps, blocks[0][2].momentum, len(blocks), tuple(flat)


def mlp_blocks(tensors, nb):
    """the inverse of mlp_tensors: nb MLPBlock records (of the 4 nb parameters alone, as a backward saves them: no buffers, None)"""
    P, Q = len(MLP_PARAMS), len(MLP_BUFFERS)
    return [MLPBlock(*tensors[P * l: P * l + P], *tensors[P * nb + Q * l: P * nb + Q * l + Q]) for l in range(nb)]


def mlp_grads(lead, nb, filed=None, gx=None):
    """What the backward of a Function whose forward took (x, lead - 1 more arguments, *mlp_tensors) returns: gx, None up to the tensors,
    the gradients `filed` as {(block, parameter field): tensor} at their places in mlp_tensors' order, None for every buffer"""
    out = [gx] + [None] * (lead - 1 + (len(MLP_PARAMS) + len(MLP_BUFFERS)) * nb)
    for (l, field), g in (filed or {}).items():
        out[lead + len(MLP_PARAMS) * l + MLP_PARAMS.index(field)] = g
    return tuple(out)


def save_groups(ctx, **groups):
    """ctx.save_for_backward of named groups, flattened in the order given; a group is one tensor or a list of tensors"""
    ctx.saved_groups = [(name, len(g) if isinstance(g, (list, tuple)) else None) for name, g in groups.items()]
    ctx.save_for_backward(*[t for g in groups.values() for t in (g if isinstance(g, (list, tuple)) else (g,))])


def saved_groups(ctx):
    """-> {name: group} of what save_groups(ctx, ...) saved"""
    sv, at, out = ctx.saved_tensors, 0, {}
    for name, n in ctx.saved_groups:
        out[name] = sv[at] if n is None else list(sv[at: at + n])
        at += 1 if n is None else n
    return out


# -------------------------------------------------------------------------------------------------
# the three big edge entry points by keyword (include/gpe_hip.h): each ends in its one L.call, arguments in the header's order
# -------------------------------------------------------------------------------------------------
EdgeSrc = collections.namedtuple('EdgeSrc', 'pq ldpq jg t ld')   # the rows an edge kernel reads: gathered relu(P_i + Q_j), or dense [E][ld]
NO_LAZY = (None, 0, None, None, 0, None)                         # lz_g, lz_ldg, lz_amx, lz_amn, lz_ldagg, lz_coef: no lazy dz3


def edge_gathered(PQ, jg):
    return EdgeSrc(PQ, PQ.stride(0), jg, None, 0)


def edge_rows(t):
    return EdgeSrc(None, 0, None, t, t.stride(0))


def edge_mlp_fwd(*, src, dims, Cin, Cout, wp, bias, out, ldo, stats_part, agg, ldagg, amax_a, amax_out, ws, out_half):
    """dims = (B, N, k); agg = (mx, mn, amx, amn), [B*N][ldagg] each, or None; ws = edge_workspace(...)"""
    mx, mn, amx, amn = agg or (None, None, None, None)
    L.call('gpe_edge_mlp_fwd', int(src.pq is None), *src, *dims, Cin, Cout, wp, bias, out, ldo, stats_part, int(agg is not None),
           mx, mn, amx, amn, ldagg, amax_a, amax_out, *ws, out_half)


def edge_redgemm(*, u, ldu, v, v_shift, dims, Mg, Ng, G, ldG, colsum, part, amax_u, amax_v, ws, lazy=NO_LAZY):
    L.call('gpe_edge_redgemm', u, ldu, int(v.pq is None), v.t, v.ld, v.pq, v.ldpq, v.jg, v_shift, *dims, Mg, Ng, G, ldG, colsum, part,
           amax_u, amax_v, *ws, *lazy)


def edge_mlp_bwd(*, a, lda, act, dims, Cin, Cout, wp, coef, out, ldo, dP, lddp, amax_a, amax_out, ws, lazy=NO_LAZY):
    """act: the edge_gathered(..) activation that is crossed, or None = the one stored in `out`, overwritten in place"""
    pq, ldpq, jg = (None, 0, None) if act is None else act[:3]
    L.call('gpe_edge_mlp_bwd', a, lda, int(act is not None), pq, ldpq, jg, *dims, Cin, Cout, wp, coef, out, ldo, dP, lddp,
           amax_a, amax_out, *ws, *lazy)


def _block_bwd(filed, blocks, l, dz, src, st_prev, dims, count, training, amax, ws, part, lazy=NO_LAZY, first=None):
    """Backward across block l >= 1 of an MLP (EdgeConvFn, DenseMLPFn): weight gradient = centred reduce-GEMM of dz against the block's
    input rows `src` -> coefficients of the BatchNorm in front -> propagate.  Files the gradients of W_l, b_l, gamma_{l-1}, beta_{l-1};
    -> dz_{l-1}: in place over the stored activation src.t, or with first = (dst, dPQ) — src is the gathered first block — in dst, its
    sums over each point's slots in dPQ.  amax: the words of (dz_l, src, dz_{l-1}); part: the reduce-GEMM's partials, None = an input
    wider than the edge kernel takes (the row reduce-GEMM); lazy: dz_l is formed from the stored activation by its two consumers."""
    W, b, gp, bp = blocks[l].W, blocks[l].b, blocks[l - 1].gamma, blocks[l - 1].beta
    Cl, Cp = W.shape[0], blocks[l - 1].W.shape[0]
    G = torch.empty(Cl, Cp, device=W.device, dtype=F32)
    db = _gbuf(b)
    if part is None:
        redgemm_raw((dz, dz.stride(0), 0, 0), (src.t, src.ld, 0, 0), count, Cl, Cp, v_shift=st_prev[0], out=(G, db))
    else:
        edge_redgemm(u=dz, ldu=dz.stride(0), v=src, v_shift=st_prev[0], dims=dims, Mg=Cl, Ng=Cp, G=G, ldG=Cp, colsum=db, part=part,
                     amax_u=amax[0], amax_v=amax[1], ws=ws, lazy=lazy)
    sums = torch.empty(1, 2, Cp, device=W.device, dtype=torch.float64)
    dW = _gbuf(W)
    L.call('gpe_bn_bwd_from_G', G, Cp, db, W, W.stride(0), Cl, Cp, st_prev, sums, dW, Cp)
    coef_p, dgp, dbp = bn_bwd_coef(sums, 1, st_prev, Cp, count, gp, bp, training)
    filed[l, 'W'], filed[l, 'b'] = _gret(W, dW), _gret(b, db)
    filed[l - 1, 'gamma'], filed[l - 1, 'beta'] = _gret(gp, dgp), _gret(bp, dbp)
    # dz_{l-1} = (a>0) ? s*(dz_l W_l) - c1 - (a-mean)*k2 : 0 with a = the activation of block l - 1, stored or re-gathered
    (out, ldo), (dP, lddp) = ((src.t, src.ld), (None, 0)) if first is None else ((first[0], Cp), (first[1], first[1].stride(0)))
    edge_mlp_bwd(a=dz, lda=dz.stride(0), act=None if first is None else src, dims=dims, Cin=Cl, Cout=Cp,
                 wp=pack_weight(W, transpose=True), coef=coef_p, out=out, ldo=ldo, dP=dP, lddp=lddp, amax_a=amax[0], amax_out=amax[2],
                 ws=ws, lazy=lazy)
    return out


# -------------------------------------------------------------------------------------------------
# nn.Linear
# -------------------------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    """y = act(x W^T + b) on the MFMA row-GEMM; backward = row-GEMM (dx) + reduce-GEMM (dW, db).
    Replaces torch.nn.Linear at nn/net_blocks.py:158,187,397 and nn/nets.py:128-130,153,229-233.
    x: [M, K] rows, or a strided [R, T, K] view (e.g. the top-layer h history of a recurrent stack) -> y [R*T, N]."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _dev_check(x)
        K = x.shape[-1]
        M = x.numel() // K
        N = weight.shape[0]
        y = torch.empty(M, N, device=x.device, dtype=F32)
        linear_raw(_rows3d(x) if x.dim() == 3 else _rows2d(x), pack_weight(weight), bias, M, N, K, _rows2d(y))
        ctx.save_for_backward(x, weight, bias)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, bias = ctx.saved_tensors
        gy = gy.contiguous()
        K = x.shape[-1]
        M = x.numel() // K
        N = weight.shape[0]
        xd = _rows3d(x) if x.dim() == 3 else _rows2d(x)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty(*x.shape, device=x.device, dtype=F32)
            linear_raw(_rows2d(gy), pack_weight(weight, transpose=True), None, M, K, N, (gx, K, 0, 0))
        if ctx.needs_input_grad[1] or bias is not None:
            # (a leaf of the backward pass: on the side stream when weight and bias gradients both land in the arena)
            with side_grads([weight, bias] if bias is not None else [], [gy, x]):
                gw = _gbuf(weight)
                gb = _gbuf(bias) if bias is not None else torch.empty(N, device=x.device, dtype=F32)
                redgemm_raw(_rows2d(gy), xd, M, N, K, out=(gw, gb))
                gw = _gret(weight, gw)
                gb = _gret(bias, gb) if bias is not None else None
        return gx, gw, gb


def linear(x, weight, bias=None):
    return LinearFn.apply(x, weight, bias)


# -------------------------------------------------------------------------------------------------
# global pooling
# -------------------------------------------------------------------------------------------------
POOL_MODES = {'mean': 0, 'max': 1, 'add': 2}


class SegmentMeanFn(torch.autograd.Function):
    """torch_geometric.nn.global_mean_pool over equal-sized clouds (nn/net_blocks.py:148,184; nn/nets.py:272)."""

    @staticmethod
    def forward(ctx, x, B, N):
        _dev_check(x)
        C = x.shape[1]
        y = torch.empty(B, C, device=x.device, dtype=F32)
        L.call('gpe_segment_mean_fwd', x, x.stride(0), B, N, C, y, C)
        ctx.dims = (B, N, C)
        return y

    @staticmethod
    def backward(ctx, gy):
        B, N, C = ctx.dims
        gy = gy.contiguous()
        gx = torch.empty(B * N, C, device=gy.device, dtype=F32)
        L.call('gpe_segment_mean_bwd', gy, C, B, N, C, gx, C, 0)
        return gx, None, None


class SegmentPoolFn(torch.autograd.Function):
    """torch_geometric.nn.global_max_pool / global_add_pool over equal-sized clouds (nn/net_blocks.py:145-150)."""

    @staticmethod
    def forward(ctx, x, B, N, mode):
        _dev_check(x)
        C = x.shape[1]
        y = torch.empty(B, C, device=x.device, dtype=F32)
        arg = torch.empty(B, C, device=x.device, dtype=torch.int32) if mode == 1 else None
        L.call('gpe_segment_pool_fwd', x, x.stride(0), B, N, C, mode, y, C, arg)
        ctx.dims = (B, N, C, mode)
        ctx.arg = arg
        return y

    @staticmethod
    def backward(ctx, gy):
        B, N, C, mode = ctx.dims
        gy = gy.contiguous()
        gx = torch.empty(B * N, C, device=gy.device, dtype=F32)
        L.call('gpe_segment_pool_bwd', gy, C, ctx.arg, B, N, C, mode, gx, C)
        return gx, None, None, None


def segment_mean(x, B, N):
    return SegmentMeanFn.apply(x, B, N)


def segment_max(x, B, N):
    return SegmentPoolFn.apply(x, B, N, 1)


def segment_add(x, B, N):
    return SegmentPoolFn.apply(x, B, N, 2)


segment_mean.pool_mode, segment_max.pool_mode, segment_add.pool_mode = 0, 1, 2


# -------------------------------------------------------------------------------------------------
# EdgeConv layer
# -------------------------------------------------------------------------------------------------
_HALF_ACT_GUARD = 'fallback'
# graph.StepGraph: CAPTURE is the StepGraph whose hipGraph capture is in progress (host reads are impossible then), HOST_DRAWN the
# provider of host-drawn device tensors (start states, dropout masks) while a StepGraph drives the step — else None
CAPTURE = None
HOST_DRAWN = None


def set_half_act_guard(mode):
    """What watches the fp16 storage of the aggregated block's activation (f16x3 mode, lazy dz3; DESIGN.md 8 row g).  The stored
    copy is clamped at 65504 and flushes positives below 6e-8; the forward measures the activation's true largest magnitude
    (an amax word on the device) — this guard reads it:
      'fallback' (default)  asynchronously, one step late and without a host synchronisation: a layer whose activation reached
                            the fp16 limit switches to fp32 storage + the eager dz3 pass for every later step, with a RuntimeWarning
                            (the step that tripped the guard ran with clamped values: its gradient elements of the clamped
                            activations are off);
      'strict'              synchronously inside the forward (one host read per EdgeConv layer and step): the launch is repeated
                            with fp32 storage before anything consumes the clamped rows — exact at every step;
      'off'                 no check (rounds 3 - 4 behaviour).
    Returns the previous mode."""
    global _HALF_ACT_GUARD
    if mode not in ('fallback', 'strict', 'off'):
        raise ValueError("half-activation guard mode must be 'fallback', 'strict' or 'off'")
    prev, _HALF_ACT_GUARD = _HALF_ACT_GUARD, mode
    return prev


if os.environ.get('GPE_HALF_ACT_GUARD'):                 # (validated: a typo raises instead of silently meaning 'fallback')
    set_half_act_guard(os.environ['GPE_HALF_ACT_GUARD'])


# The amax words handed to HalfActGuard.watch since the last optim.FlatArena.begin_step(), per device ordinal.  Bounded: a model that
# is never stepped through a FlatArena keeps the newest few only (FusedAdam takes at most eight and refuses more).
_WATCHED = {}
_WATCHED_KEEP = 9


def watched_words(device):
    """-> the amax words (int32[1] device tensors) recorded on `device` since the arena's last begin_step()."""
    return list(_WATCHED.get(torch.device(device).index, ()))


def clear_watched_words(device):
    rec = _WATCHED.get(torch.device(device).index)
    if rec:
        rec.clear()


class HalfActGuard:
    """Per-layer state of set_half_act_guard: owned by the module that owns the layer (net_blocks.DynamicEdgeConv)."""
    LIMIT = 65504.0

    def __init__(self):
        self.disabled = False
        self.last_amax = None
        self._pending = None

    def __getstate__(self):                              # copies / pickles of the owning module carry the decision, not the
        return {'disabled': self.disabled, 'last_amax': self.last_amax, '_pending': None}    # in-flight read (pinned buffer + event)

    def __deepcopy__(self, memo):
        g = HalfActGuard()
        g.disabled, g.last_amax = self.disabled, self.last_amax
        return g

    @staticmethod
    def _value(host):
        return float(np.array([int(host[0])], dtype=np.int32).view(np.float32)[0])

    def _trip(self, v):
        self.disabled = True
        warnings.warn('f16x3: the aggregated EdgeConv activation reached %.3g (fp16 storage clamps at 65504): this layer keeps it '
                      'in fp32 and forms dz3 eagerly from now on (gpe_amd.ops.set_half_act_guard)' % v, RuntimeWarning, stacklevel=3)

    def allow(self):
        """May the coming forward store the activation in fp16?  Polls the previous step's word without blocking."""
        if _HALF_ACT_GUARD == 'off':
            return True
        if CAPTURE is not None:                          # no polling inside a capture: the decision as it stands
            return not self.disabled
        if self._pending is not None and self._pending[1].query():
            v = self._value(self._pending[0])
            self._pending = None
            self.last_amax = v
            if not v < self.LIMIT:                      # (also true for NaN)
                self._trip(v)
        return not self.disabled

    def watch(self, word):
        """After the forward launch that filled `word` (int32[1], the activation's amax bits).  'strict': returns False when the
        launch must be repeated with fp32 storage.  The word of a launch whose fp16 rows stay in use is also put on the device's
        record of watched words (watched_words), eagerly and during a capture: optim.FusedAdam(guard_overflow=True) hands them to
        its norm pass, which leaves the weights alone in the step that reached the limit."""
        ok = self._watch(word)
        if ok:
            _WATCHED.setdefault(word.device.index, collections.deque(maxlen=_WATCHED_KEEP)).append(word)
        return ok

    def _watch(self, word):
        """watch() without the record (graph.StepGraph polls the captured words again after every replay)."""
        if _HALF_ACT_GUARD == 'off':
            return True
        if CAPTURE is not None:                          # the StepGraph reads this word after every replay
            CAPTURE.guards.append((self, word))
            return True
        if _HALF_ACT_GUARD == 'strict':
            v = self._value(word.cpu())
            self.last_amax = v
            if not v < self.LIMIT:
                self._trip(v)
                return False
            return True
        if self._pending is not None:
            # an earlier step's read has not been consumed: look at it now if it has landed, and otherwise KEEP it — the oldest unread
            # word is the one that says when the limit was first reached (a newer read must not overwrite it: ADVICE r5)
            self.allow()
            if self._pending is not None:
                return True
        host = torch.empty(1, dtype=torch.int32, pin_memory=True)
        host.copy_(word, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending = (host, ev)
        return True


class EdgeConvFn(torch.autograd.Function):
    """One DynamicEdgeConv(MLP([2C, H, .., H, F]), k, aggr) layer (nn/net_blocks.py:43-47,124-135,174):
    kNN graph on the input features -> per-edge [Linear->ReLU->BatchNorm] x nb -> max / mean / add over the k messages.

    Pipeline (training): kNN | per-point P,Q GEMM (block 0 split: W1.[x_i, x_j-x_i] = P_i + Q_j) | gather+stats(a_0) |
    for every further block: fold the previous BatchNorm into this Linear, fused (gather|dense)+GEMM+ReLU(+stats)
    (+max/min over the point's messages in the last block) | last BatchNorm applied AFTER the aggregation.
    Saved for backward: the graph, PQ, the post-ReLU activations a_1..a_{nb-1} [E, .], the aggregates, the BN stat blocks.
    nb = EConv_hidden_depth + 1 >= 2; the shipped configs use nb = 3, aggr = 'max'."""
    LEAD = 11                                              # forward's arguments in front of *tensors (x .. order)

    @staticmethod
    def forward(ctx, x, B, N, k, training, eps, momentum, nb, aggr, guard, order, *tensors):
        # order (int32 [B, N] or None): a locality order of the points — the previous layer's curve order — handed to the graph
        # search as a speed hint (include/gpe_hip.h gpe_knn); third output: the order this layer's search worked in
        _dev_check(x)
        ctx.set_materialize_grads(False)                   # (no zero tensors for the gradients of idx / order_out)
        dev = x.device
        BN, C = x.shape
        assert BN == B * N
        blocks = mlp_blocks(tensors, nb)
        widths = [blk.W.shape[0] for blk in blocks]
        H0 = widths[0]
        assert blocks[0].W.shape[1] == 2 * C
        if H0 % 4 or H0 > 256:
            raise ValueError('EdgeConvFn (the fused P|Q path) needs a first-block width that is a multiple of 4 and <= 256 '
                             '(got %d): use ops.edge_conv_general' % H0)
        E = BN * k
        _LAST_EDGES[0] = E                                 # (what side_grads takes for the size of the step)
        nblk = L.query('gpe_stats_blocks')
        wpq_p, _, bpq = edge_first_operands(blocks[0].W, blocks[0].b)
        ldws = max(round_up(widths[-1], 4), 2 * H0)
        ews = edge_workspace(B, N, k, ldws, dev)
        words = f16x3_words(2 * nb + 1, E, dev)           # (+ 1: max |s g| of the layer-output gradient, lazy dz3)

        def project(own_ws):
            PQ = torch.empty(BN, 2 * H0, device=dev, dtype=F32)
            linear_raw(_rows2d(x), wpq_p, bpq, BN, 2 * H0, C, _rows2d(PQ))
            if words is not None:
                L.call('gpe_edge_pq_amax', PQ, 2 * H0, H0, BN, _word(words, 0), *(edge_workspace(B, N, k, ldws, dev) if own_ws else ews))
            return PQ

        # The [P|Q] projection (and its f16x3 bound) needs the layer input only — not the graph: on a GPU-bound step it runs on the
        # side stream beside the graph search, whose kernels leave most of the chip's issue slots empty
        fork = SIDE_PQ and _side_ok(E)
        if fork:
            lane = streams.lane(dev.index)
            with lane.fork([x, words]):                     # (joined below, once the graph search is queued)
                PQ = project(own_ws=True)                   # (the side stream's own workspace)
            idx, jg, order_out = knn(x, B, N, k, want_global=True, order=order, want_order=True)
            lane.wait(made=[PQ])
        else:
            idx, jg, order_out = knn(x, B, N, k, want_global=True, order=order, want_order=True)
            PQ = project(own_ws=False)

        # caller-owned state of the edge calls: one workspace, and in f16x3 mode the amax words of this layer's tensors —
        # [0] the bound of relu(P_i + Q_j), [l] activation a_l, [nb + l] dz_l (backward)
        part = torch.empty(nblk, 2, H0, device=dev, dtype=torch.float64) if training else None
        if training:
            L.call('gpe_edge_gather_stats', PQ, 2 * H0, H0, jg, B, N, k, part)
        stats = [bn_stats(blocks[0], eps, training, momentum, part, nblk, E)]
        acts = [None]
        mx = mn = amx = amn = abar = None
        for l in range(1, nb):
            Cin, Cout = widths[l - 1], widths[l]
            ldo = round_up(Cout, 4)
            last = l == nb - 1
            # row g: the aggregated block's activation is kept in fp16 when its backward will form dz3 lazily — its
            # only readers then (include/gpe_hip.h "out_half"; gradients move by 2e-6 / 5e-6 of their maximum)
            half = bool(last and training and aggr == 'max' and words is not None and nb >= 3 and
                        L.query('gpe_edge_lazy_dz3_ok', B, N, k, Cout, Cin) == 1 and (guard is None or guard.allow()))
            a = torch.empty(E, ldo, device=dev, dtype=torch.float16 if half else F32)
            part = torch.empty(nblk, 2, Cout, device=dev, dtype=torch.float64) if training else None
            agg = None
            if last and aggr == 'max':
                mx = torch.empty(BN, ldo, device=dev, dtype=F32)
                mn = torch.empty(BN, ldo, device=dev, dtype=F32)
                amx = torch.empty(BN, ldo, device=dev, dtype=torch.uint8)
                amn = torch.empty(BN, ldo, device=dev, dtype=torch.uint8)
                agg = (mx, mn, amx, amn)
            w_out = _word(words, l)                        # (the last activation's word feeds the bound of a lazily formed dz)
            # the BatchNorm fold of this block's Linear: pack + folded bias (+ the packed weight's f16x3 amax) in one launch
            wp, bf = pack_fold(blocks[l].W, blocks[l].b, stats[l - 1], ews[0] if words is not None else None, ews[1], w_out)
            wr = 2 if words is not None else 0             # bit 1 of out_half: the weight's scale is in the workspace
            src = edge_gathered(PQ, jg) if l == 1 else edge_rows(acts[l - 1])

            def launch(a, out_half):
                edge_mlp_fwd(src=src, dims=(B, N, k), Cin=Cin, Cout=Cout, wp=wp, bias=bf, out=a, ldo=ldo, stats_part=part, agg=agg,
                             ldagg=ldo, amax_a=_word(words, l - 1), amax_out=w_out, ws=ews, out_half=out_half)

            launch(a, int(half) | wr)                      # (half: never the gathered block — the aggregated one of nb >= 3)
            if half and guard is not None and not guard.watch(w_out):
                # 'strict' guard: the activation does not fit fp16 — the same launch once more with fp32 rows (nothing has
                # consumed the clamped copy; statistics, maxima and the amax word are rewritten with the same values)
                a = torch.empty(E, ldo, device=dev, dtype=F32)
                launch(a, 0)
            acts.append(a)
            stats.append(bn_stats(blocks[l], eps, training, momentum, part, nblk, E))
        Fo = widths[-1]
        ldF = round_up(Fo, 4)
        out = torch.empty(BN, ldF, device=dev, dtype=F32)[:, :Fo]
        if aggr == 'max':
            L.call('gpe_edge_finish', mx, mn, ldF, stats[-1], BN, Fo, out, ldF)
        else:
            # mean / add: BatchNorm is affine, so it commutes with the sum over the k messages
            abar = torch.empty(BN, ldF, device=dev, dtype=F32)
            L.call('gpe_edge_sum_k', acts[-1], ldF, BN, k, Fo, abar, ldF)
            L.call('gpe_scale', abar, 1.0 / k, abar, abar.numel())
            a_s, t_s = (1.0, 1.0) if aggr == 'mean' else (float(k), float(k))
            L.call('gpe_bn_apply_scaled', abar, ldF, stats[-1], BN, Fo, a_s, t_s, out, ldF)
        ctx.dims = (B, N, k, C, nb, aggr, training)
        ctx.widths = widths
        ctx.done = False
        ctx.words = words
        ctx.rev_job = None
        if fork and training:
            # Work that only a LATER phase of the step needs and that has its inputs early — the transposed graph of the gather backward
            # needs this graph only — waits on the lane for a stretch of the step that leaves the chip idle: the first recurrent stack of
            # the forward (the pattern decoder's persistent launch sits on the CUs of one XCD) launches it there (RNNStackFn.forward)
            if order is None:
                del lane.jobs[:]                             # (a new forward pass: whatever an abandoned one left behind is dropped)
            ctx.rev_job = {'fn': knn_reverse, 'src': idx, 'out': None, 'event': None}
            lane.jobs.append(ctx.rev_job)
        save_groups(ctx, x=x, idx=idx, jg=jg, PQ=PQ, params=tensors[:len(MLP_PARAMS) * nb], acts=acts[1:], stats=stats,
                    tail=[mx, mn, amx, amn] if aggr == 'max' else [abar])
        ctx.mark_non_differentiable(idx, order_out)
        return out, idx, order_out

    @staticmethod
    def backward(ctx, g_out, _g_idx, _g_order=None):
        if ctx.done:
            raise RuntimeError('EdgeConvFn.backward ran twice on the same graph: the stored activations are overwritten '
                               'in place by the first pass (retain_graph is not supported)')
        B, N, k, C, nb, aggr, training = ctx.dims
        if g_out is None:                                  # only the graph / the order were used downstream
            return mlp_grads(EdgeConvFn.LEAD, nb)
        ctx.done = True
        widths = ctx.widths
        sv = saved_groups(ctx)
        x, idx, jg, PQ, stats, tail = sv['x'], sv['idx'], sv['jg'], sv['PQ'], sv['stats'], sv['tail']
        blocks = mlp_blocks(sv['params'], nb)
        acts = [None] + sv['acts']
        dev = x.device
        BN, E = B * N, B * N * k
        H0, Fo = widths[0], widths[-1]
        ldF = round_up(Fo, 4)
        if g_out.stride(1) != 1:
            g_out = g_out.contiguous()
        ldg = g_out.stride(0)
        filed = {}                         # (block, parameter field) -> gradient
        words = ctx.words                  # f16x3 amax words of this layer (None in the other modes): see forward
        ews = edge_workspace(B, N, k, max(ldF, 2 * H0), dev)
        # the transposed graph of the gather backward needs the forward's graph only: on a GPU-bound step it is built on the side stream
        # now and finds its CUs in the gaps between the edge kernels (main waits for it in front of gpe_edge_pull_dq)
        rev, rev_event = None, None
        job = getattr(ctx, 'rev_job', None)
        lane = streams.lane(dev.index)
        if job is not None and job['out'] is not None:
            rev, rev_event = job['out'], job['event']             # built during the forward's idle stretch (Lane.run_jobs)
        elif SIDE_PQ and _side_ok(E):
            if job is not None and job in lane.jobs:
                lane.jobs.remove(job)
            with lane.fork([idx]):                          # (joined in front of gpe_edge_pull_dq)
                rev = knn_reverse(idx)

        # ---- last block: BatchNorm applied after the aggregation -----------------------------------------
        psb = L.query('gpe_point_sums_blocks')
        part = torch.empty(psb, 2, Fo, device=dev, dtype=torch.float64)
        g_last, be_last = blocks[-1].gamma, blocks[-1].beta
        a_last = acts[-1]
        lz = NO_LAZY                                       # lazy dz3 arguments of the two consumers (off)
        if aggr == 'max':
            mx, mn, amx, amn = tail
            # (the forward stored a3 in fp16 exactly when it found the lazy path open; should the mode have changed since — a debug
            # flag, another arithmetic — the eager pass below runs on an fp32 copy)
            lazy = a_last.dtype == torch.float16 and L.query('gpe_edge_lazy_dz3_ok', B, N, k, Fo, widths[-2]) == 1
            if a_last.dtype == torch.float16 and not lazy:
                a_last = a_last.float()
            L.call('gpe_edge_bwd_point_sums', g_out, ldg, mx, mn, ldF, stats[-1], BN, Fo, part,
                   _word(words, 2 * nb) if lazy else None)
            coef, dg, dbe = bn_bwd_coef(part, psb, stats[-1], Fo, E, g_last, be_last, training)
            if lazy:
                # f16x3, k = 16: dz of the aggregated block is never materialised — the weight-gradient reduce-GEMM and the
                # propagation below form it from the stored activation while staging it (the in-place pass is 1.3 GB at cfg 2).
                # Its fp16 scale comes from a bound of |dz|: max |s g| (measured by the point sums above) + the coefficient terms.
                L.call('gpe_edge_dz3_bound', _word(words, 2 * nb), coef, Fo, _word(words, nb - 1), _word(words, 2 * nb - 1))
                lz = (g_out, ldg, amx, amn, ldF, coef)
            else:
                # dz in place over the stored activation (one coalesced pass)
                L.call('gpe_edge_dz3', a_last, ldF, g_out, ldg, amx, amn, ldF, coef, B, N, k, Fo, _word(words, 2 * nb - 1))
        else:
            # every message carries dy_e = w * g_i (w = 1/k mean, 1 add): sums over edges = (w*k) * per-point sums at
            # the mean activation of the point
            abar, = tail
            gs = g_out
            if aggr == 'add':
                gs = torch.empty(BN, Fo, device=dev, dtype=F32)
                L.call('gpe_scale', g_out.contiguous(), float(k), gs, gs.numel())
            L.call('gpe_edge_bwd_point_sums', gs, gs.stride(0), abar, abar, ldF, stats[-1], BN, Fo, part, None)
            coef, dg, dbe = bn_bwd_coef(part, psb, stats[-1], Fo, E, g_last, be_last, training)
            L.call('gpe_edge_dz3_all', a_last, ldF, g_out, ldg, 1.0 / k if aggr == 'mean' else 1.0, coef, B, N, k, Fo,
                   _word(words, 2 * nb - 1))
        filed[nb - 1, 'gamma'], filed[nb - 1, 'beta'] = _gret(g_last, dg), _gret(be_last, dbe)

        # ---- blocks nb-1 .. 1: weight gradient (centred reduce-GEMM) -> previous BN coefficients -> propagate ----
        ws = torch.empty(max(L.query('gpe_redgemm_ws', widths[l], widths[l - 1]) for l in range(1, nb)), device=dev,
                         dtype=F32)
        dPQ = torch.empty(BN, 2 * H0, device=dev, dtype=F32)
        dz = a_last
        for l in range(nb - 1, 1, -1):
            # words: dz_l is written by dz3 (l = nb - 1) or by the propagation of the block behind it
            dz = _block_bwd(filed, blocks, l, dz, edge_rows(acts[l - 1]), stats[l - 1], (B, N, k), E, training,
                            (_word(words, nb + l), _word(words, l - 1), _word(words, nb + l - 1)), ews, ws,
                            lazy=lz if l == nb - 1 else NO_LAZY)
        # the gathered first block: its dz in place over dz_1's buffer when the row pitch fits, else a fresh [E, H0]
        dst = dz if dz.stride(0) == H0 else torch.empty(E, H0, device=dev, dtype=F32)
        dz = _block_bwd(filed, blocks, 1, dz, edge_gathered(PQ, jg), stats[0], (B, N, k), E, training,
                        (_word(words, nb + 1), _word(words, 0), None), ews, ws, first=(dst, dPQ))

        # ---- block 0: gather backward = deterministic pull through the transposed graph -----------------
        if rev is not None:
            rev_off, rev_edge = rev
            lane.wait(made=rev, event=rev_event)
        else:
            rev_off, rev_edge = knn_reverse(idx)
        L.call('gpe_edge_pull_dq', dz, dz.stride(0), rev_off, rev_edge, B, N, k, H0, dPQ[:, H0:], 2 * H0)
        dWpq, dbpq = redgemm_raw(_rows2d(dPQ), _rows2d(x), BN, 2 * H0, C, want_colsum=True)
        W1, b1 = blocks[0].W, blocks[0].b
        dW1 = _gbuf(W1)
        L.call('gpe_w1_grad_from_pq', dWpq, C, H0, C, dW1, 2 * C)
        db1 = _gbuf(b1)
        db1.copy_(dbpq[:H0])
        filed[0, 'W'], filed[0, 'b'] = _gret(W1, dW1), _gret(b1, db1)
        gx = None
        if ctx.needs_input_grad[0]:
            _, wpq_t, _ = edge_first_operands(W1, b1)
            gx = torch.empty(BN, C, device=dev, dtype=F32)
            linear_raw(_rows2d(dPQ), wpq_t, None, BN, C, 2 * H0, _rows2d(gx))
        return mlp_grads(EdgeConvFn.LEAD, nb, filed, gx)


class EdgeInputsFn(torch.autograd.Function):
    """cat[x_i, x_j - x_i] per edge of the kNN graph, materialised [E, 2C] — the general formulation of the DynamicEdgeConv
    message input (nn/net_blocks.py:124-135), used by edge_conv_general for first-block widths the fused P|Q path does not
    take."""

    @staticmethod
    def forward(ctx, x, idx, jg, B, N, k):
        _dev_check(x)
        C = x.shape[1]
        ld = round_up(2 * C, 4)
        out = torch.empty(B * N * k, ld, device=x.device, dtype=F32)
        L.call('gpe_edge_inputs_fwd', x, x.stride(0), C, jg, B * N, k, out, ld)
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, k, C)
        return out[:, :2 * C]

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        B, N, k, C = ctx.dims
        if g.stride(1) != 1:
            g = g.contiguous()
        rev_off, rev_edge = knn_reverse(idx)
        gx = torch.empty(B * N, C, device=g.device, dtype=F32)
        L.call('gpe_edge_inputs_bwd', g, g.stride(0), C, rev_off, rev_edge, B, N, k, gx, C)
        return gx, None, None, None, None, None


def edge_conv_general(x, B, N, k, training, eps, momentum, nb, aggr, tensors):
    """DynamicEdgeConv for first-block widths outside the fused path's menu (EConv_hidden % 4 != 0 or > 256): kNN graph ->
    explicit [x_i, x_j - x_i] rows -> the edge MLP as a dense MLP over the E message rows (DenseMLPFn: the same kernels, every
    BatchNorm incl. the last applied per message) -> max / mean / add over each point's k messages.  Same arithmetic as the
    reference formulation; several times slower than EdgeConvFn (no P|Q split, E-row first block, stored per-edge outputs)."""
    idx, jg = knn(x, B, N, k, want_global=True)
    msg_in = EdgeInputsFn.apply(x, idx, jg, B, N, k)
    msg = DenseMLPFn.apply(msg_in, training, eps, momentum, nb, *tensors)
    if aggr == 'max':
        out = SegmentPoolFn.apply(msg, B * N, k, 1)
    elif aggr == 'add':
        out = SegmentPoolFn.apply(msg, B * N, k, 2)
    else:
        out = SegmentMeanFn.apply(msg, B * N, k)
    return out, idx


# -------------------------------------------------------------------------------------------------
# DynamicEdgeConv at prediction time: one store-free launch per layer (csrc/gpe_edge_predict.hip)
# -------------------------------------------------------------------------------------------------
EDGE_PREDICT_ROUTES = ('auto', 'fused', 'layers')
EDGE_PREDICT_MAX_K, EDGE_PREDICT_MAX_WIDTH, EDGE_PREDICT_MAX_HIDDEN, EDGE_PREDICT_H3_MAX_WIDTH = 64, 256, 3, 224
_AGGR_CODE = {'max': 0, 'mean': 1, 'add': 2}


def _edge_widths_on_menu(shapes, k):
    """shapes: the (out, in) shapes of the edge MLP's Linears"""
    nb = len(shapes)
    if nb < 2 or nb - 2 > EDGE_PREDICT_MAX_HIDDEN or not 1 <= k <= EDGE_PREDICT_MAX_K:
        return False
    H, F = shapes[0][0], shapes[-1][0]
    if H % 4 or not 0 < H <= EDGE_PREDICT_MAX_WIDTH or not 0 < F <= EDGE_PREDICT_MAX_WIDTH:
        return False
    return all(tuple(s) == (H, H) for s in shapes[1:-1]) and shapes[-1][1] == H


def edge_predict_on_menu(mlp, k):
    """can csrc/gpe_edge_predict.hip's fused kernel run this edge MLP (net_blocks.MLP([2C, H, .., H, F])) on k neighbours?  (1 <= k <= 64;
    H <= 256 and a multiple of 4, F <= 256; at most 3 H x H Linears between the first block and the last.)  Pure host logic: the same answer
    as the library's gpe_edge_predict_ok."""
    return _edge_widths_on_menu([tuple(mlp[i][0].weight.shape) for i in range(len(mlp))], k)


def _edge_predict_h3(H, F, E):
    """will gpe_edge_predict_fwd run its fp16-pipe kernel?  (the f16x3 mode, widths its LDS budget takes, past the mode's size gate)"""
    return (L.get_math() == 'f16x3' and H <= EDGE_PREDICT_H3_MAX_WIDTH and F <= EDGE_PREDICT_H3_MAX_WIDTH
            and E >= L.query('gpe_f16x3_min_rows'))


def _edge_predict_auto(H, F, E):
    """the route 'auto' takes on the menu, per arithmetic (profiles/edge_predict.md): measured at BASELINE cfg 2 and 4
    the fused kernel is slower than the layer kernels' eval forward in both arithmetics (f32 x 1.14 - 1.24, f16x3 x 1.27 - 1.76 per
    layer), so 'auto' takes 'layers' in every mode; 'fused' is chosen by name, for its memory (no [E, .] tensor: 147 MB against
    1649 MB per layer at cfg 2)"""
    return 'layers'


def edge_conv_predict(x, B, N, k, nb, aggr, tensors, order=None, route='auto', eps=1e-5):
    """One DynamicEdgeConv layer at prediction time (nn/net_blocks.py:43-47,124-135,174 under eval() and no_grad()).
    x [B*N, C] rows; tensors = the layer's (weight, bias, gamma, beta) x nb + (running_mean, running_var, num_batches_tracked) x nb,
    as EdgeConvFn takes them.  -> (out [B*N, F], idx int32 [B, N, k], order_out) like EdgeConvFn; nothing is recorded for autograd.
    route: 'fused' — kNN, the per-point [P|Q] projection, the BatchNorm folds, then ONE launch that forms, transforms and aggregates
    the k messages of every point in LDS (no [E, .] tensor exists; ValueError off the kernel's menu, edge_predict_on_menu);
    'layers' — EdgeConvFn.forward with training=False, unchanged; 'auto' — 'fused' on the menu where DESIGN.md 5.34 measured it no slower
    than the eval forward, 'layers' otherwise: today 'layers' in every arithmetic mode (the fused route is chosen by name, for its
    memory)."""
    if route not in EDGE_PREDICT_ROUTES:
        raise ValueError('unknown route %r (choose from %s)' % (route, EDGE_PREDICT_ROUTES))
    if aggr not in _AGGR_CODE:
        raise ValueError("unsupported aggregation '%s'" % aggr)
    if len(tensors) != 7 * nb or nb < 2:
        raise ValueError('an edge MLP of nb >= 2 blocks comes as 4 nb parameters + 3 nb buffers (got nb = %d, %d tensors)'
                         % (nb, len(tensors)))
    if x.dim() != 2 or x.shape[0] != B * N:
        raise ValueError('x must be [B*N, C] rows (got %s for B = %d, N = %d)' % (tuple(x.shape), B, N))
    blocks = mlp_blocks(tensors, nb)
    Ws = [blk.W for blk in blocks]
    if Ws[0].shape[1] != 2 * x.shape[1]:
        raise ValueError('the first Linear takes %d features per edge, the points have %d' % (Ws[0].shape[1], x.shape[1]))
    on_menu = _edge_widths_on_menu([tuple(w.shape) for w in Ws], k)
    H, Fo = Ws[0].shape[0], Ws[-1].shape[0]
    E = B * N * k
    if route == 'fused' and not on_menu:
        raise ValueError("route='fused' needs k <= 64, widths <= 256, a hidden width that is a multiple of 4 and at most 3 equally wide hidden "
                         "Linears; use 'auto' or 'layers'")
    if route == 'auto':
        route = _edge_predict_auto(H, Fo, E) if on_menu else 'layers'
    _dev_check(x)
    with torch.no_grad():
        x = x.detach()
        if route == 'layers':
            return EdgeConvFn.apply(x, B, N, k, False, eps, 0.1, nb, aggr, None, order, *tensors)
        dev = x.device
        BN, C = x.shape
        idx, jg, order_out = knn(x, B, N, k, want_global=True, order=order, want_order=True)
        wpq_p, _, bpq = edge_first_operands(Ws[0], blocks[0].b)
        PQ = torch.empty(BN, 2 * H, device=dev, dtype=F32)
        linear_raw(_rows2d(x), wpq_p, bpq, BN, 2 * H, C, _rows2d(PQ))
        # the folded packs of the remaining Linears (the layout of gpe_stitch_pairs_fwd's, include/gpe_hip.h): W^T diag(s) of the
        # BatchNorm in front, then b + W t; f16x3: their two-term fp16 planes, one power of two per layer (its amax word)
        nh = nb - 2
        ldh, ldf = _stitch_ldw(H), _stitch_ldw(Fo)
        h3 = _edge_predict_h3(H, Fo, E)
        KP = round_up(H, 32)
        wpk = torch.zeros(nh * (H + 1) * ldh + (H + 1) * ldf, device=dev, dtype=F32)
        planes = torch.empty(nh * KP * ldh + KP * ldf, device=dev, dtype=F32) if h3 else None
        words = torch.empty(nh + 1, device=dev, dtype=torch.int32) if h3 else None
        st = bn_stats(blocks[0], eps)
        for l in range(1, nb):
            W, b = Ws[l], blocks[l].b
            ld, n_out = (ldh, H) if l < nb - 1 else (ldf, Fo)
            o = (l - 1) * (H + 1) * ldh
            L.call('gpe_stitch_pairs_pack', W, W.stride(0), n_out, H, st[2], wpk[o:], ld)
            L.call('gpe_fold_bias', W, W.stride(0), n_out, H, b, st[3], wpk[o + H * ld:])
            if h3:
                L.call('gpe_absmax', wpk[o:], ld, H, ld, words[l - 1:])
                L.call('gpe_stitch_pairs_planes', wpk[o:], H, ld, words[l - 1:], planes[(l - 1) * KP * ldh:])
            st = bn_stats(blocks[l], eps)
        ldF = round_up(Fo, 4)
        out = torch.empty(BN, ldF, device=dev, dtype=F32)[:, :Fo]
        L.call('gpe_edge_predict_fwd', PQ, 2 * H, jg, BN, k, H, Fo, nh, wpk, planes, words, st, _AGGR_CODE[aggr], out, ldF)
        return out, idx, order_out


# -------------------------------------------------------------------------------------------------
# graph pooling (DynamicASAPool)
# -------------------------------------------------------------------------------------------------
ASAP_K = 10                        # nn/net_blocks.py:204: DynamicASAPool builds its graph with k = 10 whatever it is given
ASAP_F_MAX, ASAP_N_MAX = 512, 8192


def asap_count(N, ratio):
    """Nodes PyG's topk keeps per cloud: ceil(float(ratio) * N) evaluated in fp32, as PyG does on a float32 fitness (0.3 x 50 -> 16,
    not 15); a ratio >= 1 is a count (at most N)."""
    if not ratio > 0:
        raise ValueError('pool ratio must be positive, got %r' % (ratio,))
    if ratio >= 1:
        return min(int(ratio), N)
    return int(math.ceil(np.float32(ratio) * np.float32(N)))


def asap_state_words(B, N, F, k):
    """include/gpe_hip.h gpe_asap_fwd: the 4-byte words of the state the forward leaves for the backward."""
    return 1024 + B * N * (2 * F + k + 8)


def asap_bwd_ws_bytes(B, N, F, k):
    """include/gpe_hip.h gpe_asap_bwd: the backward's workspace."""
    nblk = min((B * N + 15) // 16, 1024)
    return 8 * (nblk + 1) * (5 * F + 3) + 4 * B * N * (F + k + 4)


class AsapPoolFn(torch.autograd.Function):
    """DynamicASAPool (nn/net_blocks.py:194-218): PyG ASAPooling on knn(x, x, 10) per cloud -> (out [B*M, F], perm, rank, idx).
    x: [B*N, F] rows of B clouds of N points; params: lin.weight, lin.bias, att.weight, att.bias, gnn_score.lin1.weight,
    lin1.bias, lin2.weight, lin3.weight, lin3.bias.  perm int32 [B*M]: the kept GLOBAL rows, per cloud in descending fitness;
    rank int32 [B*N]: output row of a kept node, -1 otherwise; idx int32 [B, N, min(10, N)]: the kNN graph.  M is computed on the
    host from (N, ratio): nothing here reads the device, so the op can be captured (graph.StepGraph).  order: a locality order of
    the points (the preceding EdgeConv layer's last_order), a speed hint of the graph search.  save=False (no_grad): nothing is
    kept for a backward."""

    @staticmethod
    def forward(ctx, x, B, N, ratio, order, save, trace, *params):
        _dev_check(x)
        F = x.shape[1]
        if not (1 <= F <= ASAP_F_MAX and 1 <= N <= ASAP_N_MAX) or x.shape[0] != B * N:
            raise ValueError('ASAP pooling takes 1 <= F <= %d features and 1 <= N <= %d points per cloud (got x %s for B=%d, '
                             'N=%d)' % (ASAP_F_MAX, ASAP_N_MAX, tuple(x.shape), B, N))
        k = min(ASAP_K, N)
        M = asap_count(N, ratio)
        xc = x if x.stride(1) == 1 else x.contiguous()
        idx = knn(xc, B, N, k, order=order)
        rev_off, rev_edge = knn_reverse(idx)
        dev = x.device
        state = torch.empty(asap_state_words(B, N, F, k), device=dev, dtype=F32)
        out = torch.empty(B * M, F, device=dev, dtype=F32)
        perm = torch.empty(B * M, device=dev, dtype=torch.int32)
        rank = torch.empty(B * N, device=dev, dtype=torch.int32)
        L.call('gpe_asap_fwd', xc, xc.stride(0), B, N, F, k, rev_off, rev_edge, *params, M, out, perm, rank, state)
        ctx.mark_non_differentiable(perm, rank, idx)
        ctx.dims = (B, N, F, k)
        if trace is not None:                              # copies, not views: the trace must not keep the whole state alive
            BN = B * N
            trace['winners'] = state[1024 + BN * F:1024 + 2 * BN * F].view(torch.int32).view(BN, F).clone()
            trace['fitness'] = state[1024 + BN * (2 * F + k + 6):1024 + BN * (2 * F + k + 7)].clone()
        if save:
            ctx.save_for_backward(xc, idx, rev_off, rev_edge, rank, state, *params)
        return out, perm, rank, idx

    @staticmethod
    def backward(ctx, gout, *_):
        xc, idx, rev_off, rev_edge, rank, state, *params = ctx.saved_tensors
        B, N, F, k = ctx.dims
        dev = xc.device
        gout = gout.contiguous()
        dx = torch.empty(B * N, F, device=dev, dtype=F32)
        grads = [_gbuf(p) for p in params]
        nws = asap_bwd_ws_bytes(B, N, F, k)
        L.call('gpe_asap_bwd', gout, xc, xc.stride(0), B, N, F, k, idx, rev_off, rev_edge, *params, rank, state, dx, F, *grads,
               _workspace(nws, dev))
        return (dx, None, None, None, None, None, None) + tuple(_gret(p, g) for p, g in zip(params, grads))


def asap_pool(x, B, N, params, ratio, order=None, trace=None):
    """-> (out [B*M, F], M): DynamicASAPool's ASAPooling on x [B*N, F] (AsapPoolFn).  trace (a dict, optional) receives the kept
    rows 'perm', the output rows 'rank', the graph 'knn', the channel-max 'winners' and the 'fitness' of this call."""
    save = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
    out, perm, rank, idx = AsapPoolFn.apply(x, B, N, ratio, order, save, trace, *params)
    if trace is not None:
        trace.update(perm=perm, rank=rank, knn=idx)
    return out, asap_count(N, ratio)


# -------------------------------------------------------------------------------------------------
# recurrent stacks (LSTM / GRU)
# -------------------------------------------------------------------------------------------------
RNN_WS_HOOK = None         # measurement aid (scripts/rnn_trace.py): called with ('fwd' | 'bwd', workspace tensor) of every recurrence
RNN_PARAMS = ('w_ih', 'w_hh', 'b_ih', 'b_hh')                    # the tensors of one layer as autograd takes them: flat, layer by layer
RNNLayer = collections.namedtuple('RNNLayer', RNN_PARAMS)
NO_PLANES = (None, None, None, None)


def rnn_layers(params, n_layers):
    """the inverse of net_blocks._rnn_params: n_layers RNNLayer records"""
    P = len(RNN_PARAMS)
    assert len(params) == P * n_layers
    return [RNNLayer(*params[P * l: P * l + P]) for l in range(n_layers)]


def rnn_grads(n_layers, filed=None, d_x=None, d_h0=None, d_c0=None):
    """What RNNStackFn.backward returns: d_x, d_h0, d_c0, None up to the parameters, the gradients `filed` as {(layer, parameter field):
    tensor} at their places in _rnn_params' order"""
    out = [d_x, d_h0, d_c0] + [None] * (RNNStackFn.LEAD - 3 + len(RNN_PARAMS) * n_layers)
    for (l, field), g in (filed or {}).items():
        out[RNNStackFn.LEAD + len(RNN_PARAMS) * l + RNN_PARAMS.index(field)] = g
    return tuple(out)


def rnn_planes(layers, kind):
    """-> (hh planes, ih planes, hh amax words, ih amax words) per layer, entry 0 of the ih lists unused: the plan's fp16 plane packs of
    `kind` (K_GATES_H3, K_TRANS_H3) of every recurrent weight for the f16x3 arithmetic; NO_PLANES unless every one of them is there
    (the kernels then run the exact fp32 instruction)"""
    hh = [planned_planes(ly.w_hh, kind) for ly in layers]
    ih = [planned_planes(ly.w_ih, kind) for ly in layers[1:]]
    if any(t is None for pair in hh + ih for t in pair):
        return NO_PLANES
    return [p for p, _ in hh], [None] + [p for p, _ in ih], [a for _, a in hh], [None] + [a for _, a in ih]


def _strides(t, n):
    """the first n strides of t; zeros for a tensor that is not there"""
    return (0,) * n if t is None else tuple(t.stride()[:n])


def _ptr_arrays(lists):
    return [None if ts is None else _ptr_array(ts) for ts in lists]


# the two recurrence entry points by keyword (include/gpe_hip.h): each ends in its one L.call, arguments in the header's order.  dims =
# (L, T, Bn, H); per-layer operands are lists (the pointer arrays are built here and live until the launch is queued — the CALLER keeps
# the tensors themselves); strides are read off the tensors; cs: None for a GRU; planes: rnn_planes(..)
def rnn_seq_fwd(*, gates, dims, xproj, whh, wih, bias, bhn, hs, cs, saved, planes, ws):
    """xproj = (layer 0's input projection, its row stride, its step stride); wih[0], bias[0] unused; bhn: the GRU's b_hn slices or None;
    ws = (arrival counters of the persistent launch or None, bytes)"""
    L.call('gpe_rnn_seq_fwd', gates, *dims, *xproj, *_ptr_arrays((whh, wih, bias, bhn)), hs, *_strides(hs, 3), cs, *_strides(cs, 2),
           saved, *_strides(saved, 2), *_ptr_arrays(planes), *ws)


def rnn_seq_bwd(*, gates, dims, g_top, d_hN, d_cN, whh_t, wih_t, hs, cs, saved, dgx, dgh, part, carry, planes):
    """g_top [Bn, T, H] (unit stride inside a row), d_hN, d_cN: the gradients that arrived, or None; dgx, dgh: gate gradients out (one
    tensor for an LSTM), same strides"""
    assert dgh.stride() == dgx.stride()
    L.call('gpe_rnn_seq_bwd', gates, *dims, g_top, *_strides(g_top, 2), d_hN, d_cN, *_ptr_arrays((whh_t, wih_t)), hs, *_strides(hs, 3),
           cs, *_strides(cs, 2), saved, *_strides(saved, 2), dgx, dgh, *_strides(dgx, 3), part, carry, *_ptr_arrays(planes))


class RNNStackFn(torch.autograd.Function):
    """torch.nn.LSTM / torch.nn.GRU (batch_first, n_layers, no dropout) as used by the reference's decoders / encoder
    (nn/net_blocks.py:336-497): returns (top-layer outputs [Bn, T, H] as a view of the h history, h_T [L, Bn, H],
    c_T [L, Bn, H] or None).

    x is either [Bn, In] — the SAME input at every step (decoders feed the encoding T times, :388,430,483): layer 0's input
    projection is then computed once — or a sequence [Bn, T, In] (one GEMM over all steps).  The recurrence itself runs in
    WAVEFRONT order (csrc/gpe_rnn_wave.hip): all cells (layer l, step t) of an anti-diagonal l + t = d are independent, so a
    diagonal is one fused launch forward (gate GEMMs on h_{l,t-1} and h_{l-1,t} + cell update) and two launches backward
    (split-K dh products of all cells, pointwise cell backward): T + L - 1 dependent steps instead of T * L.  Weight
    gradients are reduce-GEMMs over all Bn*T rows afterwards.  Gate orders follow torch: LSTM i,f,g,o; GRU r,z,n.
    Start states may carry gradient (LSTMDoubleReverseDecoderModule threads the first LSTM's final state into the
    second), final states too."""
    LEAD = 8                   # forward's arguments in front of *params

    @staticmethod
    def forward(ctx, x, h0, c0, T, n_layers, kind, want_state, h0_ok, *params):
        _dev_check(x)
        streams.lane(x.device.index).run_jobs()            # (the chip is about to idle: the jobs EdgeConvFn.forward left on the lane)
        ctx.set_materialize_grads(False)
        dev = x.device
        lstm = kind == 'lstm'
        G = 4 if lstm else 3
        seq = x.dim() == 3
        Bn, In = x.shape[0], x.shape[-1]
        Hh = h0.shape[2]
        Hp = round_up(Hh, 4)
        Lr = n_layers
        # h history with a 16-B row pitch (zero pad): slot 0 = h0, slot t+1 = h_t
        hs = torch.zeros(Lr, Bn, T + 1, Hp, device=dev, dtype=F32)
        hs[:, :, 0, :Hh].copy_(h0)
        cs = None
        if lstm:
            cs = torch.empty(Lr, T + 1, Bn, Hh, device=dev, dtype=F32)
            cs[:, 0].copy_(c0)
        saved = torch.empty(Lr, T, Bn, 4 * Hh, device=dev, dtype=F32)
        layers = rnn_layers(params, Lr)
        # the operands of every layer — fused bias, gate packs (layer 0's input weight is a GEMM of its own, below), the GRU's b_hn —
        # stay referenced by these lists until the launch is queued
        whh, wih, biases = [], [], []
        for l, ly in enumerate(layers):
            biases.append(bias_sum(ly.b_ih, ly.b_hh) if lstm else gru_bias(ly.b_ih, ly.b_hh, Hh))
            whh.append(pack_gates(ly.w_hh, Hh, G))
            wih.append(pack_gates(ly.w_ih, Hh, G) if l > 0 else None)
        bhns = None if lstm else [ly.b_hh[2 * Hh:] for ly in layers]
        if seq:
            xproj = torch.empty(Bn, T, G * Hh, device=dev, dtype=F32)
            linear_raw(_rows3d(x), pack_weight(layers[0].w_ih), biases[0], Bn * T, G * Hh, In, (xproj, G * Hh, 0, 0))
            xp_sb, xp_st = T * G * Hh, G * Hh
        else:
            xproj = torch.empty(Bn, G * Hh, device=dev, dtype=F32)
            linear_raw(_rows2d(x), pack_weight(layers[0].w_ih), biases[0], Bn, G * Hh, In, _rows2d(xproj))
            xp_sb, xp_st = G * Hh, 0
        # f16x3 arithmetic: the plan's fp16 plane packs + amax words of every recurrent weight (absent -> exact fp32 kernels)
        # (h0_ok: the fp16-pipe kernels scale the state rows by GPE_STATE_SA = 2^12 (csrc/gpe_device.h) before the fp16 split — a start
        # state of magnitude >= 16 would overflow to inf; rnn_stack decides)
        planes = rnn_planes(layers, K_GATES_H3) if h0_ok else NO_PLANES
        ws_n = L.query('gpe_rnn_seq_fwd_ws', G, Lr, T, Bn, Hh)    # arrival counters of the persistent launch (0: diagonal launches)
        ws = torch.empty(ws_n, device=dev, dtype=torch.uint8) if ws_n > 0 else None
        if RNN_WS_HOOK is not None:
            RNN_WS_HOOK('fwd', ws)
        rnn_seq_fwd(gates=G, dims=(Lr, T, Bn, Hh), xproj=(xproj, xp_sb, xp_st), whh=whh, wih=wih, bias=[None] + biases[1:], bhn=bhns,
                    hs=hs, cs=cs, saved=saved, planes=planes, ws=(ws, max(ws_n, 0)))
        hN = cN = None
        if want_state:
            hN = hs[:, :, T, :Hh].contiguous()
            cN = cs[:, T].contiguous() if lstm else None
        ctx.dims = (Bn, In, Hh, T, Lr, kind, seq)
        ctx.save_for_backward(x, hs, cs, saved, *params)
        ctx.needs_state_grad = (h0.requires_grad, c0 is not None and c0.requires_grad)
        top = hs[Lr - 1, :, 1:, :Hh]
        if lstm:
            return top, hN, cN
        return top, hN

    @staticmethod
    def backward(ctx, g_top, g_hN, g_cN=None):
        Bn, In, Hh, T, Lr, kind, seq = ctx.dims
        lstm = kind == 'lstm'
        G = 4 if lstm else 3
        sv = ctx.saved_tensors
        x, hs, cs, saved = sv[:4]
        params = sv[4:]
        layers = rnn_layers(params, Lr)
        dev = x.device
        want_h0, want_c0 = ctx.needs_state_grad
        GH = G * Hh
        GHp = round_up(GH, 4)
        dgx = torch.empty(Lr, Bn, T, GHp, device=dev, dtype=F32)
        dgh = dgx if lstm else torch.empty(Lr, Bn, T, GHp, device=dev, dtype=F32)
        part = torch.empty(L.query('gpe_rnn_seq_bwd_ws', G, Lr, T, Bn, Hh), device=dev, dtype=F32)
        if RNN_WS_HOOK is not None:
            RNN_WS_HOOK('bwd', part)
        carry = torch.empty(2, Lr, Bn, Hh, device=dev, dtype=F32)
        whh_t = [pack_weight(ly.w_hh, transpose=True) for ly in layers]
        wih_t = [None] + [pack_weight(ly.w_ih, transpose=True) for ly in layers[1:]]
        if g_top is not None and g_top.stride(2) != 1:
            g_top = g_top.contiguous()
        ghN = g_hN.contiguous() if g_hN is not None else None
        gcN = g_cN.contiguous() if (lstm and g_cN is not None) else None
        # f16x3: transposed fp16 plane packs + amax words for the persistent backward launch (absent -> exact fp32 there)
        rnn_seq_bwd(gates=G, dims=(Lr, T, Bn, Hh), g_top=g_top, d_hN=ghN, d_cN=gcN, whh_t=whh_t, wih_t=wih_t, hs=hs, cs=cs, saved=saved,
                    dgx=dgx, dgh=dgh, part=part, carry=carry, planes=rnn_planes(layers, K_TRANS_H3) if lstm else NO_PLANES)
        filed = {}
        d_x = None
        d_h0 = torch.empty(Lr, Bn, Hh, device=dev, dtype=F32) if want_h0 else None
        d_c0 = carry[0].clone() if want_c0 else None
        nz = (GH + 255) // 256
        # ---- what the rest of the backward pass waits for: the input gradient and the start-state gradients ----
        dGs = None
        gx0 = _rows3d(dgx[0][:, :, :GH])
        if not seq:
            # the same input row feeds every step: sum the gate gradients over T first, then ONE Bn-row product
            # (T times fewer rows than dG^T x over the repeated input)
            dGs = torch.empty(Bn, GH, device=dev, dtype=F32)
            L.call('gpe_reduce_inner', dgx[0], T * GHp, GHp, T, Bn, GH, dGs, GH, 0)
            if ctx.needs_input_grad[0]:
                d_x = torch.empty(Bn, In, device=dev, dtype=F32)
                linear_raw(_rows2d(dGs), pack_weight(layers[0].w_ih, transpose=True), None, Bn, In, GH, _rows2d(d_x))
        elif ctx.needs_input_grad[0]:
            d_x = torch.empty(Bn, T, In, device=dev, dtype=F32)
            linear_raw(gx0, pack_weight(layers[0].w_ih, transpose=True), None, Bn * T, In, GH, (d_x, In, 0, 0))
        if want_h0:
            for l in range(Lr):
                # dh_0 = dG_{l,0} . W_hh (+ the z-gated direct path of a GRU)
                rec = torch.empty(nz, Bn, Hh, device=dev, dtype=F32)
                L.call('gpe_linear_splitk', dgh[l][:, 0], T * GHp, whh_t[l], rec, Bn, Hh, GH)
                L.call('gpe_reduce_inner', rec, Hh, Bn * Hh, nz, Bn, Hh, d_h0[l], Hh, 0)
                if not lstm:
                    L.call('gpe_add', d_h0[l], carry[0][l], d_h0[l], Bn * Hh)
        # ---- the weight gradients: leaves of the backward pass (on the side stream when every one of them lands in the arena) ----
        with side_grads(list(params), [dgx, dgh, hs, x, dGs]):
            for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(layers):
                gx_rows, gh_rows = _rows3d(dgx[l][:, :, :GH]), _rows3d(dgh[l][:, :, :GH])
                d_whh, d_bhh = _gbuf(w_hh), _gbuf(b_hh)
                redgemm_raw(gh_rows, _rows3d(hs[l][:, :T, :Hh]), Bn * T, GH, Hh, out=(d_whh, d_bhh))
                d_wih, d_bih = _gbuf(w_ih), _gbuf(b_ih)
                if l == 0 and not seq:
                    redgemm_raw(_rows2d(dGs), _rows2d(x), Bn, GH, In, out=(d_wih, d_bih))
                else:
                    Kin = In if l == 0 else Hh
                    src = _rows3d(x) if l == 0 else _rows3d(hs[l - 1][:, 1:, :Hh])
                    redgemm_raw(gx_rows, src, Bn * T, GH, Kin, out=(d_wih, d_bih))
                filed[l, 'w_ih'], filed[l, 'w_hh'] = _gret(w_ih, d_wih), _gret(w_hh, d_whh)
                filed[l, 'b_ih'], filed[l, 'b_hh'] = _gret(b_ih, d_bih), _gret(b_hh, d_bhh)
        return rnn_grads(Lr, filed, d_x, d_h0, d_c0)


class DropoutMulFn(torch.autograd.Function):
    """y = x * mask on a (strided) [Bn, T, H] sequence: the dropout torch's recurrent modules apply between layers."""

    @staticmethod
    def forward(ctx, x, mask):
        _dev_check(x)
        assert x.dim() == 3 and x.stride(2) == 1 and mask.is_contiguous() and mask.shape == x.shape
        Bn, T, H = x.shape
        out = torch.empty(Bn, T, H, device=x.device, dtype=F32)
        L.call('gpe_mul_rows', x, x.stride(0), x.stride(1), mask, Bn, T, H, out)
        ctx.save_for_backward(mask)
        return out

    @staticmethod
    def backward(ctx, g):
        mask, = ctx.saved_tensors
        if g.stride(2) != 1:
            g = g.contiguous()
        Bn, T, H = mask.shape
        gx = torch.empty(Bn, T, H, device=g.device, dtype=F32)
        L.call('gpe_mul_rows', g, g.stride(0), g.stride(1), mask, Bn, T, H, gx)
        return gx, None


def _dropout_mask(T, Bn, H, p, device):
    """The mask at::dropout draws for a recurrent layer's output: torch's nn.LSTM / nn.GRU work time-major, so the noise tensor
    is [T, Bn, H] (ATen RNN.cpp apply_layer_stack -> dropout -> empty_like(input).bernoulli_(1 - p).div_(1 - p)).  Drawn on the
    CPU generator in that shape — the stream the reference's CPU run consumes, like the random start states — and handed over
    batch-major."""
    if HOST_DRAWN is not None:
        def fill(pin):
            pin.copy_(torch.empty(T, Bn, H).bernoulli_(1 - p).div_(1 - p).transpose(0, 1))
        return HOST_DRAWN.get((Bn, T, H), fill)
    noise = torch.empty(T, Bn, H).bernoulli_(1 - p).div_(1 - p)
    return noise.transpose(0, 1).contiguous().to(device, non_blocking=True)


def rnn_stack(x, h0, c0, T, n_layers, kind, params, want_state=False, dropout=0.0, training=False, h0_bounded=False):
    """nn.LSTM / nn.GRU(batch_first=True, num_layers, dropout).  Without dropout (or in eval mode, or with one layer) the whole
    stack runs in wavefront order (RNNStackFn).  With dropout the layers run one after the other — the mask sits between them —
    each as a one-layer RNNStackFn over the masked output sequence of the layer below.

    f16x3 arithmetic (gpe_amd.set_math): the forward gate products run on the fp16 pipe with the state rows scaled by 2^12, which
    is exact for every state a cell produces (|h| < 1) and for start states below 16.  h0_bounded=True promises |h0| < 16 (the
    package's own modules: the reference's zero / kaiming start states, nn/net_blocks.py:308-315, and chained decoder states);
    otherwise the largest |h0| is READ BACK here (one host synchronisation per call, f16x3 mode only) and a start state of
    magnitude >= 16 takes the exact fp32 kernels for the whole sequence."""
    h0_ok = True
    if not h0_bounded and L.get_math() == 'f16x3' and h0 is not None:
        h0_ok = bool(h0.abs().max().item() < 16.0)
    if not (dropout > 0 and training and n_layers > 1):
        out = RNNStackFn.apply(x, h0, c0, T, n_layers, kind, want_state, h0_ok, *params)
        return out if kind == 'lstm' else (out[0], out[1], None)
    lstm = kind == 'lstm'
    layers = rnn_layers(params, n_layers)
    inp, hs, cs = x, [], []
    for l in range(n_layers):
        out = RNNStackFn.apply(inp, h0[l:l + 1], c0[l:l + 1] if lstm else None, T, 1, kind, want_state, h0_ok, *layers[l])
        top = out[0]
        if want_state:
            hs.append(out[1])
            if lstm:
                cs.append(out[2])
        if l < n_layers - 1:
            inp = DropoutMulFn.apply(top, _dropout_mask(T, top.shape[0], top.shape[2], float(dropout), top.device))
    hN = torch.cat(hs, 0) if want_state else None
    cN = torch.cat(cs, 0) if (want_state and lstm) else None
    return top, hN, cN


# -------------------------------------------------------------------------------------------------
# dense MLP (attention variant, MLP decoder, stitch model)
# -------------------------------------------------------------------------------------------------
class DenseMLPFn(torch.autograd.Function):
    """MLP(channels) = [Linear -> ReLU -> BatchNorm1d] x n on dense rows (nn/net_blocks.py:43-47 as used by
    point_segment_mlp, nn/nets.py:223-226; MLPDecoder, nn/net_blocks.py:273-298; StitchOnEdge3DPairs, nn/nets.py:342).
    Same kernels as the edge MLP with one "message" per row (k = 1): fused Linear+ReLU(+fp64 BN statistics), every
    BatchNorm folded into the next Linear, the last one applied explicitly; backward = the edge MLP's chain (centred
    reduce-GEMM -> BN coefficients -> propagate in place).  Layers wider than 256 (the global-attention MLP is 403 wide,
    an MLP decoder thousands) run as K slabs / several column blocks of the generic row GEMM."""
    LEAD = 5                                               # forward's arguments in front of *tensors (x .. n_blocks)

    @staticmethod
    def forward(ctx, x, training, eps, momentum, n_blocks, *tensors):
        _dev_check(x)
        dev = x.device
        M = x.shape[0]
        nblk = L.query('gpe_stats_blocks')
        acts, stats = [], []
        a_in, Cin = x, x.shape[1]
        scale = tvec = None
        ews = edge_workspace(1, M, 1, 4, dev)
        words = f16x3_words(2 * n_blocks, M, dev)          # [l] activation a_l, [n + l] dz_l (backward)
        for l, blk in enumerate(mlp_blocks(tensors, n_blocks)):
            W, b = blk.W, blk.b
            Cout = W.shape[0]
            ldo = round_up(Cout, 4)
            a = torch.empty(M, ldo, device=dev, dtype=F32)
            part = torch.empty(nblk, 2, Cout, device=dev, dtype=torch.float64) if training else None
            edge_mlp_fwd(src=edge_rows(a_in), dims=(1, M, 1), Cin=Cin, Cout=Cout, wp=pack_weight(W, col_scale=scale),
                         bias=b if tvec is None else fold_bias(W, b, tvec), out=a, ldo=ldo, stats_part=part, agg=None, ldagg=0,
                         amax_a=_word(words, l - 1) if l > 0 else None, amax_out=_word(words, l) if l < n_blocks - 1 else None,
                         ws=ews, out_half=0)
            st = bn_stats(blk, eps, training, momentum, part, nblk, M)
            acts.append(a)
            stats.append(st)
            scale, tvec = st[2], st[3]
            a_in, Cin = a, Cout
        y = torch.empty(M, Cin, device=dev, dtype=F32)
        L.call('gpe_bn_apply', a_in, a_in.stride(0), stats[-1], M, Cin, y, Cin)
        ctx.n_blocks = n_blocks
        ctx.training = training
        ctx.done = False
        ctx.words = words
        save_groups(ctx, x=x, params=tensors[:len(MLP_PARAMS) * n_blocks], acts=acts, stats=stats)
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.done:
            raise RuntimeError('DenseMLPFn.backward ran twice on the same graph: the stored activations are overwritten '
                               'in place by the first pass (retain_graph is not supported)')
        ctx.done = True
        n, training = ctx.n_blocks, ctx.training
        sv = saved_groups(ctx)
        x, acts, stats = sv['x'], sv['acts'], sv['stats']
        blocks = mlp_blocks(sv['params'], n)
        dev = x.device
        M = x.shape[0]
        gy = gy.contiguous()
        filed = {}                         # (block, parameter field) -> gradient
        # last block: BN applied explicitly -> same algebra as the edge layer's BN-after-max with one slot per row
        a, st = acts[-1], stats[-1]
        C = blocks[-1].W.shape[0]
        g_l, be_l = blocks[-1].gamma, blocks[-1].beta
        psb = L.query('gpe_point_sums_blocks')
        part = torch.empty(psb, 2, C, device=dev, dtype=torch.float64)
        L.call('gpe_edge_bwd_point_sums', gy, C, a, a, a.stride(0), st, M, C, part, None)
        coef, dgam, dbet = bn_bwd_coef(part, psb, st, C, M, g_l, be_l, training)
        words = ctx.words
        ews = edge_workspace(1, M, 1, 4, dev)
        L.call('gpe_edge_dz3_all', a, a.stride(0), gy, C, 1.0, coef, 1, M, 1, C, _word(words, 2 * n - 1))
        filed[n - 1, 'gamma'], filed[n - 1, 'beta'] = _gret(g_l, dgam), _gret(be_l, dbet)
        dz = a                                     # holds dz_{n-1} now
        for l in range(n - 1, 0, -1):
            Cl, Cp = blocks[l].W.shape[0], blocks[l - 1].W.shape[0]
            # (an input wider than the edge reduce-GEMM takes: the row reduce-GEMM, no partials)
            ws = None if Cp > 256 else torch.empty(L.query('gpe_redgemm_ws', Cl, Cp), device=dev, dtype=F32)
            dz = _block_bwd(filed, blocks, l, dz, edge_rows(acts[l - 1]), stats[l - 1], (1, M, 1), M, training,
                            (_word(words, n + l), _word(words, l - 1), _word(words, n + l - 1)), ews, ws)
        W0, b0 = blocks[0].W, blocks[0].b
        H0, K0 = W0.shape[0], x.shape[1]
        dW, db = _gbuf(W0), _gbuf(b0)
        redgemm_raw((dz, dz.stride(0), 0, 0), _rows2d(x), M, H0, K0, out=(dW, db))
        filed[0, 'W'], filed[0, 'b'] = _gret(W0, dW), _gret(b0, db)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty(M, K0, device=dev, dtype=F32)
            linear_raw((dz, dz.stride(0), 0, 0), pack_weight(W0, transpose=True), None, M, K0, H0, _rows2d(gx))
        return mlp_grads(DenseMLPFn.LEAD, n, filed, gx)


def dense_mlp(x, mlp, training):
    """mlp: the nn.Sequential parameter container built by net_blocks.MLP."""
    x = x if x.stride(1) == 1 else x.contiguous()
    eps, momentum, n, tensors = mlp_tensors(mlp)
    return DenseMLPFn.apply(x, training, eps, momentum, n, *tensors)


# -------------------------------------------------------------------------------------------------
# attention over the points: sparsemax weights and the pooling they drive (nn/nets.py:225-276)
# -------------------------------------------------------------------------------------------------
class SparsemaxFn(torch.autograd.Function):
    """sparsemax.Sparsemax(dim=1) (nn/nets.py:225)."""

    @staticmethod
    def forward(ctx, z):
        _dev_check(z)
        z = z.contiguous()
        M, W = z.shape
        out = torch.empty_like(z)
        L.call('gpe_sparsemax_fwd', z, W, M, W, out, W)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        out, = ctx.saved_tensors
        g = g.contiguous()
        M, W = out.shape
        gz = torch.empty_like(out)
        L.call('gpe_sparsemax_bwd', out, W, g, W, M, W, gz, W)
        return gz


class AttentionPoolFn(torch.autograd.Function):
    """pooled[b, p, :] = pool_n w[b, n, p] * feat[b, n, :]  — the reference's 23-iteration loop of
    `w[:, p] * features -> global_pool` (nn/nets.py:263-276) as one batched launch for all clouds and panels.
    mode: 0 mean (shipped), 1 max, 2 add — the encoder's `global_pool` setting."""

    @staticmethod
    def forward(ctx, w, feat, B, N, mode=0):
        _dev_check(w)
        dev = w.device
        P, C = w.shape[1], feat.shape[1]
        pooled = torch.empty(B, P, C, device=dev, dtype=F32)
        nws = L.query('gpe_attn_pool_ws', B, N, P, C)
        part = torch.empty(nws, device=dev, dtype=F32)
        arg = torch.empty(B, P, C, device=dev, dtype=torch.int32) if mode == 1 else None
        part_arg = torch.empty(nws, device=dev, dtype=torch.int32) if mode == 1 else None
        L.call('gpe_attn_pool_fwd', w, w.stride(0), feat, feat.stride(0), B, N, P, C, mode, pooled, arg, part, part_arg)
        ctx.dims = (B, N, P, C, mode)
        ctx.arg = arg
        ctx.save_for_backward(w, feat)
        return pooled.view(B * P, C)

    @staticmethod
    def backward(ctx, g):
        w, feat = ctx.saved_tensors
        B, N, P, C, mode = ctx.dims
        dev = w.device
        g = g.contiguous()
        gw = torch.empty(B * N, P, device=dev, dtype=F32)
        gf = torch.empty(B * N, C, device=dev, dtype=F32)
        L.call('gpe_attn_pool_bwd', w, w.stride(0), feat, feat.stride(0), g, ctx.arg, B, N, P, C, mode, gw, P, gf, C)
        return gw, gf, None, None, None


# -------------------------------------------------------------------------------------------------
# PointNet++ set abstraction (PointNetPlusPlus, nn/net_blocks.py:10-88)
# -------------------------------------------------------------------------------------------------
def fps_start(B, N, device):
    """PyG's fps(random_start=True) (what nn/net_blocks.py:16 calls): the start point of every cloud, drawn as
    `(torch.rand(B) * N).long()` on torch's default CPU generator — the stream the reference's CPU run consumes, like the
    random LSTM states — ONE draw per fps call (oracle/ref_path.py fps_start)."""
    start = (torch.rand(B) * float(N)).long().clamp_(max=N - 1)
    return start.to(torch.int32).to(device, non_blocking=True)


def fps(pos, B, N, M, start=None):
    """torch_geometric.nn.fps over equal-sized clouds: -> int32 [B, M] LOCAL indices in selection order, starting at
    start[b] (int32 [B] on the device; None = the cloud's first point, i.e. random_start=False); ties -> lower index."""
    _dev_check(pos)
    idx = torch.empty(B, M, device=pos.device, dtype=torch.int32)
    L.call('gpe_fps', pos, pos.stride(0), B, N, pos.shape[1], M, start, idx)
    return idx


def radius_neighbors(pos, cidx, B, N, r, max_num_neighbors):
    """torch_geometric.nn.radius(pos, pos[idx], r, ..., max_num_neighbors): -> (nbr int32 [B*M, maxn] local point indices,
    first maxn in ascending order, cnt int32 [B*M])."""
    _dev_check(pos)
    M = cidx.shape[1]
    nbr = torch.empty(B * M, max_num_neighbors, device=pos.device, dtype=torch.int32)
    cnt = torch.empty(B * M, device=pos.device, dtype=torch.int32)
    L.call('gpe_radius', pos, pos.stride(0), cidx, B, N, pos.shape[1], M, float(r), max_num_neighbors, nbr, cnt)
    return nbr, cnt


def pointconv_self_loops(nbr, cnt, B, N, M):
    """PyG PointNetConv's default add_self_loops=True on the ball-query edge list: -> (edge count per centroid after the
    re-indexing, slot of the removed neighbour or -1).  See csrc/gpe_pointnet.hip."""
    cnt2 = torch.empty_like(cnt)
    drop = torch.empty_like(cnt)
    L.call('gpe_pointconv_self_loops', nbr, cnt, B, N, M, nbr.shape[1], cnt2, drop)
    return cnt2, drop


def ball_messages(pos, x, cidx, nbr, off, n_edges, B, N, drop=None):
    """PointConv message inputs [E, Cx + 3] over the compact edge list + the centroid (segment) id of every edge row.
    drop: from pointconv_self_loops (then `off` is the scan of ITS counts)."""
    M, maxn = cidx.shape[1], nbr.shape[1]
    C = pos.shape[1]
    Cx = 0 if x is None else x.shape[1]
    msg = torch.empty(n_edges, Cx + C, device=pos.device, dtype=F32)
    seg = torch.empty(n_edges, device=pos.device, dtype=torch.int32)
    L.call('gpe_ball_messages', pos, pos.stride(0), x, 0 if x is None else x.stride(0), Cx, cidx, nbr, off, drop, B, N, C, M,
           maxn, msg, Cx + C, seg)
    return msg, seg


class RaggedMaxFn(torch.autograd.Function):
    """max over each centroid's (ragged) run of edge rows: PointConv's aggr='max'."""

    @staticmethod
    def forward(ctx, x, off, seg, S):
        _dev_check(x)
        E, C = x.shape
        y = torch.empty(S, C, device=x.device, dtype=F32)
        arg = torch.empty(S, C, device=x.device, dtype=torch.int64)
        L.call('gpe_ragged_max_fwd', x, x.stride(0), off, S, C, y, C, arg)
        ctx.save_for_backward(off, arg, seg)
        ctx.dims = (E, C)
        return y

    @staticmethod
    def backward(ctx, gy):
        off, arg, seg = ctx.saved_tensors
        E, C = ctx.dims
        gy = gy.contiguous()
        gx = torch.empty(E, C, device=gy.device, dtype=F32)
        L.call('gpe_ragged_max_bwd', gy, C, off, arg, seg, E, C, gx, C)
        return gx, None, None, None


# -------------------------------------------------------------------------------------------------
# The leaf modules, re-exported: callers keep spelling ops.X
# -------------------------------------------------------------------------------------------------
# ops_stitch imports names of this module, so these lines close a cycle.  It is safe only because they come last and because the
# package's __init__ imports ops before any leaf: whichever leaf is asked for first, __init__ runs first, and this module is complete
# when ops_stitch starts.  Keep both orders.  Each leaf's __all__ makes the star exact; nothing here is lazy.
from .ops_stitch import *  # noqa: E402,F401,F403
from .ops_losses import *  # noqa: E402,F401,F403
from .ops_data import *  # noqa: E402,F401,F403
from .ops_scan import *  # noqa: E402,F401,F403
from .ops_eval import *  # noqa: E402,F401,F403

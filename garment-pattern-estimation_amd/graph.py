"""A training step captured ONCE as a hipGraph and replayed (host-bound shapes: the reference's shipped training shape — BASELINE
cfg 1, N = 1024, batch 8, k = 5 — is ~200 launches of 3 - 30 us each; the Python side of a launch costs more than the kernel).

    sg = StepGraph(lambda feats, gt: model.loss(model(feats), gt)[0], optimizer)      # optimizer: optim.FusedAdam
    for feats, gt in loader:
        loss = sg.step(feats, gt)          # the first `warmup` calls run eagerly; then one capture; then replays

forward_loss may also return (loss, loss_dict, ...): what follows the loss is kept as `sg.extras`, so the metrics of a replayed step can
be logged (the stitch classifier: lambda f, g: model.loss(model(f), g)[:2], then sg.extras[0]['stitch_recall']).

What a replay cannot carry in frozen kernel arguments is fed through device memory in front of the graph launch:
  * the reference draws the LSTM start states (and dropout masks) on the CPU generator inside forward() (nn/net_blocks.py:391-392):
    every such tensor has a static device buffer; before each replay the host draws them IN THE SAME ORDER from the same generator
    into pinned memory and queues the copies (HostDrawn below; net_blocks._init_tenzor and ops._dropout_mask go through it);
  * Adam's step-dependent scalars (OneCycle learning rate, bias corrections) live in a two-float device buffer per arena run
    (include/gpe_hip.h gpe_adam_step_dev);
  * the inputs are copied into static buffers.
The fp16-activation guard (ops.set_half_act_guard) keeps working in its default 'fallback' mode: the amax words of the captured forward
are read asynchronously after every replay; a layer that trips it invalidates the graph, and the next step is captured again on the
fp32 path.  'strict' (a host read inside the forward) cannot be captured and raises.
FusedAdam's guarded step (max_grad_norm / skip_nonfinite / guard_overflow / param_grad_norms) is captured like the plain one: the norm,
the clip factor and the skip flag live in device memory and the Adam launch reads them there; optimizer.grad_norm, .skipped, ... are static
tensors that every replay overwrites, like `loss`.

The rule for control flow: which launches a step makes must be a function of the tensor SHAPES, of the non-tensor arguments of
step() and of `key` — nothing else.  Non-tensor arguments (an epoch, a flag; leaves of nested dicts / lists / tuples too) are handed to
forward_loss as given, at every call; `key` is an optional callable, evaluated at every step, for whatever forward_loss reads from
outside its arguments (a closure over the trainer's epoch).  When any of these values differs from the previous step's, the graph is
dropped, that step runs eagerly (lazily built state of the new branch — workspaces, pack plans — must exist before a capture), and the
next step is captured again:

    sg = StepGraph(lambda f, g, epoch: model.loss(model(f), g, epoch=epoch)[0], optimizer)
    loss = sg.step(feats, gt, epoch)                                  # re-captured whenever `epoch` changes
    sg = StepGraph(lambda f, g: model.loss(model(f), g, epoch=trainer.epoch)[0], optimizer,
                   key=lambda: trainer.epoch >= model.loss.config['epoch_with_stitches'])      # re-captured when the loss changes

A forward_loss that reads anything else (an outer variable that no argument and no `key` reflects) gets, in every replay, the
value it had at the capture: a replay runs no Python.  invalidate() drops the graph by hand.

One process per GPU, world size 1: a gradient exchange inside the captured region is not supported (RCCL launches are not captured
here).  The captured step is single-stream; the tensors a replay returns are static buffers, overwritten by the next replay."""
import ctypes

import torch

from . import _lib as L
from . import ops
from . import streams


class HostDrawn:
    """Host-drawn device tensors of a step (start states, dropout masks), drawn in call order from the CPU generator."""

    def __init__(self, device):
        self.device = device
        self.entries = []            # streams.Staged: .dst the device tensor, .fill what draws it
        self.cursor = 0
        self.capturing = False

    def begin_step(self):
        """Draw every registered tensor (registration order = call order = the reference's draw order) and queue its copy."""
        self.cursor = 0
        for e in self.entries:
            e.refill()

    def get(self, shape, fill_fn):
        shape = tuple(shape)
        i = self.cursor
        self.cursor += 1
        if i == len(self.entries):
            if self.capturing:
                raise RuntimeError('StepGraph: the captured step draws a host tensor the warm-up steps did not draw (shape %s): the '
                                   'step must issue the same sequence of launches every time' % (shape,))
            self.entries.append(streams.Staged(shape, self.device, fill_fn))
            self.entries[i].refill()
        dst = self.entries[i].dst
        if tuple(dst.shape) != shape:
            raise RuntimeError('StepGraph: host-drawn tensor %d changed shape (%s -> %s)' % (i, tuple(dst.shape), shape))
        return dst


class StepGraph:
    def __init__(self, forward_loss, optimizer, warmup=2, device=None, key=None):
        """forward_loss(*inputs) -> scalar loss tensor (forward + loss; backward and optimizer.step() are run here), or a tuple /
        list whose first element is that loss: what follows it (tensors, or nested dicts / lists / tuples of tensors — a loss dict)
        is kept, detached, as the tuple `self.extras`: the step's own values during the warm-up, from the capture on the static
        tensors that every replay overwrites (None for a plain tensor return).  step() returns the loss either way.
        Non-tensor inputs reach forward_loss as the current call gave them; a change of one drops the graph (module docstring).
        optimizer: optim.FusedAdam.  warmup: eager steps before the capture (>= 1: lazily built state — pack plans, workspaces,
        kernel attributes — must exist before a capture).  key: optional callable without arguments, evaluated at every step; its
        value is compared like a non-tensor input (it names the branch of the step that forward_loss takes for reasons its
        arguments do not show)."""
        if not (hasattr(optimizer, 'step_captured') and hasattr(optimizer, 'advance_captured')):
            raise TypeError('StepGraph needs an optimizer whose step-dependent scalars live in device memory (optim.FusedAdam); a '
                            'torch optimizer bakes them into its kernels\' arguments')
        self.forward_loss = forward_loss
        self.opt = optimizer
        self.warmup = max(int(warmup), 1)
        self.key = key
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.host = HostDrawn(self.device)
        self.calls = 0
        self.graph = None
        self.static_in = None
        self.leaves = None           # the non-tensor leaves of the last step's inputs, in order, and the value of `key`
        self.eager_left = self.warmup
        self.loss = None
        self.extras = None
        self.guards = []             # (HalfActGuard, amax word) pairs met during the capture
        self.hyper = []              # per arena run: streams.Staged of Adam's two step-dependent floats
        self.runs = None
        self.replays = 0
        self.captures = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise RuntimeError('StepGraph captures a single-process step (world size 1)')

    # ---- inputs: tensors, or (nested) dicts / lists / tuples of tensors ----
    def _flat(self, obj, out):
        if isinstance(obj, torch.Tensor):
            out.append(obj)
        elif isinstance(obj, dict):
            for k in obj:
                self._flat(obj[k], out)
        elif isinstance(obj, (list, tuple)):
            for v in obj:
                self._flat(v, out)
        return out

    def _like(self, obj):
        if isinstance(obj, torch.Tensor):
            return torch.empty_like(obj, device=self.device)
        if isinstance(obj, dict):
            return {k: self._like(v) for k, v in obj.items()}
        if isinstance(obj, (list, tuple)):
            return type(obj)(self._like(v) for v in obj)
        return obj

    def _leaves(self, obj, out):
        """the non-tensor leaves of `obj`, in the order _flat walks it"""
        if isinstance(obj, torch.Tensor):
            pass
        elif isinstance(obj, dict):
            for k in obj:
                self._leaves(obj[k], out)
        elif isinstance(obj, (list, tuple)):
            for v in obj:
                self._leaves(v, out)
        else:
            out.append(obj)
        return out

    def _merge(self, static, obj):
        """the structure of `obj` with the static tensors in place of its tensors: non-tensor leaves are those of THIS call"""
        if isinstance(obj, torch.Tensor):
            if not isinstance(static, torch.Tensor):
                raise self._changed()
            return static
        if isinstance(obj, dict):
            if not isinstance(static, dict) or list(static) != list(obj):
                raise self._changed()
            return {k: self._merge(static[k], v) for k, v in obj.items()}
        if isinstance(obj, (list, tuple)):
            if type(static) is not type(obj) or len(static) != len(obj):
                raise self._changed()
            return type(obj)(self._merge(s, v) for s, v in zip(static, obj))
        if isinstance(static, (torch.Tensor, dict, list, tuple)):
            raise self._changed()
        return obj

    @staticmethod
    def _changed():
        return RuntimeError('StepGraph: the inputs changed shape or type; a captured step is one fixed shape')

    @staticmethod
    def _same(a, b):
        try:
            return type(a) is type(b) and bool(a == b)
        except Exception:                    # (a leaf whose == has no truth value: compare by identity)
            return a is b

    def _stage(self, inputs):
        if self.static_in is None:
            self.static_in = self._like(inputs)
        dst, src = self._flat(self.static_in, []), self._flat(inputs, [])
        if len(dst) != len(src) or any(d.shape != s.shape or d.dtype != s.dtype for d, s in zip(dst, src)):
            raise self._changed()
        self.static_in = self._merge(self.static_in, inputs)
        leaves = self._leaves(inputs, [])
        if self.key is not None:
            leaves.append(self.key())
        was = self.leaves
        if was is not None and (len(was) != len(leaves) or not all(self._same(a, b) for a, b in zip(was, leaves))):
            self.invalidate()
            self.eager_left = max(self.eager_left, 1)      # the new branch builds its lazy state before a capture
        self.leaves = leaves
        for d, s in zip(dst, src):
            if d.data_ptr() != s.data_ptr():
                d.copy_(s, non_blocking=True)

    def invalidate(self):
        """Drop the captured graph: the next step past the warm-up captures again.  The static input buffers, the host-drawn
        tensors and the step counters stay."""
        self.graph = None

    def _detached(self, obj):
        if isinstance(obj, torch.Tensor):
            return obj.detach()
        if isinstance(obj, dict):
            return {k: self._detached(v) for k, v in obj.items()}
        if isinstance(obj, (list, tuple)):
            return type(obj)(self._detached(v) for v in obj)
        return obj

    def _forward(self):
        """-> the loss of forward_loss; what it returned behind the loss becomes self.extras"""
        r = self.forward_loss(*self.static_in)
        if isinstance(r, (tuple, list)):
            if not r:
                raise ValueError('StepGraph: forward_loss returned an empty %s (the first element is the loss)' % type(r).__name__)
            self.extras = self._detached(tuple(r[1:]))
            return r[0]
        self.extras = None
        return r

    def _eager(self):
        loss = self._forward()
        loss.backward()
        self.opt.step()
        return loss

    def _capture(self):
        if ops._HALF_ACT_GUARD == 'strict':
            raise RuntimeError("StepGraph: the 'strict' half-activation guard reads the device inside the forward and cannot be captured")
        self.guards = []
        self.hyper_slot(7)                 # pinned memory cannot be allocated inside a capture: eight runs are plenty
        self.graph = torch.cuda.CUDAGraph()
        self.host.capturing = True
        ops.CAPTURE = self
        try:
            with torch.cuda.graph(self.graph, stream=self.stream):
                loss = self._forward()
                loss.backward()
                self.runs = self.opt.step_captured(self)
        finally:
            ops.CAPTURE = None
            self.host.capturing = False
        self.loss = loss.detach()
        self.captures += 1

    def step(self, *inputs):
        """One training step on `inputs`; returns the loss (a static device tensor from the first replay on).  The caller's
        stream is made to wait for the step, so the returned tensor can be used there right away."""
        outer = torch.cuda.current_stream(self.device)
        try:
            return self._step(inputs)
        finally:
            if outer != self.stream:
                outer.wait_stream(self.stream)

    def _step(self, inputs):
        outer = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.stream):
            if outer != self.stream:
                self.stream.wait_stream(outer)       # the inputs were produced there
            self._stage(inputs)
            ops.HOST_DRAWN = self.host
            try:
                self.host.begin_step()
                self.calls += 1
                if self.eager_left > 0:
                    self.eager_left -= 1
                    return self._eager()
                if self.graph is None:
                    self._capture()
                    self.host.cursor = 0
                self.opt.advance_captured(self, self.runs)
                self.graph.replay()
                self.replays += 1
                tripped = False
                for guard, word in self.guards:
                    was = guard.disabled
                    guard._watch(word)           # (the poll only: the word went on the optimizer's record during the capture)
                    guard.allow()
                    tripped = tripped or (guard.disabled and not was)
                if tripped:
                    self.graph = None            # the next step is captured again, on the fp32 rows of the layer that tripped
                return self.loss
            finally:
                ops.HOST_DRAWN = None

    def synchronize(self):
        self.stream.synchronize()

    # ---- Adam's step-dependent scalars ----
    def hyper_slot(self, i):
        if i >= len(self.hyper) and ops.CAPTURE is not None:
            raise RuntimeError('StepGraph: more optimizer runs than pre-allocated scalar slots')
        while len(self.hyper) <= i:
            self.hyper.append(streams.Staged(2, self.device))
        return self.hyper[i]

    def write_hyper(self, i, lr, beta1, beta2, step):
        slot = self.hyper_slot(i)
        rc = L.lib().gpe_adam_hyper(float(lr), float(beta1), float(beta2), int(step), ctypes.c_void_p(slot.next().data_ptr()))
        if rc != 0:
            raise RuntimeError('gpe_adam_hyper failed with code %d' % rc)
        slot.push()

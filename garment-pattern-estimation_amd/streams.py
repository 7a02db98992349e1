"""What the package does beside the caller's stream: the ONE side stream per device that work is forked onto and joined back from
(`lane`), and host data on its way to the device through pinned memory (`Staged`, `Uploader`).  Mechanism only: what
runs on a lane and when (size gates, debug switches) is decided in ops.py.  One host thread drives a lane at a time."""
import contextlib

import torch


def stream_key(device):
    """(device ordinal, handle of its current stream): the key of per-stream caller-owned state (workspaces, tickets)."""
    idx = torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    return idx, torch.cuda.current_stream(idx).cuda_stream


class Lane:
    def __init__(self, index):
        self.index = index
        self.stream = None           # created by the first fork: building a lane touches no device
        self.dirty = False           # the side stream holds launches the main stream has not waited for
        self.queued = False          # join() is queued as a final callback of the running backward pass
        self.jobs = []               # idle-stretch jobs {'fn', 'src', 'out', 'event'} waiting for run_jobs(); owners may drop theirs

    @contextlib.contextmanager
    def fork(self, tensors=(), leaf=False):
        """The body runs on the side stream, behind everything the device's current stream has queued.  `tensors`: main-stream
        memory it reads (kept from the allocator until the side stream has passed it).  leaf=False: the caller joins inline: wait()."""
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.index)
        self.stream.wait_stream(torch.cuda.current_stream(self.index))
        for t in tensors:
            if t is not None:
                t.record_stream(self.stream)
        if leaf:
            # nothing in the running backward pass reads the results: joined when the pass ends, by a final autograd callback bound
            # to THIS lane, and again by whoever consumes the results (join() costs nothing on a clean lane)
            self.dirty = True
            if not self.queued:
                self.queued = True
                torch.autograd.Variable._execution_engine.queue_callback(self.join)
        with torch.cuda.stream(self.stream):
            yield True

    def wait(self, made=(), event=None):
        """The inline join of a fork(): the current stream waits for `event` of the side stream, or for all of it, and goes on to
        use the tensors `made` inside the fork.  The flags stay: an event is not a full join."""
        main = torch.cuda.current_stream(self.index)
        if event is not None:
            main.wait_event(event)
        else:
            main.wait_stream(self.stream)
        for t in made:
            t.record_stream(main)

    def join(self):
        """This device's current stream waits for everything pending on the side stream.  On the side stream itself (a collective
        issued inside a leaf fork) there is nothing to wait for, and the lane stays dirty for the main stream."""
        self.queued = False
        if self.dirty and torch.cuda.current_stream(self.index) != self.stream:
            self.dirty = False
            torch.cuda.current_stream(self.index).wait_stream(self.stream)

    def run_jobs(self):
        """The caller knows the chip is about to idle: launch the waiting jobs (joined like leaf work, but from a forward pass:
        no callback).  Nothing forks inside a stream capture: the jobs are dropped and their owners do the work themselves."""
        jobs, self.jobs = self.jobs, []
        if not jobs or torch.cuda.is_current_stream_capturing():
            return
        with self.fork([j['src'] for j in jobs]):
            self.dirty = True
            for j in jobs:
                j['out'] = j['fn'](j['src'])
                j['event'] = self.stream.record_event()


_LANES = {}


def lane(index):
    """The side lane of a device ordinal: callers pass the device of the tensors they fork for, never "the current device"."""
    return _LANES.get(index) or _LANES.setdefault(index, Lane(index))


class Staged:
    """A fixed device tensor `dst` fed through two pinned buffers: while the copy out of one may be in flight, the host fills the
    other.  `fill(pinned)` (optional) draws the host values: refill().  Pinned memory cannot be allocated inside a stream capture."""

    def __init__(self, shape, device, fill=None):
        self.dst = torch.zeros(shape, device=device)
        self.fill = fill
        self.pins = [torch.zeros(shape, pin_memory=True) for _ in range(2)]
        self.events = [torch.cuda.Event() for _ in range(2)]
        self.flip = 0

    def next(self):
        """-> the pinned buffer to write now (the copy that last read it, two pushes ago, has run)."""
        self.flip ^= 1
        self.events[self.flip].synchronize()
        return self.pins[self.flip]

    def push(self):
        """Queue the copy of the buffer next() gave out on the current stream."""
        self.dst.copy_(self.pins[self.flip], non_blocking=True)
        self.events[self.flip].record()

    def refill(self):
        self.fill(self.next())
        self.push()


class Uploader:
    """Host data -> a FRESH fp32 device tensor through pinned slots and a copy stream of its own: the compute stream is not drained,
    it only waits for the copy's event.  Which slot a call uses (`key`) is the owner's policy."""

    def __init__(self, device):
        self.device = device
        self.stream = torch.cuda.Stream(device=device)
        self.slots = {}              # key -> (pinned buffer, event of the last copy out of it)

    def upload(self, key, shape, fill):
        slot = self.slots.get(key)
        if slot is None or slot[0].shape != shape:
            slot = self.slots[key] = (torch.empty(shape, dtype=torch.float32, pin_memory=True), torch.cuda.Event())
        buf, ev = slot
        ev.synchronize()             # the previous copy out of this buffer has finished
        fill(buf)
        compute = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.stream):
            out = torch.empty(shape, device=self.device, dtype=torch.float32)      # owned by the copy stream's pool
            out.copy_(buf, non_blocking=True)
            ev.record(self.stream)
        compute.wait_event(ev)
        out.record_stream(compute)
        return out

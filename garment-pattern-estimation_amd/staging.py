"""Input side of a training step (reference: nn/trainer.py:93 `features = batch['features'].to(device)` from pageable
memory, after nn/data/transforms.py:35-50 standardised every sample on the CPU).

BatchStager keeps two pinned host buffers and a copy stream per device: batch i+1 is copied while step i computes, the
compute stream only waits on the copy's event, and the per-axis standardisation `(x - shift) / scale` runs as one kernel
on the device instead of per sample on the host."""
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

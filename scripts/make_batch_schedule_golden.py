#!/usr/bin/env python3
"""Generates tests/golden/batch_schedule_small.pt: how the REFERENCE'S OWN BalancedBatchSampler (nn/data/utils.py:16-92, imported
and run unmodified) distributes the garments of a small split over the batches of an epoch.

Only runnable where the reference checkout exists (like scripts/make_stitch_sample_golden.py, whose sys.path set-up on the read-only
stubs it shares).  Split: four garment types of 7, 5, 1 and 11 garments (ids 0 .. 23 in type order), drop_last=True, at batch sizes
5 (four batches, four garments dropped, quotas 1, 1, 0, 2: the exhausted-class path is taken) and 4 (six batches, quotas 1, 0, 0,
1).  random.seed(0) once, then N = 2000 epochs per setting.  The fixture holds COUNTS ONLY, per setting
(tests/batch_schedule_restate.py Counts):
  comp      int64 [n, 6]: batch number, the garments of every type in it, the epochs that batch had this composition
  batch_of  int64 [4, rows + 1]: for the first garment of every type, the epochs it landed in batch t (last column: dropped)
  slot_of   int64 [4, B]: ... and the slot it took inside its batch

    python scripts/make_batch_schedule_golden.py [REFERENCE_DIR]
"""
import contextlib
import io
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('GPE_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(REPO, 'oracle', 'refgen', 'stubs'), os.path.join(REF, 'nn'), REPO, os.path.join(REPO, 'tests')]

from data.utils import BalancedBatchSampler  # noqa: E402  (the reference's class)
import batch_schedule_restate as R  # noqa: E402

GOLDEN = os.path.join(REPO, 'tests', 'golden')
SIZES, BATCH_SIZES, EPOCHS = [7, 5, 1, 11], [5, 4], 2000


def main():
    off = np.concatenate([[0], np.cumsum(SIZES)])
    ids_by_type = {'type%d' % c: torch.arange(int(off[c]), int(off[c + 1])) for c in range(len(SIZES))}
    class_of = {g: c for c in range(len(SIZES)) for g in range(int(off[c]), int(off[c + 1]))}
    watched = [int(off[c]) for c in range(len(SIZES))]
    random.seed(0)
    out = {'sizes': SIZES, 'watched': watched, 'epochs': EPOCHS, 'settings': {}}
    for B in BATCH_SIZES:
        with contextlib.redirect_stdout(io.StringIO()):
            sampler = BalancedBatchSampler(ids_by_type, batch_size=B, drop_last=True)       # ---- the reference, unmodified ----
        quotas = [sampler.batch_len_per_type[k] for k in sampler.class_names]
        assert quotas == R.quotas(SIZES, B), (quotas, R.quotas(SIZES, B))
        counts = R.Counts(len(SIZES), B, len(sampler))
        for _ in range(EPOCHS):
            batches = list(iter(sampler))
            assert len(batches) == len(sampler) and all(len(b) == B for b in batches)
            flat = [g for b in batches for g in b]
            assert len(set(flat)) == len(flat)
            counts.add(batches, class_of, watched)
        broken = sum(v for k, v in counts.comp.items() if any(n < q for n, q in zip(k[1:], quotas)))
        print('B = %d: quotas %s, %d batches per epoch, %d distinct (batch, composition) cells, %d of %d batches below a quota'
              % (B, quotas, len(sampler), len(counts.comp), broken, EPOCHS * len(sampler)))
        out['settings'][B] = {'N': counts.N, 'C': counts.C, 'B': B, 'rows': counts.rows, 'quotas': quotas,
                              'comp': torch.from_numpy(counts.comp_rows()), 'batch_of': torch.from_numpy(counts.batch_of),
                              'slot_of': torch.from_numpy(counts.slot_of)}
    path = os.path.join(GOLDEN, 'batch_schedule_small.pt')
    torch.save(out, path)
    print('batch_schedule_small: %.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()

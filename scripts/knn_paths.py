"""Measurement aid (GPU): which graph-search kernel runs for which call (csrc/gpe_knn_plan.h).
One gpe_knn per case — every row of the ladder, the reservation cases of tests/test_gpu_grid_sizes.py at 0 / 100 / 192 reserved CUs
(the scan's wide / narrow choice), a search with and without an order hint, calls without a workspace.  idx, idx_glob and order_out
of every case are saved to --out as .npy and gpe_knn_ws_bytes of the case is printed.  The GPE_KNN_* switches are taken from the
environment of the process (GPE_DEBUG=1 arms them; they are read once, so every setting is a run of its own).  Run it under
`rocprofv3 --kernel-trace` (nothing else traced) once per library (GPE_HIP_LIB selects another build) and compare the ordered kernel
lists (name with template arguments, grid, workgroup, dynamic LDS), the printed lines and the saved arrays of the two runs.

  python scripts/knn_paths.py --out DIR"""
import argparse, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpe_amd as gpe
from gpe_amd import _lib as Lb

# (B, N, C, ld, k, options).  Options: order = 'reverse' passes an order hint, ws = 'none' / 'short' calls without a workspace / with
# one a byte short of the query, reserve = CUs held back
CASES = [
    (2, 300, 3, 3, 8, {}),                                   # 1a sorted cloud
    (2, 300, 3, 4, 8, {}),                                   #    padded rows
    (2, 300, 3, 3, 8, {'ws': 'none'}),                       # 1b an xyz cloud that cannot be sorted
    (2, 64, 3, 3, 4, {}), (2, 9000, 3, 3, 4, {}),            # 1b xyz clouds off the sorted search's sizes; the C <= 4 instance
    (2, 70, 7, 7, 64, {}), (3, 200, 8, 8, 5, {}), (3, 200, 6, 6, 5, {}), (3, 200, 6, 7, 5, {}),     # 1b staging 1 / 4 / 2 / 1 floats
    (1, 200, 40, 40, 49, {}), (2, 513, 256, 256, 64, {}),    # 1b wide rows, k > 48
    (8, 2048, 8, 256, 16, {}),                               # 1b pinned, four pieces by the L2 rule (a 2 MB table per cloud)
    (2, 130, 24, 24, 5, {'ws': 'none'}), (2, 130, 24, 24, 5, {'ws': 'short'}),                        # 2a, and a byte short
    (2, 300, 150, 152, 16, {}), (2, 130, 64, 64, 32, {}), (9, 200, 33, 36, 5, {}),                    # 2b threshold scan
    (3, 97, 32, 32, 33, {}), (2, 130, 33, 36, 40, {}), (1, 200, 150, 152, 48, {}), (1, 200, 160, 160, 33, {}),   # 2c <2> <2> <5> <5>
    (1, 200, 161, 164, 16, {}), (1, 700, 200, 200, 16, {}), (2, 300, 256, 256, 48, {}),               # 2c <8>
    (1, 300, 300, 300, 8, {}), (2, 130, 300, 301, 8, {}), (2, 130, 299, 302, 8, {}),                  # 2d staging 4 / 1 / 2 floats
    (3, 700, 150, 152, 16, {}), (3, 700, 150, 152, 16, {'order': 'reverse'}),                         # order hint: scan
    (2, 300, 200, 200, 16, {}), (2, 300, 200, 200, 16, {'order': 'reverse'}),                         #             list kernel
]
for R in (0, 100, 192):                                      # tests/test_gpu_grid_sizes.py KNN_GRID_CASES
    CASES += [(8, 2048, 150, 150, 16, {'reserve': R}), (12, 1000, 150, 150, 16, {'reserve': R}), (16, 2048, 150, 150, 16, {'reserve': R}),
              (12, 2048, 3, 3, 16, {'reserve': R})]

ap = argparse.ArgumentParser()
ap.add_argument('--out', required=True)
args = ap.parse_args()
os.makedirs(args.out, exist_ok=True)
print('switches: %s' % ' '.join('%s=%s' % kv for kv in sorted(os.environ.items()) if kv[0].startswith('GPE_KNN_') or kv[0] == 'GPE_DEBUG'))

for ci, (B, N, C, ld, k, opt) in enumerate(CASES):
    g = torch.Generator().manual_seed(1000 + ci)
    buf = torch.zeros(B * N, ld)
    buf[:, :C] = torch.randn(B * N, C, generator=g)
    x = buf.cuda()[:, :C]
    idx = torch.full((B, N, k), -7, device='cuda', dtype=torch.int32)
    jg = torch.full((B, N, k), -7, device='cuda', dtype=torch.int32)
    oo = torch.full((B, N), -7, device='cuda', dtype=torch.int32)
    order = None
    if opt.get('order') == 'reverse':
        order = torch.arange(N - 1, -1, -1, dtype=torch.int32).expand(B, N).contiguous().cuda()
    query = Lb.query('gpe_knn_ws_bytes', B, N, C, k)
    nws = {'none': 0, 'short': query - 1}.get(opt.get('ws'), query)
    ws = torch.empty(nws, device='cuda', dtype=torch.uint8) if nws else None
    Lb.query('gpe_reserve_cus_set', opt.get('reserve', 0))
    Lb.call('gpe_knn', x, B, N, C, x.stride(0), k, idx, jg, order, oo, ws, nws)
    torch.cuda.synchronize()
    Lb.query('gpe_reserve_cus_set', 0)
    for n, t in (('idx', idx), ('idx_glob', jg), ('order_out', oo)):
        np.save(os.path.join(args.out, 'case%02d_%s.npy' % (ci, n)), t.cpu().numpy())
    print('case %2d %s %s: ws %d bytes, idx sum %d, order sum %d' % (ci, (B, N, C, ld, k), opt, query, int(idx.long().sum()), int(oo.long().sum())),
          flush=True)

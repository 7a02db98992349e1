"""Measurement aid (GPU): which recurrence kernel runs for which stack (csrc/gpe_rnn_seq.hip).
One forward + backward of ops.rnn_stack per case and arithmetic mode; every output, final state and gradient is saved to --out as
.npy, and the two workspace queries of the case are printed.  Run it under `rocprofv3 --kernel-trace` (nothing else traced) once
per library (GPE_HIP_LIB selects another build) and compare the ordered kernel lists (name with template arguments, grid,
workgroup), the memset sizes, the printed lines and the saved tensors of the two runs.

  python scripts/rnn_paths.py --out DIR"""
import argparse, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpe_amd as gpe
from gpe_amd import ops, net_blocks
from gpe_amd import _lib as Lb

PANEL, PATTERN = (736, 250, 250, 14, 3), (32, 250, 250, 23, 2)
# (kind, (Bn, In, H, T, L), options): every outcome of the ladder.  Options: seq = a sequence input, modes, plan = False drops the
# PackPlan's packs (f16x3 mode without planes: the exact kernels), reserve = CUs held back, dbg = gpe_debug_set bits
CASES = [('lstm', PATTERN, {}), ('lstm', (5, 20, 20, 3, 1), {}),                    # persistent, both directions
         ('lstm', PANEL, {}),                                                       # f16x3: multi-tile forward, diagonal backward
         ('lstm', (900, 40, 96, 5, 2), {'seq': True}), ('gru', (70, 250, 250, 9, 2), {}),
         # diagonals in several groups, clipped diagonals, two K slabs (tests/test_gpu_kernels.py)
         ('lstm', (5, 12, 20, 5, 5), {}), ('gru', (5, 12, 20, 5, 5), {}), ('lstm', (17, 12, 20, 7, 6), {}), ('gru', (17, 12, 20, 7, 6), {}),
         ('lstm', (5, 12, 20, 3, 5), {}), ('gru', (5, 12, 20, 3, 5), {}), ('lstm', (20, 24, 260, 3, 2), {}),
         ('lstm', PATTERN, {'modes': ['f16x3'], 'plan': False}), ('lstm', PANEL, {'modes': ['f16x3'], 'plan': False}),
         ('lstm', PANEL, {'modes': ['f16x3'], 'reserve': 16}), ('lstm', PANEL, {'modes': ['f16x3'], 'reserve': 192}),
         ('lstm', PATTERN, {'dbg': 1024}), ('lstm', PANEL, {'dbg': 2048 | 4096}), ('lstm', PANEL, {'dbg': 65536}),
         ('lstm', PANEL, {'dbg': 131072})]

ap = argparse.ArgumentParser()
ap.add_argument('--out', required=True)
args = ap.parse_args()
os.makedirs(args.out, exist_ok=True)

for ci, (kind, (Bn, In, Hh, T, L), opt) in enumerate(CASES):
    G = 4 if kind == 'lstm' else 3
    torch.manual_seed(ci)
    rnn = (torch.nn.LSTM if kind == 'lstm' else torch.nn.GRU)(In, Hh, L, batch_first=True).cuda()
    g = torch.Generator().manual_seed(100 + ci)
    x = (torch.randn(Bn, T, In, generator=g) if opt.get('seq') else torch.randn(Bn, In, generator=g)).cuda()
    h0 = (torch.randn(L, Bn, Hh, generator=g) * 0.3).cuda()
    c0 = (torch.randn(L, Bn, Hh, generator=g) * 0.3).cuda() if kind == 'lstm' else None
    wgt = torch.randn(Bn, T, Hh, generator=g).cuda()
    params = net_blocks._rnn_params(rnn, L)
    plan = ops.PackPlan()
    net_blocks._register_rnn_packs(plan, rnn, L, Hh, G)
    for mode in opt.get('modes', ['f32', 'f16x3']):
        gpe.set_math(mode)
        plan.refresh()
        if not opt.get('plan', True):
            ops.bump_weights_epoch()
        Lb.query('gpe_reserve_cus_set', opt.get('reserve', 0))
        Lb.query('gpe_debug_set', opt.get('dbg', 0))
        ws = (Lb.query('gpe_rnn_seq_fwd_ws', G, L, T, Bn, Hh), Lb.query('gpe_rnn_seq_bwd_ws', G, L, T, Bn, Hh))
        for p in rnn.parameters():
            p.grad = None
        xd = x.clone().requires_grad_()
        top, hN, cN = ops.rnn_stack(xd, h0, c0, T, L, kind, params, want_state=True, h0_bounded=True)
        loss = (top * wgt).sum() + hN.sum() * 0.5
        (loss + cN.sum() * 0.25 if cN is not None else loss).backward()
        torch.cuda.synchronize()
        Lb.query('gpe_debug_set', 0)
        Lb.query('gpe_reserve_cus_set', 0)
        tensors = {'top': top, 'hN': hN, 'dx': xd.grad}
        if cN is not None:
            tensors['cN'] = cN
        tensors.update({'d_' + n: p.grad for n, p in rnn.named_parameters()})
        for n, t in tensors.items():
            np.save(os.path.join(args.out, '%s_case%02d_%s.npy' % (mode, ci, n)), t.detach().cpu().numpy())
        print('%-5s case %2d %s %s %s: fwd_ws %d bytes, bwd_ws %d floats, %d tensors' %
              (mode, ci, kind, (Bn, In, Hh, T, L), opt, ws[0], ws[1], len(tensors)), flush=True)

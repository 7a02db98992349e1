"""Measurement aid (GPU): which fused edge GEMM kernel runs for which launch (csrc/gpe_edge_dispatch.hip).
One DynamicEdgeConv forward + backward per case and arithmetic mode; every output and gradient is saved to --out as .npy.
Run it under `rocprofv3 --kernel-trace` (nothing else traced) once per library (GPE_HIP_LIB selects another build) and compare
the ordered kernel lists (name with template arguments, grid, LDS bytes) and the saved tensors of the two runs.

  python scripts/edge_paths.py --out DIR [--modes f32,bf16x3,mixed,bf16x6,f16x3] [--gate 0|default]"""
import argparse, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpe_amd as gpe

# (B, N, C, H, Fo, k): k = 16 (the second: ragged last tile), 5, generic, pseudo-points (20, 32), no pseudo-split (17: producer/
# consumer), off the menu (rg_dispatch_nt), and the one large enough for the lazy-dz3 / fp16-row instances at the default gate
CASES = [(2, 128, 3, 200, 150, 16), (1, 256, 150, 200, 150, 16), (3, 43, 3, 200, 150, 16), (2, 100, 3, 200, 150, 5),
         (1, 77, 150, 200, 150, 8), (1, 90, 150, 200, 150, 20), (2, 64, 150, 200, 150, 20), (1, 70, 3, 200, 150, 32),
         (1, 64, 150, 200, 150, 17), (2, 96, 24, 32, 24, 5), (2, 2048, 150, 200, 150, 16)]

ap = argparse.ArgumentParser()
ap.add_argument('--out', required=True)
ap.add_argument('--modes', default='f32,bf16x3,mixed,bf16x6,f16x3')
ap.add_argument('--gate', default='0', help="rows below which f16x3 is not used: a number, or 'default'")
args = ap.parse_args()
os.makedirs(args.out, exist_ok=True)
if args.gate != 'default':
    gpe.set_f16x3_min_rows(int(args.gate))

for mode in args.modes.split(','):
    gpe.set_math(mode)
    for ci, (B, N, C, H, Fo, k) in enumerate(CASES):
        torch.manual_seed(ci)
        conv = gpe.net_blocks.DynamicEdgeConv(gpe.net_blocks.MLP([2 * C, H, H, Fo]), k=k)
        with torch.no_grad():
            for blk in conv.nn:
                blk[2].weight.uniform_(0.5, 1.5)
                blk[2].bias.uniform_(-0.3, 0.3)
            conv.nn[2][2].weight[::5] *= -1              # a negative BatchNorm scale: the min-tracking path
        conv = conv.cuda().train()
        g = torch.Generator().manual_seed(100 + ci)
        x = torch.randn(B * N, C, generator=g).cuda().requires_grad_()
        wgt = torch.randn(B * N, Fo, generator=g).cuda()
        y = conv(x, B, N)
        (y * wgt).sum().backward()
        torch.cuda.synchronize()
        tensors = {'y': y, 'dx': x.grad}
        tensors.update({'d_' + n: p.grad for n, p in conv.named_parameters()})
        tensors.update({'b_' + n: b for n, b in conv.named_buffers()})
        for n, t in tensors.items():
            np.save(os.path.join(args.out, '%s_case%02d_%s.npy' % (mode, ci, n)), t.detach().cpu().numpy())
        print('%-6s case %2d %s: %d tensors' % (mode, ci, (B, N, C, H, Fo, k), len(tensors)), flush=True)

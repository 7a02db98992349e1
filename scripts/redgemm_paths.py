"""Measurement aid (GPU): which reduce-GEMM kernel runs for which call (csrc/gpe_redgemm_plan.h).
One call per case — every rung of the ladder and its neighbours, in the math modes f32, bf16x3 and f16x3 (f16x3_min_rows = 0), the
f16x3 dense cases also with gpe_debug_set(16384) (off the bf16-pipe TN kernel), the reservation-sensitive cases at 0 / 100 / 192
reserved CUs, and one EdgeConv layer forward + backward whose weight gradient takes the lazy kernels.  G and colsum (the layer:
its parameter gradients) of every case are saved to --out as .npy; gpe_redgemm_ws and the return code are printed per case.  The
GPE_RD_* switches are taken from the environment of the process (GPE_DEBUG=1 arms them; they are read once, so every setting is a
run of its own).  Run it under `rocprofv3 --kernel-trace` (nothing else traced) once per library (GPE_HIP_LIB selects another build)
and compare the ordered kernel lists (name with template arguments, grid, workgroup), the printed lines and the saved arrays of the
two runs.  The trace does not show dynamic LDS sizes.

  python scripts/redgemm_paths.py --out DIR"""
import argparse, os, re, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpe_amd as gpe
from gpe_amd import _lib as Lb
ops = gpe.ops

# dense calls through gpe_redgemm: (rows, Mg, Ng, options).  Options: upitch / vpitch = row pitch in floats (default: the width), T =
# two-level rows [rows / T][T] (V with one spare slot per sequence), shift, nocs = no column sum, acc = accumulate_into, reserve = CUs
# held back, modes = math modes to run in (default all three)
RAW = [
    (4099, 37, 2, {'upitch': 40, 'shift': 1}), (4096, 300, 4, {}), (4096, 1000, 4, {}), (4096, 300, 4, {'nocs': 1}),   # thin <1> <2> <4>
    (4095, 400, 3, {}), (4096, 1025, 4, {}), (4102, 400, 3, {'T': 7}),                                                 # just off thin
    (736, 1000, 250, {'T': 23, 'vpitch': 252}), (20000, 77, 130, {'upitch': 80, 'vpitch': 132, 'shift': 1}),           # TN (f16x3)
    (65536, 150, 200, {'upitch': 152}),                                                                               # the edge shape without words
    (31, 250, 150, {'upitch': 252, 'vpitch': 152}), (1000, 40, 250, {'vpitch': 252}),                                  # the TN menu refuses
    (10304, 1000, 250, {'T': 14, 'vpitch': 252}), (77, 8, 250, {}), (1000, 152, 201, {}),                              # deep <true> <true> <false>
    (300, 23, 153, {}), (5000, 1000, 250, {'vpitch': 252}),                                                           # big-block (bf16x3: deep is closed)
    (131072 + 9, 8, 250, {'reserve': 192, 'vpitch': 252}),                                                            # 64 gx tiles + 1 at 64 usable CUs
    (1000, 150, 200, {'upitch': 152, 'acc': 1}),                                                                      # accumulate
]
# edge calls through gpe_edge_redgemm: (B, N, k, Mg, Ng, options).  gather = V is relu(P_i + Q_j); words = 'both' / 'u' (f16x3: amax_v
# = NULL) ; ws = 0: no edge workspace; lazy = the lazy fields set (a refusal below the producer/consumer threshold)
EDGE = [
    (1, 255 * 8, 16, 200, 200, {'gather': 1}),                     # big-block, gathered: one tile short of 4 gx
    (2, 1000, 1, 200, 200, {'gather': 1}),                         # gathered with k = 1: never producer/consumer
    (8, 256, 16, 150, 200, {}), (8, 256, 16, 200, 200, {}),        # 1024 tiles = 4 gx: pc / b3, dense
    (8, 256, 16, 150, 200, {'gather': 1}), (8, 256, 16, 200, 200, {'gather': 1}),     # gathered, clouds pinned
    (5, 410, 16, 200, 200, {'gather': 1}),                         # gathered, unpinned
    (8, 256, 16, 200, 200, {'gather': 1, 'words': 'u', 'modes': ('f16x3',)}),         # the bound passes run in the call
    (8, 256, 16, 200, 200, {'gather': 1, 'words': 'u', 'ws': 0, 'modes': ('f16x3',)}),   # no workspace: exact fp32
    (2, 64, 16, 150, 200, {'lazy': 1, 'modes': ('f16x3',)}),       # a direct lazy call below the threshold: -22
]
for R in (0, 100, 192):                                            # tests/test_gpu_grid_sizes.py: path, gx and partials follow the usable CUs
    RAW += [(10304, 1000, 250, {'T': 14, 'vpitch': 252, 'reserve': R}), (20000, 200, 7, {'reserve': R}), (65536, 400, 152, {'reserve': R})]
    EDGE += [(8, 256, 16, 200, 200, {'reserve': R}), (8, 256, 16, 200, 200, {'gather': 1, 'reserve': R})]

ap = argparse.ArgumentParser()
ap.add_argument('--out', required=True)
args = ap.parse_args()
os.makedirs(args.out, exist_ok=True)
print('switches: %s' % ' '.join('%s=%s' % kv for kv in sorted(os.environ.items()) if kv[0].startswith('GPE_RD_') or kv[0] == 'GPE_DEBUG'))
gpe.set_f16x3_min_rows(0)


def save(tag, **arrays):
    for n, t in arrays.items():
        if t is not None:
            np.save(os.path.join(args.out, '%s_%s.npy' % (tag, n)), t.detach().cpu().numpy())


def rows_of(rows, cols, pitch, T, gen, spare):
    """-> (descriptor, the [rows, cols] view) of random rows with the given pitch, single-level or [rows / T][T (+ spare)]"""
    pitch = pitch or cols
    if T:
        buf = torch.randn(rows // T, T + spare, pitch, generator=gen).cuda()
        return ops._rows3d(buf[:, :T, :cols]), buf
    buf = torch.randn(rows, pitch, generator=gen).cuda()
    return (buf[:, :cols], pitch, 0, 0), buf


def run_raw(tag, rows, Mg, Ng, opt):
    gen = torch.Generator().manual_seed(rows + 7 * Mg + Ng)
    ud, ukeep = rows_of(rows, Mg, opt.get('upitch'), opt.get('T'), gen, 0)
    vd, vkeep = rows_of(rows, Ng, opt.get('vpitch'), opt.get('T'), gen, 1)
    sh = torch.randn(Ng, generator=gen).cuda() if opt.get('shift') else None
    acc = (torch.ones(Mg, Ng).cuda(), torch.ones(Mg).cuda()) if opt.get('acc') else None
    Lb.query('gpe_reserve_cus_set', opt.get('reserve', 0))
    G, cs = ops.redgemm_raw(ud, vd, rows, Mg, Ng, want_colsum=not opt.get('nocs'), accumulate_into=acc, v_shift=sh)
    torch.cuda.synchronize()
    Lb.query('gpe_reserve_cus_set', 0)
    save(tag, G=G, colsum=cs)
    print('%s raw %s %s: ws %d floats, rc 0, G sum %r' % (tag, (rows, Mg, Ng), opt, Lb.query('gpe_redgemm_ws', Mg, Ng), float(G.double().sum())), flush=True)


def run_edge(tag, B, N, k, Mg, Ng, opt, mode):
    gen = torch.Generator().manual_seed(B * N + 7 * Mg + k)
    E, BN, pu = B * N * k, B * N, (Mg + 3) // 4 * 4
    u = torch.randn(E, pu, generator=gen).cuda()
    shift = torch.randn(Ng, generator=gen).cuda()
    G, cs = torch.zeros(Mg, Ng).cuda(), torch.zeros(Mg).cuda()
    nws = Lb.query('gpe_redgemm_ws', Mg, Ng)
    part = torch.empty(nws).cuda()
    ews, newsb = ops.edge_workspace(B, N, k, 2 * Ng, 'cuda') if opt.get('ws', 1) else (None, 0)
    words = torch.zeros(2, dtype=torch.int32, device='cuda')
    wu = wv = None
    v = pq = jg = None
    if opt.get('gather'):
        pq = torch.randn(BN, 2 * Ng, generator=gen).cuda()
        jg = (torch.randint(0, N, (B, N, k), generator=gen) + torch.arange(B).view(B, 1, 1) * N).int().cuda()
    else:
        v = torch.randn(E, Ng, generator=gen).abs().cuda()
    if mode == 'f16x3':
        Lb.call('gpe_absmax', u, pu, E, Mg, words[0:1])
        wu = words[0:1]
        if opt.get('words', 'both') == 'both':
            if opt.get('gather'):
                Lb.call('gpe_edge_pq_amax', pq, 2 * Ng, Ng, BN, words[1:2], *ops.edge_workspace(B, N, k, 2 * Ng, 'cuda'))
            else:
                Lb.call('gpe_absmax', v, Ng, E, Ng, words[1:2])
            wv = words[1:2]
    lz = (None, 0, None, None, 0, None)
    if opt.get('lazy'):
        agg = torch.zeros(BN, pu, dtype=torch.uint8, device='cuda')
        lz = (torch.randn(BN, Mg, generator=gen).cuda(), Mg, agg, agg.clone(), pu, torch.ones(4, Mg).cuda())
    Lb.query('gpe_reserve_cus_set', opt.get('reserve', 0))
    rc = 0
    try:
        Lb.call('gpe_edge_redgemm', u, pu, 0 if opt.get('gather') else 1, v, Ng, pq, 2 * Ng, jg, shift, B, N, k, Mg, Ng, G, Ng, cs, part, wu, wv,
                ews, newsb, *lz)
    except RuntimeError as e:                 # _lib.call raises on a non-zero return code and names it
        rc = int(re.search(r'failed with code (-?\d+)', str(e)).group(1))
    torch.cuda.synchronize()
    Lb.query('gpe_reserve_cus_set', 0)
    save(tag, G=G, colsum=cs)
    print('%s edge %s %s: ws %d floats, rc %d, G sum %r' % (tag, (B, N, k, Mg, Ng), opt, nws, rc, float(G.double().sum())), flush=True)


def run_layer(tag, Fo):
    """one EdgeConv layer 3 -> 200 -> 200 -> Fo at (B, N, k) = (8, 512, 16), f16x3: its backward takes a lazy reduce-GEMM (Fo = 150: the
    10 x 13 instance, 200: 13 x 13)"""
    B, N, C, k = 8, 512, 3, 16
    torch.manual_seed(5)
    conv = gpe.net_blocks.DynamicEdgeConv(gpe.net_blocks.MLP([2 * C, 200, 200, Fo]), k=k).cuda().train()
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(B * N, C, generator=gen).cuda().requires_grad_()
    wgt = torch.randn(B * N, Fo, generator=gen).cuda()
    lazy = Lb.query('gpe_edge_lazy_dz3_ok', B, N, k, Fo, 200)
    y = conv(x, B, N)
    try:
        (y * wgt).sum().backward()
    except RuntimeError as e:                 # GPE_RD_NOPC=1: the lazy call is refused (-22) — the same in every build
        print('%s layer %s -> %d: lazy_dz3_ok %d, backward refused: %s' % (tag, (B, N, k), Fo, lazy, str(e).splitlines()[-1]), flush=True)
        return
    torch.cuda.synchronize()
    save(tag, y=y, dx=x.grad, **{n.replace('.', '_'): p.grad for n, p in conv.named_parameters()})
    print('%s layer %s -> %d: lazy_dz3_ok %d, dx sum %r' % (tag, (B, N, k), Fo, lazy, float(x.grad.double().sum())), flush=True)


for mode in ('f32', 'bf16x3', 'f16x3'):
    gpe.set_math(mode)
    for dbg in ((0, 16384) if mode == 'f16x3' else (0,)):
        Lb.query('gpe_debug_set', dbg)
        for ci, (rows, Mg, Ng, opt) in enumerate(RAW):
            if mode in opt.get('modes', (mode,)):
                run_raw('%s_d%d_raw%02d' % (mode, dbg, ci), rows, Mg, Ng, opt)
    Lb.query('gpe_debug_set', 0)
    for ci, (B, N, k, Mg, Ng, opt) in enumerate(EDGE):
        if mode in opt.get('modes', (mode,)):
            run_edge('%s_edge%02d' % (mode, ci), B, N, k, Mg, Ng, opt, mode)
run_layer('f16x3_layer150', 150)
run_layer('f16x3_layer200', 200)
gpe.set_math('f32')

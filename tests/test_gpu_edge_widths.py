"""-m gpu: the fused edge GEMM kernels at every width class and boundary of their menu, through DynamicEdgeConv.

The register-stationary families take any width in (96, 208] in two tile classes (10 or 13 tiles of 16 columns / chunks of 16 k,
csrc/gpe_edge_dispatch.h:24-25) and four launch kinds (F2 gather forward H -> H, F3 dense forward H -> Fo with the aggregation,
B3 in-place backward Fo -> H, B2 gathered backward H -> H).  The rest of the suite runs them at H = 200, Fo = 150 only; here a layer
[2C, H, H, Fo] runs at the widths that put every (NT, KCH) class, the full and the half last K chunk, the lower bounds of the
two-waves-per-SIMD family, the clamped last column quad and both edges of the menu under every arithmetic mode, against the fp64
oracle on the build's graph and on the build's ReLU / argmax decisions (tests/relu_align.py), with the bars of
test_gpu_kernels.TOL.  Then: the alternative families of the exact mode on identical inputs (gpe_debug_set 64 / 128 / 256), and
that no result depends on what `torch.empty` memory held before."""
import copy
import gc

import pytest
import torch

from relu_align import ARGSEL_TOL, align_relus, capture_relu_masks, check_alignment
from test_gpu_kernels import TOL, _oracle_conv, _product_conv, gpe, relerr, relerr_fro  # noqa: F401  (gpe: the module's fixture; relerr_fro: TOL's norm)

pytestmark = pytest.mark.gpu

# Which family runs each launch kind, read from the selection code (the library has no query for it):
#   gpe_edgegemm_try            csrc/gpe_edge_dispatch.hip:89-132   menu test :97, bf16x6 :106-109, f16x3 (w8, then single-role) :112-122,
#                                                                   exact single-role :125-128, producer/consumer :129-130
#   menu / classes / tiles      csrc/gpe_edge_dispatch.h:24-25 (width in (96, 208], class 10 up to 160, else 13), :34-41, :79-86
#   gpe_edge_w8                 csrc/gpe_edgegemm_w8.hip:42-46 (k = 16 / 5 / four-row pseudo-points; plane row >= 384 B at KCH 13, 256 B at
#                                                               KCH 10: K >= 192 / 128)
#   W8Menu                      csrc/gpe_edgegemm_w8_kernel.h:779-785 (F2, B2 at (13,13); F3 at (NT 10, KCH 13); B3 at (NT 13, KCH 10))
#   Bf16x6Menu, gpe_edge_bf16x6 csrc/gpe_edgegemm_x6.hip:7-15 (NT 10 or KCH 10; NT 13 forward only)
#   gpe_edge_sr                 csrc/gpe_edgegemm_sr.hip:97 (declines B3 at (13,13))
#   sr_launch                   csrc/gpe_edgegemm_sr_kernel.h:527-557 (HALF: K <= 16 (KCH - 1) + 8, :529; k = 16 / four-row / generic k)
#   the edge entry points       csrc/gpe_rowgemm.hip:431-436, 489-494 (not on the menu: the generic LDS-streamed kernel)
# SR single-role exact fp32, PC producer/consumer exact fp32, X6 single-role split bf16x6, W8 two waves per SIMD f16x3, H3 single-role
# split f16x3, PCb producer/consumer two-term split-bf16, GEN the generic LDS-streamed kernel.  Per kind: (NT, KCH) -> family.
# 'mixed' and 'bf16x3' are both row-GEMM arithmetic 1 (csrc/gpe_state.hip:24-28): never re-tiled (:103), always PCb (:129-130).
#
#  (H, Fo)     F2            F3            B3            B2           | f32          bf16x6        f16x3 (k 16/5/20)  f16x3 (k 8)  mixed, bf16x3
#  (208,160)   (13,13) full  (10,13) full  (13,10) full  (13,13) full | SR SR SR SR  SR X6 SR SR   W8 W8 W8 W8        -            PCb x 4
#  (192,128)   (13,13) half  (10,13) half  (13,10) half  (13,13) half | SR SR SR SR  SR X6 SR SR   W8 W8 W8 W8        -            PCb x 4
#              K = 192 / 128: plane rows of exactly 384 / 256 bytes, the last K chunk empty
#  (188,124)   (13,13) half  (10,13) half  (13,10) half  (13,13) half | SR SR SR SR  SR X6 SR SR   H3 H3 H3 H3        -            PCb x 4
#              plane rows of 376 / 248 bytes: gpe_edge_w8 declines (:46)
#  (100,100)   (10,10) half  (10,10) half  (10,10) half  (10,10) half | SR SR SR SR  X6 X6 X6 X6   H3 H3 H3 H3        -            PCb x 4
#              three empty chunks and tiles; no (10,10) on W8Menu; k = 20 with E % 64 == 0: SR's straight-line four-row instances (:547)
#  (160,164)   (10,10) full  (13,10) full  (10,13) half  (10,10) full | SR SR SR SR  X6 X6 X6 X6   H3 H3 H3 H3        H3 x 4       PCb x 4
#              B3's K = 164: HALF with two empty chunks; F3 / B3 in the transposed classes, not on W8Menu
#  (196,208)   (13,13) half  (13,13) half  (13,13) full  (13,13) half | SR SR PC SR  SR SR PC SR   W8 H3 H3 W8        -            PCb x 4
#              B3 (13,13): gpe_edge_sr (:97) and gpe_edge_bf16x6 (:13) decline; F3 (13,13) is not on Bf16x6Menu
#  (204,157)   (13,13) full  (10,13) full  (13,10) full  (13,13) full | SR SR SR SR  SR X6 SR SR   W8 W8 W8 W8        -            PCb x 4
#              K = 204: four dead columns in a full chunk; forward N = 157 (pitch 160); B3's K = 157: last quad with one live column
#  (96,212), (256,212)   off the menu (:97 -> GPE_EDGE_NOT_MINE)           | GEN x 4 in every mode
# k = 20 runs as five four-row pseudo-points (gpe_edge_pseudo_kq, csrc/gpe_edge_dispatch.hip:8-14): W8's k = 4 instances in f16x3, SR's
# KC = 4 instances in f32 (full K at 208: generic k for B2 (13,13), csrc/gpe_edgegemm_sr_kernel.h:544); B3 needs nothing per point and
# always runs four-row tiles (:34).  The P|Q projection in front of F2 is a dense GEMM of K = C (C = 24, 150: the wide input).
WIDTH_CASES = [
    # (H, Fo, B, N, k, C)       k = 16 at every width, B * N not a multiple of the tile's 4 points
    (208, 160, 2, 67, 16, 3),
    (192, 128, 1, 130, 16, 3),
    (188, 124, 2, 67, 16, 3),
    (100, 100, 1, 130, 16, 3),
    (160, 164, 2, 67, 16, 3),
    (196, 208, 1, 130, 16, 3),
    (204, 157, 2, 67, 16, 3),
    (96, 212, 1, 130, 16, 3),
    (256, 212, 2, 67, 16, 3),
    # k = 5: W8's 60-row tile of 12 points, E = 670 / 750 rows (E % 60 = 10 / 30)
    (208, 160, 2, 67, 5, 3),
    (192, 128, 3, 50, 5, 3),
    # k = 20 as pseudo-points: E = 2560 = 40 * 64 rows, and E = 1800 (E % 64 = 8)
    (208, 160, 2, 64, 20, 3),
    (208, 160, 1, 90, 20, 3),
    (100, 100, 2, 64, 20, 3),
    (100, 100, 1, 90, 20, 3),
    # k = 8: two points per wave, E = 616 (E % 64 = 40)
    (160, 164, 1, 77, 8, 3),
    # the wide P|Q input
    (208, 160, 2, 67, 16, 24),
    (208, 160, 1, 130, 16, 150),
]

_REF = {}        # per shape: the C definition's graph and the fp32 oracle's forward (neither depends on the arithmetic mode)


def _inputs(H, Fo, B, N, k, C):
    oconv = _oracle_conv(C, H, Fo, k, seed=H + Fo + B + N + k + C)      # includes negative BatchNorm scales: the min side
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * N, C, generator=g)
    wgt = torch.randn(B * N, Fo, generator=g)
    return oconv, x, wgt


def _run_build(gpe, oconv, x, wgt, H, Fo, B, N, k, C):
    """One training forward + backward of the build on a fresh copy of the layer -> (results, the decisions it took)."""
    pconv = _product_conv(gpe, oconv, C, H, Fo, k).train()
    xd = x.cuda().requires_grad_()
    with capture_relu_masks() as masks:
        out = pconv(xd, B, N)
    (out * wgt.cuda()).sum().backward()
    torch.cuda.synchronize()
    res = {'out': out.detach().clone(), 'dx': xd.grad.clone(), 'knn': pconv.last_knn.clone(),
           'grads': {n: p.grad.clone() for n, p in pconv.named_parameters()},
           'bufs': {n: b.clone() for n, b in pconv.named_buffers()}}
    return res, masks


def _check_against_oracle(res, masks, oconv, x, wgt, H, Fo, B, N, k, C, tol, tag):
    """The bars of test_edgeconv_layer_at_every_reservation: forward, dx, every parameter gradient, the running statistics and the
    graph, the fp64 oracle standing on the build's graph and decisions."""
    from oracle import ref_path as O
    key = (H, Fo, B, N, k, C)
    batch = torch.arange(B).repeat_interleave(N)
    if key not in _REF:
        ref_idx = O.knn_local(x, B, k)
        o32 = copy.deepcopy(oconv).train()
        o32.knn_override = ref_idx
        with torch.no_grad():
            _REF[key] = (ref_idx, o32(x.clone(), batch))
    ref_idx, out_32 = _REF[key]
    assert torch.equal(res['knn'].cpu().view(B * N, k).long(), ref_idx)

    o64 = copy.deepcopy(oconv).double().train()
    o64.knn_override = ref_idx
    st = align_relus(o64, masks)
    if masks.argsel:
        o64.argsel_override = masks.argsel[0]
    xr = x.double().requires_grad_()
    out_r = o64(xr, batch)
    check_alignment(st, len(masks))
    assert o64.argsel_gap < ARGSEL_TOL
    (out_r * wgt.double()).sum().backward()

    err32 = relerr(out_32, out_r)
    err = relerr(res['out'], out_r)
    e_dx = tol.get('dx_norm', tol['norm'])(res['dx'], xr.grad)
    e_p = {n: tol['norm'](res['grads'][n], p.grad) for n, p in o64.named_parameters()}
    e_b = {n: relerr(res['bufs'][n], b) for n, b in o64.named_buffers() if 'num_batches' not in n}
    worst = max(e_p, key=e_p.get)
    print('%s H=%d Fo=%d B=%d N=%d k=%d C=%d: fwd %.2e (oracle-fp32 %.2e) dx %.2e dparam %.2e (%s) running %.2e, %d decisions aligned'
          % (tag, H, Fo, B, N, k, C, err, err32, e_dx, e_p[worst], worst, max(e_b.values()), st['flips']))
    assert err < max(tol['fwd'], 20 * err32), ('fwd', err)
    assert e_dx < tol['dx'], ('dx', e_dx)
    for n, e in e_p.items():
        assert e < tol['dparam'], (n, e)
    for n, bbuf in o64.named_buffers():
        if 'num_batches' in n:
            assert res['bufs'][n].item() == bbuf.item()
        else:
            assert e_b[n] < 1e-5, (n, e_b[n])


# --------------------------------------------------------------------------------------------------
# 1. layer parity over the width list, every arithmetic mode
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,Fo,B,N,k,C', WIDTH_CASES)
def test_edgeconv_layer_at_every_width_class(gpe, math_mode, H, Fo, B, N, k, C):
    oconv, x, wgt = _inputs(H, Fo, B, N, k, C)
    res, masks = _run_build(gpe, oconv, x, wgt, H, Fo, B, N, k, C)
    _check_against_oracle(res, masks, oconv, x, wgt, H, Fo, B, N, k, C, TOL[math_mode], math_mode)


@pytest.mark.parametrize('H,Fo', [(208, 160), (100, 100), (204, 157)])
def test_edgeconv_eval_forward_at_width_classes(gpe, H, Fo):
    """Evaluation mode (no statistics launch, BatchNorm from running buffers away from their defaults): the bar of
    test_edgeconv_eval_mode."""
    B, N, C, k = 2, 67, 3, 16
    oconv = _oracle_conv(C, H, Fo, k, seed=H + Fo)
    with torch.no_grad():
        for blk in oconv.nn:
            blk[2].running_mean.uniform_(0.1, 0.4)
            blk[2].running_var.uniform_(0.5, 1.5)
    pconv = _product_conv(gpe, oconv, C, H, Fo, k).eval()
    x = torch.randn(B * N, C, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        out = pconv(x.cuda(), B, N)
    o64 = copy.deepcopy(oconv).double().eval()
    o64.knn_override = pconv.last_knn.cpu().view(B * N, k).long()
    ref = o64(x.double(), torch.arange(B).repeat_interleave(N))
    e = relerr(out, ref)
    print('eval H=%d Fo=%d: fwd %.2e' % (H, Fo, e))
    assert e < 1e-5
    assert dict(pconv.named_buffers())['nn.0.2.num_batches_tracked'].item() == 0


# --------------------------------------------------------------------------------------------------
# 2. exact mode: the alternative families on identical inputs
# --------------------------------------------------------------------------------------------------
AB_CASES = [(H, Fo, B, N, k, 3) for H, Fo in [(200, 150), (208, 160), (100, 100), (164, 100), (192, 128)]
            for B, N, k in [(2, 67, 16), (2, 64, 20)]]


@pytest.mark.parametrize('H,Fo,B,N,k,C', AB_CASES)
def test_exact_mode_families_agree(gpe, H, Fo, B, N, k, C):
    """'f32' only.  gpe_debug_set(64): the producer/consumer family in place of the single-role one (csrc/gpe_edge_dispatch.hip:125);
    128: no half last K chunk (csrc/gpe_edgegemm_sr_kernel.h:529); 256 (k = 20): generic k in place of the four-row form (:545).
    The three bits are read by host selection code only — and 128 also by the f16x3 scale passes (csrc/gpe_edgegemm_h3.hip:166),
    where it reuses stale scale words: it is never set outside 'f32'.  Every run meets the oracle bars; forwards agree pairwise."""
    L = gpe._lib
    tol = TOL['f32']
    oconv, x, wgt = _inputs(H, Fo, B, N, k, C)
    outs = {}
    prev = gpe.set_math('f32')
    try:
        assert L.get_math() == 'f32'
        for flag in (0, 64, 128) + ((256,) if k == 20 else ()):
            L.query('gpe_debug_set', flag)
            try:
                res, masks = _run_build(gpe, oconv, x, wgt, H, Fo, B, N, k, C)
            finally:
                L.query('gpe_debug_set', 0)
            _check_against_oracle(res, masks, oconv, x, wgt, H, Fo, B, N, k, C, tol, 'f32 debug=%d' % flag)
            outs[flag] = res['out']
    finally:
        L.query('gpe_debug_set', 0)
        gpe.set_math(prev)
    flags = sorted(outs)
    for i, a in enumerate(flags):
        for b in flags[i + 1:]:
            e = relerr(outs[a], outs[b])
            print('H=%d Fo=%d k=%d: forward debug=%d vs debug=%d %.2e' % (H, Fo, k, a, b, e))
            assert e < tol['fwd'], (a, b, e)


# --------------------------------------------------------------------------------------------------
# 3. results do not depend on unwritten memory
# --------------------------------------------------------------------------------------------------
def _free_blocks():
    """Sizes of the blocks the caching allocator holds free for the current stream (what torch.empty is served from)."""
    dev, stream = torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream
    sizes = []
    for seg in torch.cuda.memory_snapshot():
        if seg['device'] != dev or seg['stream'] != stream:
            continue
        for b in seg['blocks']:
            if b['state'] != 'inactive':
                continue
            n = b['size']
            # (a request above 1 MiB is served from the large pool: the rare larger free block of a small-pool segment goes in pieces)
            while seg.get('segment_type') == 'small' and n > (1 << 20):
                sizes.append(1 << 20)
                n -= 1 << 20
            sizes.append(n)
    return sizes


def _poison_free_device_memory():
    """Leaves all-ones bytes (NaN as fp32 and as fp16) in every byte the caching allocator will hand out next.  Segments that are
    wholly free go back to the driver (empty_cache).  The free fragments of segments that live tensors keep are taken one by one: a
    request of exactly a free block's size is served by that block (best fit), so holding one filled tensor per free block of the
    allocator's own snapshot covers them all.  On top, 16 x 16 MiB (a segment of the large pool each) and 64 x 1 MiB (two fill a
    2 MiB segment of the small pool) are filled the same way.  Freeing all of it leaves only poisoned blocks in both pools."""
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()
    held = []
    for _ in range(16):                                 # (a request that had to reserve leaves a remainder: next round)
        free = _free_blocks()
        if not free:
            break
        held += [torch.full((size,), 255, dtype=torch.uint8, device='cuda') for size in sorted(free, reverse=True)]
    held += [torch.full((16 << 20,), 255, dtype=torch.uint8, device='cuda') for _ in range(16)]
    held += [torch.full((1 << 20,), 255, dtype=torch.uint8, device='cuda') for _ in range(64)]
    left = _free_blocks()
    assert not left, ('free blocks that were not poisoned', left)
    torch.cuda.synchronize()
    del held
    torch.cuda.synchronize()


@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
@pytest.mark.parametrize('H,Fo,B,N,k', [(200, 150, 2, 67, 16), (204, 157, 2, 67, 16), (100, 100, 1, 130, 16), (200, 150, 1, 90, 20)])
def test_results_do_not_depend_on_unwritten_memory(gpe, mode, H, Fo, B, N, k):
    """Activations, aggregates and workspaces come from torch.empty with row pitches rounded up to 4, and pad columns are fetched by
    16-byte loads: a second run over memory that held NaN must give the same bits as the first (repeats are bit-reproducible)."""
    C = 3
    oconv, x, wgt = _inputs(H, Fo, B, N, k, C)
    prev = gpe.set_math(mode)
    gate = gpe.set_f16x3_min_rows(0)
    try:
        first, _ = _run_build(gpe, oconv, x, wgt, H, Fo, B, N, k, C)
        _poison_free_device_memory()
        for buf in gpe.ops._WS.values():                 # the grow-only workspaces of the C-ABI calls: all-ones bytes, NaN as floats
            buf.fill_(255)
        # the precondition, not a skip: what the layer allocates next comes back holding NaN — rows of an activation, a per-point
        # aggregate, the [P|Q] table.  (Looked at on the host: a device-side isnan() would put its own result into the pools.)
        E = B * N * k
        for shape in [(E, (H + 3) // 4 * 4), (E, (Fo + 3) // 4 * 4), (B * N, (Fo + 3) // 4 * 4), (B * N, 2 * H)]:
            probe = torch.empty(*shape, device='cuda')
            assert bool(torch.isnan(probe.cpu()).all()), ('the allocator handed out a block that was not poisoned', shape)
            del probe
        second, _ = _run_build(gpe, oconv, x, wgt, H, Fo, B, N, k, C)
    finally:
        gpe.set_f16x3_min_rows(gate)
        gpe.set_math(prev)
    assert torch.equal(first['knn'], second['knn'])
    for name in ('out', 'dx'):
        assert not torch.isnan(second[name]).any(), name
        assert torch.equal(first[name], second[name]), (name, relerr(second[name], first[name]))
    for kind in ('grads', 'bufs'):
        for n, t in first[kind].items():
            assert torch.equal(t, second[kind][n]), (kind, n, relerr(second[kind][n].float(), t.float()))

"""-m gpu: kernel parity across compute-unit reservations, grid sizes and cloud pinning.

Many launches size their grid from gpe_num_cus() = the device's CU count minus the process-wide reservation
(include/gpe_hip.h gpe_reserve_cus_set), and several pin clouds to XCDs depending on the batch.  Those two inputs pick
the kernel, the tile walk and the number of fp64 partial sums.  The rest of the suite runs at one setting (all 256 CUs
of an MI355X); here every case runs at reservations R in RESERVES — 256, 252, 240, 156 and 64 usable CUs on an MI355X,
which is also what a partitioned device looks like — with shapes that put each grid-size decision on both sides of its
threshold for the R in use.  Oracles and bars are those of tests/test_gpu_kernels.py and tests/test_gpu_model.py.

Results are not bit-identical across reservations (summation order and kernel choice change), except the kNN graphs,
which are exact at every R."""
import copy

import pytest
import torch

from relu_align import ARGSEL_TOL, align_relus, capture_relu_masks, check_alignment
from test_gpu_kernels import TOL, _oracle_conv, _product_conv, gpe, relerr  # noqa: F401  (gpe: the module's fixture)
from test_gpu_model import _synthetic_case, _whole_batch_gradient_parity

pytestmark = pytest.mark.gpu

RESERVES = [0, 4, 16, 100, 192]
RD_RT = 32                      # rows per reduce-GEMM row tile (csrc/gpe_redgemm.hip)


def _usable_cus(reserve):
    """What gpe_num_cus() answers at this reservation (csrc/gpe_state.hip)."""
    c = torch.cuda.get_device_properties(0).multi_processor_count
    if c <= 0:
        c = 256
    return max(c - reserve, 8)


def _rid(r):
    return 'R%d' % r


@pytest.fixture(autouse=True)
def _no_leaked_reservation(gpe):
    """No case may start under, or leave behind, a reservation: the rest of the suite runs on the whole chip."""
    before = gpe.get_reserved_cus()
    assert before == 0, 'a reservation of %d CUs leaked into this test' % before
    yield
    after = gpe.get_reserved_cus()
    if after:
        gpe.set_reserved_cus(0)
    assert after == 0, 'the test left %d CUs reserved' % after


@pytest.fixture(params=RESERVES, ids=_rid)
def reserve(request, gpe):
    """-> (R, usable CUs): R compute units left out of every persistent launch for the duration of the test."""
    r = request.param
    prev = gpe.set_reserved_cus(r)
    try:
        cus = _usable_cus(r)
        print('reserved CUs %d -> %d usable' % (r, cus))
        yield r, cus
    finally:
        gpe.set_reserved_cus(prev)


# --------------------------------------------------------------------------------------------------
# 1. kNN, bit-exact against oracle/knn_ref.c at every R (so also bit-identical across R)
# --------------------------------------------------------------------------------------------------
KNN_GRID_CASES = [
    # layer-2 filter path (threshold scan, 64 or 128 queries per workgroup: wide when B * ceil(N / 128) >= usable CUs)
    (8, 2048, 150, 16),     # 128 query tiles: narrow at R <= 100, wide at R = 192; 8 clouds pinned, one per XCD
    (12, 1000, 150, 16),    # 96 query tiles: narrow except at R = 192; B % 8 != 0, pinned unevenly (two XCDs hold two clouds)
    (16, 2048, 150, 16),    # 256 query tiles: wide at every R; two clouds per XCD
    (12, 2048, 3, 16),      # xyz path (sorted-cloud kernel), 12 clouds pinned unevenly
]
_KNN_REF = {}
_KNN_SEEN = {}


@pytest.mark.parametrize('B,N,C,k', KNN_GRID_CASES)
def test_knn_bit_exact_at_every_reservation(gpe, reserve, B, N, C, k):
    from oracle import ref_path as O
    key = (B, N, C, k)
    g = torch.Generator().manual_seed(B * 1000 + N + C + k + 7)
    x = torch.randn(B * N, C, generator=g)
    if key not in _KNN_REF:                      # the C definition's graph does not depend on R: computed once per shape
        _KNN_REF[key] = O.knn_local(x, B, k).to(torch.int32).view(B, N, k)
    got = gpe.ops.knn(x.cuda(), B, N, k).cpu()
    bad = (got != _KNN_REF[key]).any(-1).sum().item()
    assert bad == 0, '%d / %d queries differ at R = %d' % (bad, B * N, reserve[0])
    if key in _KNN_SEEN:
        assert torch.equal(got, _KNN_SEEN[key])
    _KNN_SEEN[key] = got


# --------------------------------------------------------------------------------------------------
# 2. EdgeConv layer forward + backward (H = 200, F = 150: the register-stationary / two-plane edge kernels)
# --------------------------------------------------------------------------------------------------
EDGE_GRID_CASES = [
    # (B, N, k)
    (8, 512, 16),     # pinned: 128 tiles of 64 rows per cloud, gx / 8 workgroups per XCD (32 / 30 / 8 at R = 0 / 16 / 192, none at
                      # R = 4 / 100: gx % 8 != 0); f16x3 lazy dz3 at every R (rows / 32 = 2048 >= 8 * usable CUs)
    (16, 256, 16),    # pinned, two clouds per XCD
    (12, 300, 16),    # B % 8 != 0: edge kernels unpinned, gather-stats / pull-dq / kNN walks pinned unevenly; lazy dz3 only at R >= 100
    (8, 301, 16),     # 4816 rows per cloud, not a multiple of the 64-row tile: unpinned; lazy dz3 only at R = 192
    (8, 400, 5),      # k = 5: the two-wave generic kernels, ragged last tile
    (8, 256, 20),     # k = 20: pseudo-points (5 x 4 rows per point, folded afterwards)
]


@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
@pytest.mark.parametrize('B,N,k', EDGE_GRID_CASES)
def test_edgeconv_layer_at_every_reservation(gpe, reserve, mode, B, N, k):
    """The bars of test_edgeconv_layer_fwd_bwd against the fp64 oracle on the build's graph.  At 2400 - 4800 points a handful of
    ReLU / max-aggregation decisions sit within rounding of a tie, so the fp64 oracle also stands on the build's decisions
    (tests/relu_align.py: allowed only where |z_fp64| < 5e-5 or the two messages are that close)."""
    from oracle import ref_path as O
    C, H, Fo = 3, 200, 150
    tol = TOL[mode]
    prev = gpe.set_math(mode)
    gate = gpe.set_f16x3_min_rows(0)            # as the math_mode fixture: the fp16-pipe kernels at these sizes too
    try:
        oconv = _oracle_conv(C, H, Fo, k, seed=B + N + k)
        pconv = _product_conv(gpe, oconv, C, H, Fo, k)
        g = torch.Generator().manual_seed(2)
        x = torch.randn(B * N, C, generator=g)
        wgt = torch.randn(B * N, Fo, generator=g)
        batch = torch.arange(B).repeat_interleave(N)
        xd = x.cuda().requires_grad_()
        pconv.train()
        with capture_relu_masks() as masks:
            out = pconv(xd, B, N)
        (out * wgt.cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        gpe.set_f16x3_min_rows(gate)
        gpe.set_math(prev)

    ref_idx = O.knn_local(x, B, k)
    assert torch.equal(pconv.last_knn.cpu().view(B * N, k).long(), ref_idx)

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

    o32 = copy.deepcopy(oconv).train()
    o32.knn_override = ref_idx
    out_32 = o32(x.clone(), batch)
    err32 = relerr(out_32, out_r)
    err = relerr(out, out_r)
    print('R=%d %s edgeconv fwd relerr build=%.2e oracle-fp32=%.2e (ReLU decisions aligned: %d)' % (reserve[0], mode, err, err32, st['flips']))
    assert err < max(tol['fwd'], 20 * err32)
    e = tol.get('dx_norm', tol['norm'])(xd.grad, xr.grad)
    assert e < tol['dx'], ('dx', e)
    pn = dict(pconv.named_parameters())
    for n, p in o64.named_parameters():
        e = tol['norm'](pn[n].grad, p.grad)
        assert e < tol['dparam'], (n, e)
    pb = dict(pconv.named_buffers())
    for n, bbuf in o64.named_buffers():
        if 'num_batches' in n:
            assert pb[n].item() == bbuf.item()
        else:
            assert relerr(pb[n], bbuf) < 1e-5, n


# --------------------------------------------------------------------------------------------------
# 3. gpe_edge_redgemm, dense and gathered V (after test_edge_redgemm_producer_consumer_tiles)
# --------------------------------------------------------------------------------------------------
def _edge_redgemm_case(gpe, mode, B, N, k, Mg, Ng, seed):
    """G = U^T (V - shift) and colsum(U) of an E-row edge product against fp64 on the device: NaN pad columns of U and V must never
    reach an output."""
    L = gpe._lib
    g = torch.Generator(device='cuda').manual_seed(seed)
    E = B * N * k
    pu = (Mg + 3) // 4 * 4 + 4
    ubuf = torch.full((E, pu), float('nan'), device='cuda')
    ubuf[:, :Mg] = torch.randn(E, Mg, device='cuda', generator=g)
    shift = torch.randn(Ng, device='cuda', generator=g)
    G = torch.empty(Mg, Ng, device='cuda')
    cs = torch.empty(Mg, device='cuda')
    ws = torch.empty(L.query('gpe_redgemm_ws', Mg, Ng), device='cuda')
    if mode == 'dense':
        pv = Ng + 8
        vbuf = torch.full((E, pv), float('nan'), device='cuda')
        vbuf[:, :Ng] = torch.randn(E, Ng, device='cuda', generator=g)
        L.call('gpe_edge_redgemm', ubuf, pu, 1, vbuf, pv, None, 0, None, shift, B, N, k, Mg, Ng, G, Ng, cs, ws, None, None, None, 0, None, 0, None, None, 0, None)
        vref = vbuf[:, :Ng].double() - shift.double()
    else:
        pq = torch.randn(B * N, 2 * Ng, device='cuda', generator=g)
        jg = (torch.randint(0, N, (B, N, k), device='cuda', generator=g) + torch.arange(B, device='cuda').view(B, 1, 1) * N).int()
        L.call('gpe_edge_redgemm', ubuf, pu, 0, None, 0, pq, 2 * Ng, jg, shift, B, N, k, Mg, Ng, G, Ng, cs, ws, None, None, None, 0, None, 0, None, None, 0, None)
        i = torch.arange(B * N, device='cuda').repeat_interleave(k)
        vref = torch.relu(pq[i, :Ng].double() + pq[jg.view(-1).long(), Ng:].double()) - shift.double()
    uref = ubuf[:, :Mg].double()
    assert relerr(G, uref.t() @ vref) < 3e-6, (mode, B, N, k, Mg, Ng)
    assert relerr(cs, uref.sum(0)) < 3e-6


@pytest.mark.parametrize('Mg', [150, 200])
@pytest.mark.parametrize('mode', ['dense', 'gather'])
@pytest.mark.parametrize('side', ['below', 'above'])
def test_edge_redgemm_around_the_producer_consumer_threshold(gpe, reserve, side, mode, Mg):
    """The producer/consumer kernels need >= 4 row tiles per workgroup (num_tiles >= 4 gx, gx = usable CUs for these 10 / 13 x 13 tile
    grids).  One tile below: the deep kernel (dense V) or the generic kernel (gathered V); one tile above: producer/consumer.  Row
    counts are ragged (rows % 32 != 0); gathered cases are one cloud (never pinned)."""
    R, cus = reserve
    gx = min(cus, 256)
    tiles = 4 * gx - 1 if side == 'below' else 4 * gx + 1
    f = gpe.set_math('f32')
    try:
        if mode == 'dense':
            rows = tiles * RD_RT - 13 if side == 'below' else (tiles - 1) * RD_RT + 13
            assert (rows + RD_RT - 1) // RD_RT == tiles
            _edge_redgemm_case(gpe, 'dense', 1, rows, 1, Mg, 200, seed=R * 7 + tiles + Mg)
        else:
            N = 8 * gx - 3 if side == 'below' else 8 * gx + 1          # k = 16: 16 * N rows, cdiv by 32 = tiles, half a tile ragged
            assert (16 * N + RD_RT - 1) // RD_RT == tiles
            _edge_redgemm_case(gpe, 'gather', 1, N, 16, Mg, 200, seed=R * 7 + tiles + Mg)
    finally:
        gpe.set_math(f)


@pytest.mark.parametrize('B,N', [(32, 2048), (8, None)])
def test_edge_redgemm_gathered_pinning(gpe, reserve, B, N):
    """Gathered V with cloud -> XCD pinning (B % 8 == 0, gx % 8 == 0, whole row tiles per cloud): (32, 2048, 16) is cfg 2's layer —
    pinned at R = 0 / 16 / 192, where each XCD's gx / 8 workgroups walk 1024 tiles per cloud (32, 30, 8: a remainder at R = 16), and
    unpinned at R = 4 / 100 (gx % 8 != 0); (8, gx + 2, 16) sits just above the producer/consumer threshold with (gx + 2) / 2 tiles per
    cloud for gx / 8 workgroups of an XCD."""
    R, cus = reserve
    gx = min(cus, 256)
    if N is None:
        N = gx + 2
    f = gpe.set_math('f32')
    try:
        _edge_redgemm_case(gpe, 'gather', B, N, 16, 200, 200, seed=R + B)
    finally:
        gpe.set_math(f)


# --------------------------------------------------------------------------------------------------
# 4. dense redgemm around the deep-kernel switch, and the split-bf16 weight-gradient GEMM's split count
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', ['below', 'above'])
def test_redgemm_around_the_deep_kernel_switch(gpe, reserve, side):
    """1000 x 250 outputs (the decoders' weight-gradient shape) make a 5-high block grid, gx = usable CUs / 5; fewer than 64 gx row
    tiles run the deep kernel, more the generic big-block kernel (exact fp32 mode).  One ragged tile either side."""
    R, cus = reserve
    Mg, Ng = 1000, 250
    gx = min(cus, 256) // 5
    tiles = 64 * gx - 1 if side == 'below' else 64 * gx + 1
    rows = tiles * RD_RT - 7 if side == 'below' else (tiles - 1) * RD_RT + 9
    ops = gpe.ops
    g = torch.Generator(device='cuda').manual_seed(rows)
    u = torch.randn(rows, Mg, device='cuda', generator=g)
    v = torch.randn(rows, Ng, device='cuda', generator=g)
    f = gpe.set_math('f32')
    try:
        G, cs = ops.redgemm_raw(ops._rows2d(u), ops._rows2d(v), rows, Mg, Ng)
    finally:
        gpe.set_math(f)
    e = relerr(G, u.double().t() @ v.double())
    print('R=%d %s: %d rows, relerr %.2e' % (R, side, rows, e))
    assert e < 3e-6
    assert relerr(cs, u.double().sum(0)) < 3e-6


def test_split_bf16_weight_gradient_split_count(gpe, reserve):
    """f16x3: the decoders' 10304 x 1000 x 250 weight gradient on the bf16 pipe (csrc/gpe_gemm_x6.hip), split over
    S = usable CUs / 16 row ranges (16, 15, 15, 9, 4 partial images); the bars of test_dense_gemms_on_the_bf16_pipe, and
    gpe_debug_set(16384) (the exact kernels) gives other bits: that path really ran."""
    from gpe_amd import _lib as Lb
    ops = gpe.ops
    rows, Mg, Ng, T = 10304, 1000, 250, 14
    Bn = rows // T
    g = torch.Generator(device='cuda').manual_seed(17)
    ub = torch.randn(Bn, T, Mg, device='cuda', generator=g)
    vb = torch.randn(Bn, T + 1, (Ng + 3) // 4 * 4, device='cuda', generator=g)
    ud, vd = ops._rows3d(ub), ops._rows3d(vb[:, :T, :Ng])
    u, v = ub.reshape(rows, Mg).double(), vb[:, :T, :Ng].reshape(rows, Ng).double()
    ref = u.t() @ v
    prev = gpe.set_math('f16x3')
    outs = []
    try:
        for dbg in (0, 16384):
            Lb.query('gpe_debug_set', dbg)
            G, cs = ops.redgemm_raw(ud, vd, rows, Mg, Ng)
            assert relerr(G, ref) < 3e-6, dbg
            assert relerr(cs, u.sum(0)) < 3e-6
            outs.append(G)
    finally:
        Lb.query('gpe_debug_set', 0)
        gpe.set_math(prev)
    assert not torch.equal(outs[0], outs[1])


# --------------------------------------------------------------------------------------------------
# 5. LSTM decoder where the persistent plan changes with R (the persistent-stack repeats at R = 4 / 100 / 192 are parameters of
#    test_gpu_kernels.test_multi_tile_persistent_lstm_forward)
# --------------------------------------------------------------------------------------------------
def test_lstm_decoder_persistent_plan_at_every_reservation(gpe, reserve):
    """Four layers of 250 (L * NB = 64 workgroups per row group) over 32 rows (two row tiles).  The persistent stack needs a row group
    per row tile, RG = min(usable / 64, 2): one launch at R <= 100, the diagonal launches at R = 192 (RG = 1; L * NB cannot exceed 64
    usable CUs, since a persistent stack has at most 4 layers of 16 column blocks).  Against the fp64 oracle decoder with the bars of
    test_lstm_decoder_fwd_bwd."""
    from oracle import ref_path as O
    Bn, In, Hh, T, L, Out = 32, 250, 250, 14, 4, 8
    torch.manual_seed(Bn + T + L)
    odec = O.LSTMDecoderModule(In, Hh, Out, L, custom_init='kaiming_normal_')
    pdec = gpe.net_blocks.LSTMDecoderModule(In, Hh, Out, L, custom_init='kaiming_normal_')
    pdec.load_state_dict(odec.state_dict())
    pdec = pdec.cuda()
    enc = torch.randn(Bn, In, generator=torch.Generator().manual_seed(1))
    wgt = torch.randn(Bn, T, Out, generator=torch.Generator().manual_seed(2))
    o64 = copy.deepcopy(odec).double()
    er = enc.double().requires_grad_()
    torch.manual_seed(77)
    out_r = o64(er, T)
    (out_r * wgt.double()).sum().backward()
    ed = enc.cuda().requires_grad_()
    torch.manual_seed(77)
    out = pdec(ed, T)
    (out * wgt.cuda()).sum().backward()
    assert torch.equal(pdec.last_states[0].cpu(), o64.last_states[0].float())
    assert relerr(out, out_r) < 2e-5
    assert relerr(ed.grad, er.grad) < 1e-4
    pn = dict(pdec.named_parameters())
    for n, p in o64.named_parameters():
        e = relerr(pn[n].grad, p.grad)
        assert e < 1e-4, (n, e)


# --------------------------------------------------------------------------------------------------
# 6. whole model, every output / the loss / every parameter gradient against the fp64 oracle
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reserve', [16, 192], indirect=True, ids=_rid)
def test_cfg2_shape_batch8_f16x3_gradients(gpe, reserve):
    """cfg 2's shape (N = 2048, k = 16, H = 200, F = 150) at batch 8 in f16x3: R = 16 is what DistributedHotPath reserves when more
    than one rank trains (pinned edge kernels with 30 workgroups per XCD, a remainder in every cloud), R = 192 a 64-CU device (wide
    layer-2 kNN scan, RG = 1 recurrent plans, S = 4 weight-gradient splits)."""
    prev = gpe.set_math('f16x3')
    gate = gpe.set_f16x3_min_rows(0)
    try:
        nn_cfg = gpe.configs.lstm_model_config(k_neighbors=16)
        _whole_batch_gradient_parity(gpe, _synthetic_case(gpe, 'GarmentFullPattern3D', nn_cfg, 8, 2048, 31),
                                     'cfg2_b8_R%d' % reserve[0], 'f16x3')
    finally:
        gpe.set_f16x3_min_rows(gate)
        gpe.set_math(prev)


@pytest.mark.parametrize('reserve', [16], indirect=True, ids=_rid)
def test_cfg1_f32_gradients_under_a_reservation(gpe, reserve):
    """cfg 1 (N = 1024, k = 5, batch 8) in exact fp32 at the multi-rank default reservation."""
    prev = gpe.set_math('f32')
    try:
        nn_cfg = gpe.configs.lstm_model_config()
        _whole_batch_gradient_parity(gpe, _synthetic_case(gpe, 'GarmentFullPattern3D', nn_cfg, 8, 1024, 32),
                                     'cfg1_R%d' % reserve[0], 'f32')
    finally:
        gpe.set_math(prev)


# --------------------------------------------------------------------------------------------------
def test_world1_hot_path_keeps_the_callers_reservation(gpe):
    """DistributedHotPath with one rank and reserve_cus=None leaves a reservation set with set_reserved_cus() in force and reports it;
    an explicit reserve_cus still applies."""
    import torch.distributed as dist
    from gpe_amd import parallel
    assert not dist.is_initialized()
    model = torch.nn.Linear(8, 4).cuda()
    gpe.set_reserved_cus(16)
    try:
        ddp = parallel.DistributedHotPath(model, device_ids=[torch.device('cuda', 0)])
        assert ddp.world == 1
        assert gpe.get_reserved_cus() == 16 and ddp.reserved_cus == 16
        ddp = parallel.DistributedHotPath(model, device_ids=[torch.device('cuda', 0)], reserve_cus=4)
        assert gpe.get_reserved_cus() == 4 and ddp.reserved_cus == 4
    finally:
        gpe.set_reserved_cus(0)

"""-m gpu: the small operators (sparsemax and its loss, attention pooling, the segment pools, the PointNet++ sampling kernels, the
ground-truth matching kernels, a few flag / pitch arguments) at the edges where such kernels go wrong: block and slab boundaries,
strided views, padded pitches through the C ABI, exact ties, -inf, rows far from zero.

Every reference is plain fp64 torch / NumPy written here, or the oracle's definition (oracle/ref_path.py).  Tie rules are stated
explicitly: first maximum in point / row order for the pools, lower index for FPS, first `maxn` in index order with d^2 <= r^2 for
the ball query, first row-major minimum for the order match, first minimum shift for the origin match.

Worst figures observed on an MI355X are in each test's docstring (the integer work of sections D and E is exact); tolerances are
the sibling tests' bars in test_gpu_kernels.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


SENTINEL = -777.25


def _padded(t, ld, fill=SENTINEL):
    """[rows, ld] device buffer filled with the sentinel, t in its first columns."""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.cuda()


def _pad_untouched(buf, width, fill=SENTINEL):
    return bool((buf[:, width:] == fill).all().item())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ======================================================================================================================
# A. sparsemax forward / backward / loss
# ======================================================================================================================
SPX_ROWS = [1, 255, 256, 257, 700]          # the 256-thread block edge; the loss's fp64 partials with nblk = 1, 2 and 3
# rows drawn per (W, offset) before the boundary filter.  At offset 1e5 the fp32 scores are multiples of 2^-7, so a margin is a
# multiple of 2^-7 too and is EXACTLY 0 for 0.2% (W = 2) .. 0.8% (W = 32) of the rows (2e5-row sample); 20000 rows keep the
# sampling noise of that rate (sd 0.06%) away from the 1% assertion
SPX_POOL = 20000


def _sparsemax_rows(W, offset, seed):
    """randn*2 + offset rows (fp32) away from the support decision boundary: rows whose fp64 margin |1 + k z_(k) - cumsum_k| is
    within 1e-4 for some k are dropped (the comparison of supports is only meaningful away from it), at most 1% of them."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(SPX_POOL, W, generator=g) * 2 + offset).float()
    zs = torch.sort(z.double(), dim=-1, descending=True).values
    k = torch.arange(1, W + 1, dtype=torch.float64)
    margin = (1 + k * zs - zs.cumsum(-1)).abs().min(-1).values
    keep = margin > 1e-4
    assert (~keep).sum().item() <= SPX_POOL // 100, 'more than 1%% of the rows sit on the decision boundary (%d)' % (~keep).sum()
    return z[keep]


@pytest.mark.parametrize('offset', [0.0, 30.0, 1e3, 1e5])
@pytest.mark.parametrize('W', [1, 2, 5, 23, 31, 32])
def test_sparsemax_shifted_rows(gpe, W, offset):
    """Sparsemax is invariant to a constant added to a row; the kernels work on max-shifted scores, so the 2e-6 bar of
    test_sparsemax_fwd_bwd / test_sparsemax_loss and the identical support hold at every offset.
    MI355X, worst over all W, rows and offsets: output 6.0e-8, gradient 9.2e-8, loss 6.4e-8, loss gradient 1.5e-7, no support
    differs.  The parent's kernels (support rule and tau on the raw fp32 scores) fail it from offset 30 on: output error 2.6e-6
    at offset 30, 8.0e-5 at 1e3, 7.8e-3 at 1e5; loss error 2.0e-5 at 1e3."""
    from oracle import ref_path as O
    pool = _sparsemax_rows(W, offset, 100 * W + int(offset) % 97)
    g = torch.Generator().manual_seed(W)
    worst = dict(fwd=0.0, bwd=0.0, loss=0.0, lgrad=0.0)
    for rows in SPX_ROWS:
        z = pool[:rows].contiguous()
        gy = torch.randn(rows, W, generator=g)
        zr = z.double().requires_grad_()
        pr = O.Sparsemax(dim=1)(zr)
        pr.backward(gy.double())
        zd = z.cuda().requires_grad_()
        pd = gpe.ops.SparsemaxFn.apply(zd)
        pd.backward(gy.cuda())
        worst['fwd'] = max(worst['fwd'], relerr(pd, pr))
        worst['bwd'] = max(worst['bwd'], relerr(zd.grad, zr.grad))
        print('sparsemax W=%d offset=%g rows=%d fwd %.2e bwd %.2e' % (W, offset, rows, relerr(pd, pr), relerr(zd.grad, zr.grad)))
        assert relerr(pd, pr) < 2e-6, (rows, relerr(pd, pr))
        assert torch.equal(pd.cpu() > 0, pr > 0), rows                      # identical support
        assert relerr(zd.grad, zr.grad) < 2e-6, rows
        if offset <= 1e3:
            t = torch.randint(0, W, (rows,), generator=g)
            xr = z.double().requires_grad_()
            ref = O.SparsemaxLoss()(xr, t)
            (0.05 * ref).backward()
            xd = z.cuda().requires_grad_()
            out = gpe.ops.SparsemaxLossFn.apply(xd, t.cuda())
            (0.05 * out).backward()
            lerr = abs(out.item() - ref.item()) / max(1.0, abs(ref.item()))
            print('  loss err %.2e grad %.2e' % (lerr, relerr(xd.grad, xr.grad)))
            worst['loss'] = max(worst['loss'], lerr)
            worst['lgrad'] = max(worst['lgrad'], relerr(xd.grad, xr.grad))
            assert lerr < 2e-6, (rows, out.item(), ref.item())
            assert relerr(xd.grad, xr.grad) < 2e-6, rows
    print('sparsemax worst W=%d offset=%g %s' % (W, offset, worst))


@pytest.mark.parametrize('offset', [0.0, 1e3])
def test_sparsemax_structured_rows(gpe, offset):
    """Known answers: equal entries -> uniform 1/W; two equal maxima far above the rest -> 0.5 each; one entry more than 1 above
    the rest -> exact one-hot; scale 1e-3 -> full support; -inf beside finite entries -> exact 0 there, zero gradient, no NaN."""
    from oracle import ref_path as O
    W = 23
    g = torch.Generator().manual_seed(5)
    rows = []
    rows.append(torch.full((W,), 0.75))                                     # 0: all equal
    r = torch.randn(W, generator=g); r[3] = r[17] = 40.0; rows.append(r)    # 1: two exactly equal maxima
    r = torch.randn(W, generator=g).clamp(-3, 3); r[11] = 4.5; rows.append(r)   # 2: one entry > 1 above the rest
    rows.append(torch.randn(W, generator=g) * 1e-3)                         # 3: tiny scale, full support
    r = torch.randn(W, generator=g); r[::3] = -float('inf'); rows.append(r)     # 4: -inf entries beside finite ones
    r = torch.full((W,), -float('inf')); r[6] = 0.3; rows.append(r)             # 5: a single finite entry
    z = torch.stack(rows) + offset
    gy = torch.randn(len(rows), W, generator=g)
    zd = z.cuda().requires_grad_()
    pd = gpe.ops.SparsemaxFn.apply(zd)
    pd.backward(gy.cuda())
    p, gz = pd.detach().cpu(), zd.grad.cpu()
    assert torch.isfinite(p).all() and torch.isfinite(gz).all()
    assert relerr(p.sum(1), torch.ones(len(rows))) < 2e-6
    assert (p[0] - 1.0 / W).abs().max().item() < 2e-6
    assert p[1, 3].item() == 0.5 and p[1, 17].item() == 0.5 and p[1].sum().item() == 1.0
    onehot = torch.zeros(W); onehot[11] = 1.0
    assert torch.equal(p[2], onehot)
    assert (p[3] > 0).all()
    assert (p[4][::3] == 0).all() and (gz[4][::3] == 0).all()
    onehot = torch.zeros(W); onehot[6] = 1.0
    assert torch.equal(p[5], onehot) and (gz[5] == 0).all()
    # ... and all of it against the fp64 rule (the -inf rows included: the rule never selects them)
    zr = z.double().requires_grad_()
    pr = O.Sparsemax(dim=1)(zr)
    pr.backward(gy.double())
    assert relerr(p, pr) < 2e-6
    assert torch.equal(p > 0, pr > 0)
    assert relerr(gz, zr.grad) < 2e-6


@pytest.mark.parametrize('rows,W', [(257, 23), (3, 32), (256, 1)])
def test_sparsemax_row_pitch_through_the_abi(gpe, rows, W):
    """ldz = ldo = ldg = ldgz = W + 3 (the wrappers only pass W): the padding columns keep their sentinel."""
    from oracle import ref_path as O
    L = gpe._lib
    ld = W + 3
    g = torch.Generator().manual_seed(rows + W)
    z = torch.randn(rows, W, generator=g) * 2 + 30.0
    gy = torch.randn(rows, W, generator=g)
    t = torch.randint(0, W, (rows,), generator=g)
    zr = z.double().requires_grad_()
    pr = O.Sparsemax(dim=1)(zr)
    pr.backward(gy.double())
    zb, gb = _padded(z, ld), _padded(gy, ld)
    out = torch.full((rows, ld), SENTINEL, device='cuda')
    gz = torch.full((rows, ld), SENTINEL, device='cuda')
    L.call('gpe_sparsemax_fwd', zb, ld, rows, W, out, ld)
    L.call('gpe_sparsemax_bwd', out, ld, gb, ld, rows, W, gz, ld)
    assert _pad_untouched(out, W) and _pad_untouched(gz, W) and _pad_untouched(zb, W)
    assert relerr(out[:, :W], pr) < 2e-6
    assert torch.equal(out[:, :W].cpu() > 0, pr > 0)
    assert relerr(gz[:, :W], zr.grad) < 2e-6
    # the loss: ldx = ldg = W + 3
    xr = z.double().requires_grad_()
    ref = O.SparsemaxLoss()(xr, t)
    ref.backward()
    gx = torch.full((rows, ld), SENTINEL, device='cuda')
    part = torch.empty((rows + 255) // 256, device='cuda', dtype=torch.float64)
    loss = torch.empty(1, device='cuda')
    bad = torch.zeros(1, device='cuda', dtype=torch.int32)
    L.call('gpe_sparsemax_loss', zb, ld, t.to(torch.int32).cuda(), rows, W, gx, ld, part, loss, bad)
    assert bad.item() == 0 and _pad_untouched(gx, W)
    assert abs(loss.item() - ref.item()) < 2e-6 * max(1.0, abs(ref.item()))
    assert relerr(gx[:, :W], xr.grad) < 2e-6


def test_sparsemax_rejects_rows_wider_than_32(gpe):
    """W = 33 is refused by the entry points' argument checks (nothing is launched) and the wrappers raise."""
    z = torch.randn(4, 33).cuda()
    with pytest.raises(RuntimeError, match='gpe_sparsemax_fwd failed'):
        gpe.ops.SparsemaxFn.apply(z)
    with pytest.raises(RuntimeError, match='gpe_sparsemax_loss failed'):
        gpe.ops.SparsemaxLossFn.apply(z, torch.zeros(4, dtype=torch.long).cuda())
    torch.cuda.synchronize()


# ======================================================================================================================
# B. attention pooling
# ======================================================================================================================
AP_NS = [1, 63, 64, 65, 200]                # slab edges of the 64-row staging, a last slab of one row


def _attn_inputs(gpe, B, N, P, C, seed):
    """w as the model produces it (sparsemax of wide logits: exact zeros), panel 1 of cloud 0 zero at EVERY point; w and feat are
    column slices of wider tensors (stride(0) > width)."""
    g = torch.Generator().manual_seed(seed)
    w = gpe.ops.SparsemaxFn.apply((torch.randn(B * N, P, generator=g) * 3).cuda()).cpu()
    if P > 1:
        w[:N, 1] = 0.0
    f = torch.randn(B * N, C, generator=g)
    f[::7] = -f[::7].abs()                                   # -0.0 among the zero products
    gy = torch.randn(B * P, C, generator=g)
    wide_w = torch.full((B * N, P + 5), SENTINEL); wide_w[:, 2:2 + P] = w
    wide_f = torch.full((B * N, C + 3), SENTINEL); wide_f[:, 1:1 + C] = f
    return w, f, gy, wide_w, wide_f


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('P,C', [(1, 1), (5, 6), (23, 27), (23, 172), (23, 340), (32, 64)])
def test_attention_pool_edges(gpe, P, C, mode):
    """mean / max / add over N in {1, 63, 64, 65, 200} with strided sparsemax weights.  (23, 172) is the first width with work in a
    thread's second tile slot, (23, 340) the widest the entry point takes.
    max: the reference forms the products in fp32 (one multiply: bit-identical to the kernel's), takes the FIRST maximum in point
    order (np.argmax; -0.0 == +0.0) and routes g to that point alone, in fp64: pooled values bit-equal, gradients within 3e-6.
    MI355X, worst over all cases: mean / add output 3.3e-7 (fp32 sums inside a 64-row slab, fp64 across slabs), weight gradient
    8.1e-7, feature gradient 1.1e-7; max: bit-equal."""
    B = 2
    for N in AP_NS:
        w, f, gy, wide_w, wide_f = _attn_inputs(gpe, B, N, P, C, 7 * N + P + C + mode)
        wdv = wide_w.cuda()[:, 2:2 + P].requires_grad_()
        fdv = wide_f.cuda()[:, 1:1 + C].requires_grad_()
        assert wdv.stride(0) > P and fdv.stride(0) > C
        out = gpe.ops.AttentionPoolFn.apply(wdv, fdv, B, N, mode)
        gw, gf = torch.autograd.grad(out, (wdv, fdv), gy.cuda())
        if mode == 1:
            w3, f3, g3 = w.numpy().reshape(B, N, P), f.numpy().reshape(B, N, C), gy.double().numpy().reshape(B, P, C)
            prod = w3[:, :, :, None] * f3[:, :, None, :]                    # fp32 products [B, N, P, C]
            assert prod.dtype == np.float32
            arg = np.argmax(prod, axis=1)                                   # first maximum in point order
            ref = np.take_along_axis(prod, arg[:, None], axis=1)[:, 0]
            assert torch.equal(_bits(out.view(B, P, C)), torch.from_numpy(ref.copy()).view(torch.int32)), N
            gw_ref, gf_ref = np.zeros((B, N, P)), np.zeros((B, N, C))
            bi, pi, ci = np.meshgrid(np.arange(B), np.arange(P), np.arange(C), indexing='ij')
            np.add.at(gw_ref, (bi, arg, pi), g3 * f3.astype(np.float64)[bi, arg, ci])
            np.add.at(gf_ref, (bi, arg, ci), g3 * w3.astype(np.float64)[bi, arg, pi])
            if P > 1 and N > 1:                                             # the tie case was taken: a maximum of 0 with candidates
                zero_max = (ref[0, 1] == 0) & ((prod[0, :, 1, :] == 0).sum(0) > 1)
                assert zero_max.any()
                assert (arg[0, 1][(prod[0, :, 1, :] == 0).all(0)] == 0).all()
            e_w, e_f = relerr(gw, torch.from_numpy(gw_ref).view(B * N, P)), relerr(gf, torch.from_numpy(gf_ref).view(B * N, C))
        else:
            wr, fr = w.double().requires_grad_(), f.double().requires_grad_()
            ref = torch.einsum('bnp,bnc->bpc', wr.view(B, N, P), fr.view(B, N, C))
            if mode == 0:
                ref = ref / N
            ref.reshape(B * P, C).backward(gy.double())
            print('attn pool P=%d C=%d mode=%d N=%d fwd %.2e' % (P, C, mode, N, relerr(out, ref.reshape(B * P, C))))
            assert relerr(out, ref.reshape(B * P, C)) < 3e-6, N
            e_w, e_f = relerr(gw, wr.grad), relerr(gf, fr.grad)
        print('attn pool P=%d C=%d mode=%d N=%d gw %.2e gf %.2e' % (P, C, mode, N, e_w, e_f))
        assert e_w < 3e-6 and e_f < 3e-6, (N, e_w, e_f)


def test_attention_pool_rejects_too_many_tiles(gpe):
    """(P, C) = (23, 344): 6 x 86 = 516 tiles > 512, refused by the entry point's argument check."""
    B, N, P, C = 1, 8, 23, 344
    with pytest.raises(RuntimeError, match='gpe_attn_pool_fwd failed'):
        gpe.ops.AttentionPoolFn.apply(torch.rand(B * N, P).cuda(), torch.randn(B * N, C).cuda(), B, N, 0)
    torch.cuda.synchronize()


# ======================================================================================================================
# C. segment mean / max / add
# ======================================================================================================================
SEG_NS = [1, 3, 28, 29, 32, 33, 61, 100]    # around the mean's unrolled 32-row loop (n + 28 < N) and the 16-wave row striding


def _first_max(x3):
    """x3 [B, N, C] numpy -> (values, first arg-maximum in row order)."""
    arg = np.argmax(x3, axis=1)
    return np.take_along_axis(x3, arg[:, None], axis=1)[:, 0], arg


@pytest.mark.parametrize('C', [1, 64, 65, 255, 256, 257, 300])
def test_segment_pools_edges(gpe, C):
    """mean / add / max of a strided [B*N, C] view against fp64; max under ties: cloud 0 constant columns, cloud 1 the maximum at
    rows n and n + 16 (two waves), cloud 2 at n and n + 1, cloud 3 with -inf entries: the first row wins and takes the gradient.
    MI355X: max values and gradients exact, mean / add and their gradients 5.9e-8 at worst."""
    B = 4
    worst = 0.0
    for N in SEG_NS:
        g = torch.Generator().manual_seed(N * 1000 + C)
        x = torch.randn(B, N, C, generator=g)
        x[0] = torch.randn(1, C, generator=g)
        n0 = min(N - 1, 5)
        for b, step in ((1, 16), (2, 1)):
            top = x[b].max(0).values + 1.0
            x[b, n0] = top
            if n0 + step < N:
                x[b, n0 + step] = top
        if N > 1:
            x[3, 1::3] = -float('inf')
        gy = torch.randn(B, C, generator=g)
        wide = torch.full((B * N, C + 3), SENTINEL)
        wide[:, 2:2 + C] = x.view(B * N, C)
        xd = wide.cuda()[:, 2:2 + C].requires_grad_()
        assert xd.stride(0) > C
        # max: explicit first-maximum rule
        ymax = gpe.ops.segment_max(xd, B, N)
        gmax, = torch.autograd.grad(ymax, xd, gy.cuda())
        ref, arg = _first_max(x.numpy())
        assert torch.equal(_bits(ymax), torch.from_numpy(ref.copy()).view(torch.int32)), N
        gref = np.zeros((B, N, C), dtype=np.float32)
        bi, ci = np.meshgrid(np.arange(B), np.arange(C), indexing='ij')
        gref[bi, arg, ci] = gy.numpy()
        assert torch.equal(gmax.cpu(), torch.from_numpy(gref).view(B * N, C)), N
        if N > 1:
            assert (arg[0] == 0).all() and (arg[1] == n0).all() and (arg[2] == n0).all()
        # mean and add (clouds 0..2: finite)
        fin = 3 if N > 1 else B
        xf = wide.cuda()[:fin * N, 2:2 + C].requires_grad_()
        x64 = x[:fin].double()
        ymean = gpe.ops.segment_mean(xf, fin, N)
        gmean, = torch.autograd.grad(ymean, xf, gy[:fin].cuda())
        yadd = gpe.ops.segment_add(xf, fin, N)
        gadd, = torch.autograd.grad(yadd, xf, gy[:fin].cuda())
        errs = [relerr(ymean, x64.mean(1)), relerr(yadd, x64.sum(1)),
                relerr(gmean, (gy[:fin].double() / N)[:, None, :].expand(fin, N, C).reshape(fin * N, C)),
                relerr(gadd, gy[:fin].double()[:, None, :].expand(fin, N, C).reshape(fin * N, C))]
        worst = max(worst, max(errs))
        assert max(errs) < 1e-6, (N, errs)
    print('segment pools C=%d worst %.2e' % (C, worst))


@pytest.mark.parametrize('N,C', [(100, 65), (33, 300), (1, 1), (1000, 5)])
def test_segment_sums_accumulate_in_fp64(gpe, N, C):
    """x = 1e6 + randn: mean and add hold 1e-7 relative to the fp64 result; the fp32 rounding of the stored result alone is up to
    2^-24 = 6e-8, so the bar leaves the sum itself no room for more than a few fp32 roundings.  MI355X: 4.0e-8."""
    B = 3
    x = 1e6 + torch.randn(B * N, C, generator=torch.Generator().manual_seed(N + C))
    xd = x.cuda()
    e_mean = relerr(gpe.ops.segment_mean(xd, B, N), x.double().view(B, N, C).mean(1))
    e_add = relerr(gpe.ops.segment_add(xd, B, N), x.double().view(B, N, C).sum(1))
    print('segment fp64 accumulation N=%d C=%d mean %.2e add %.2e' % (N, C, e_mean, e_add))
    assert e_mean < 1e-7 and e_add < 1e-7


@pytest.mark.parametrize('N,C', [(29, 65), (1, 256), (100, 3)])
def test_segment_mean_bwd_accumulates(gpe, N, C):
    """gpe_segment_mean_bwd(accumulate = 1) through the ABI, padded pitches: gx += gy / N, padding untouched."""
    B = 3
    g = torch.Generator().manual_seed(N + C)
    gy = torch.randn(B, C, generator=g)
    pre = torch.randn(B * N, C, generator=g)
    gyb, gxb = _padded(gy, C + 1), _padded(pre, C + 2)
    gpe._lib.call('gpe_segment_mean_bwd', gyb, C + 1, B, N, C, gxb, C + 2, 1)
    ref = pre.double() + (gy.double() / N)[:, None, :].expand(B, N, C).reshape(B * N, C)
    assert relerr(gxb[:, :C], ref) < 1e-6
    assert _pad_untouched(gxb, C) and _pad_untouched(gyb, C)
    gpe._lib.call('gpe_segment_mean_bwd', gyb, C + 1, B, N, C, gxb, C + 2, 0)
    assert relerr(gxb[:, :C], ref - pre.double()) < 1e-6 and _pad_untouched(gxb, C)


# ======================================================================================================================
# D. PointNet++ kernels: bit-exact against the oracle's definitions
# ======================================================================================================================
FPS_SHAPES = [(2, 160, 40), (3, 1025, 257), (2, 1500, 375), (1, 16384, 32), (1, 70, 70)]
FPS_DATA = ['gauss', 'lattice', 'dup', 'same']


def _cloud(kind, B, N, C, g):
    if kind == 'gauss':
        return torch.randn(B * N, C, generator=g)
    if kind == 'lattice':                                   # exact distances, ties everywhere
        return torch.randint(0, 6, (B * N, C), generator=g).float()
    if kind == 'dup':                                       # every point once more, half a cloud further on
        h = (N + 1) // 2
        base = torch.randn(B, h, C, generator=g)
        return torch.cat([base, base], 1)[:, :N].reshape(B * N, C).contiguous()
    return torch.full((B * N, C), 0.3)


@pytest.mark.parametrize('data', FPS_DATA)
@pytest.mark.parametrize('B,N,M', FPS_SHAPES)
def test_fps_bit_exact(gpe, B, N, M, data):
    """gpe_fps vs O.fps with the same start points, up to the size limit N = 16384 (16 points per thread) and M = N; C in
    {2, 3, 8}, a padded pitch, start points random or None.  On the lattice / duplicated / identical clouds the running minimum
    ties inside a thread, across lanes and across waves: the lower index wins."""
    from oracle import ref_path as O
    si, di = FPS_SHAPES.index((B, N, M)), FPS_DATA.index(data)
    C = [3, 2, 8][(si + di) % 3]
    g = torch.Generator().manual_seed(N + 10 * di)
    pos = _cloud(data, B, N, C, g)
    start = torch.randint(0, N, (B,), generator=g) if (si + di) % 2 == 0 else None
    batch = torch.arange(B).repeat_interleave(N)
    ref = O.fps(pos, batch, (M - 0.5) / N, start=start if start is not None else torch.zeros(B, dtype=torch.long))
    ref = (ref.view(B, M) - (torch.arange(B) * N)[:, None]).to(torch.int32)
    pd = _padded(pos, C + 1)[:, :C] if di % 2 == 0 else pos.cuda()
    got = gpe.ops.fps(pd, B, N, M, None if start is None else start.to(torch.int32).cuda()).cpu()
    bad = (got != ref).sum().item()
    assert bad == 0, '%d / %d samples differ (C=%d, first at %s)' % (bad, B * M, C, (got != ref).nonzero()[:1].tolist())


def test_fps_start_is_clamped_and_oversize_is_rejected(gpe):
    from oracle import ref_path as O
    B, N, M, C = 3, 200, 20, 3
    pos = torch.randn(B * N, C, generator=torch.Generator().manual_seed(1))
    batch = torch.arange(B).repeat_interleave(N)
    start = torch.tensor([-5, N, 10 ** 6], dtype=torch.int32)
    ref = O.fps(pos, batch, (M - 0.5) / N, start=start.long().clamp(0, N - 1))
    got = gpe.ops.fps(pos.cuda(), B, N, M, start.cuda()).cpu()
    assert torch.equal(got.long() + (torch.arange(B) * N)[:, None], ref.view(B, M))
    with pytest.raises(RuntimeError, match='gpe_fps failed'):               # N = 16385: refused by the argument check
        gpe.ops.fps(torch.zeros(16385, 3).cuda(), 1, 16385, 4)
    torch.cuda.synchronize()


def _radius_check(gpe, pos, cidx, B, N, r, maxn):
    from oracle import ref_path as O
    M = cidx.shape[1]
    flat = (cidx.long() + (torch.arange(B) * N)[:, None]).view(-1)
    bx, by = torch.arange(B).repeat_interleave(N), torch.arange(B).repeat_interleave(M)
    row, col = O.radius(pos, pos[flat], r, bx, by, max_num_neighbors=maxn)
    nbr, cnt = gpe.ops.radius_neighbors(pos.cuda(), cidx.to(torch.int32).cuda(), B, N, r, maxn)
    nbr, cnt = nbr.cpu().long(), cnt.cpu().long()
    assert torch.equal(cnt, torch.bincount(row, minlength=B * M))
    got = torch.cat([nbr[s, :cnt[s]] + (s // M) * N for s in range(B * M)])       # the slots beyond cnt are unspecified
    assert torch.equal(got, col)
    return cnt


@pytest.mark.parametrize('maxn', [1, 25, 64, 70])
@pytest.mark.parametrize('N', [63, 64, 65, 160, 1500])
def test_radius_bit_exact(gpe, N, maxn):
    """gpe_radius vs O.radius: a 0.25 lattice with r = 0.5 (d^2 == r^2 exactly: `<=`), r = 0 (coincident points only), r large (the
    first maxn points: the cap is crossed inside a 64-lane chunk, or exactly at a chunk end for maxn = 64)."""
    B, M = 2, 12
    g = torch.Generator().manual_seed(N + maxn)
    pos = torch.randint(0, 7, (B * N, 3), generator=g).float() * 0.25
    cidx = torch.stack([torch.randperm(N, generator=g)[:M] for _ in range(B)])
    cidx[0, 0], cidx[1, 1] = 0, N - 1
    pos[1] = pos[0]                                                         # a coincident copy of centroid 0
    cnt = _radius_check(gpe, pos, cidx, B, N, 0.5, maxn)
    d2 = ((pos.view(B, N, 1, 3) - pos.view(B, N, 3)[torch.arange(B)[:, None], cidx].view(B, 1, M, 3)) ** 2).sum(-1)
    assert (d2 == 0.25).any()                                               # the boundary case is in the data
    cnt0 = _radius_check(gpe, pos, cidx, B, N, 0.0, maxn)
    assert (cnt0 >= 1).all() and (maxn == 1 or cnt0[0] > 1)                 # the centroid itself, and its coincident copies
    cntl = _radius_check(gpe, pos, cidx, B, N, 1e3, maxn)
    assert (cntl == min(N, maxn)).all()
    assert cnt.max().item() <= maxn


@pytest.mark.parametrize('Cx', [0, 5])
def test_pointconv_edge_list_and_messages(gpe, Cx):
    """gpe_pointconv_self_loops + gpe_ball_messages vs O.pointconv_edges with B = 3 (flat point s lies in another cloud than
    centroid s for s >= N): message rows bit-equal to x[src] | pos[src] - pos[centroid], seg_of_row equal; both outcomes occur
    (a dropped neighbour, none)."""
    from oracle import ref_path as O
    B, N, M, maxn, r = 3, 40, 20, 8, 0.9
    g = torch.Generator().manual_seed(11 + Cx)
    pos = torch.randn(B * N, 3, generator=g)
    x = torch.randn(B * N, Cx, generator=g) if Cx else None
    posd = pos.cuda()
    xd = _padded(x, Cx + 2)[:, :Cx] if Cx else None
    cidx = gpe.ops.fps(posd, B, N, M)                                       # start = point 0: centroid 0 IS flat point 0
    nbr, cnt = gpe.ops.radius_neighbors(posd, cidx, B, N, r, maxn)
    cnt2, drop = gpe.ops.pointconv_self_loops(nbr, cnt, B, N, M)
    off = torch.zeros(B * M + 1, dtype=torch.int64)
    off[1:] = cnt2.cpu().long().cumsum(0)
    E = int(off[-1])
    msg, seg = gpe.ops.ball_messages(posd, xd, cidx, nbr, off.cuda(), E, B, N, drop)
    nbr_c, cnt_c, cidx_c = nbr.cpu().long(), cnt.cpu().long(), cidx.cpu().long()
    src = torch.cat([nbr_c[s, :cnt_c[s]] + (s // M) * N for s in range(B * M)])
    dst = torch.arange(B * M).repeat_interleave(cnt_c)
    ei = O.pointconv_edges(torch.stack([src, dst]), B * N, B * M)
    order = torch.sort(ei[1], stable=True).indices                          # per centroid: kept neighbours in order, then the loop
    esrc, edst = ei[0][order], ei[1][order]
    assert E == ei.shape[1]
    assert torch.equal(seg.cpu().long(), edst)
    assert torch.equal(cnt2.cpu().long(), torch.bincount(edst, minlength=B * M))
    centre = (edst // M) * N + cidx_c.view(-1)[edst]
    ref = pos[esrc] - pos[centre]
    if Cx:
        ref = torch.cat([x[esrc], ref], 1)
    assert torch.equal(_bits(msg), _bits(ref))
    d = drop.cpu()
    assert (d >= 0).any() and (d < 0).any()
    assert (d[M:] < 0).all()                                                # flat point s < B*M lies in cloud b = s // M only for b = 0
    assert (esrc[edst >= M] < N).any()                                      # a loop source from another cloud than its centroid


@pytest.mark.parametrize('C', [1, 24, 65])
def test_ragged_max_first_row_wins(gpe, C):
    """RaggedMaxFn on a strided x with segment lengths 0, 1 and 40 and tied maxima (small integers): the FIRST row of a segment
    with the maximum gives the value and takes the whole gradient (torch's scatter_reduce('amax') would spread it over the ties:
    not the rule here); empty segments give 0 and no gradient."""
    lens = [0, 1, 40, 0, 3, 17, 1, 0]
    S, E = len(lens), sum(lens)
    off = torch.zeros(S + 1, dtype=torch.int64)
    off[1:] = torch.tensor(lens).cumsum(0)
    seg = torch.arange(S).repeat_interleave(torch.tensor(lens)).to(torch.int32)
    g = torch.Generator().manual_seed(C)
    x = torch.randint(-3, 3, (E, C), generator=g).float()
    gy = torch.randn(S, C, generator=g)
    xd = _padded(x, C + 3)[:, :C].requires_grad_()
    y = gpe.ops.RaggedMaxFn.apply(xd, off.cuda(), seg.cuda(), S)
    gx, = torch.autograd.grad(y, xd, gy.cuda())
    yref, gref = torch.zeros(S, C), torch.zeros(E, C)
    ties = 0
    for s in range(S):
        for c in range(C):
            rows = x[off[s]:off[s + 1], c]
            if rows.numel():
                best = 0
                for e in range(1, rows.numel()):
                    if rows[e] > rows[best]:
                        best = e
                ties += int((rows == rows[best]).sum() > 1)
                yref[s, c] = rows[best]
                gref[off[s] + best, c] = gy[s, c]
    assert ties > 0
    assert torch.equal(y.cpu(), yref)
    assert torch.equal(gx.cpu(), gref)


# ======================================================================================================================
# E. matching under exact ties
# ======================================================================================================================
def _grid(g, *shape):
    """multiples of 1/8 in [-4, 4]: every squared distance below is exact in fp32 in any summation order."""
    return torch.randint(-32, 33, shape, generator=g).float() / 8


def _greedy_order(pred, gt):
    """composed_loss.py:530-570 on one pattern: P rounds of `global minimum of the distance matrix, FIRST in row-major order on
    ties; perm[row] = col; strike the row and the column`."""
    P = pred.shape[0]
    d = np.sqrt(((pred.double().numpy()[:, None, :] - gt.double().numpy()[None, :, :]) ** 2).sum(-1))
    perm = np.full(P, -1, dtype=np.int64)
    for _ in range(P):
        e = int(np.argmin(d.reshape(-1)))                                   # first minimum, row-major
        row, col = divmod(e, P)
        perm[row] = col
        d[row, :] = np.inf
        d[:, col] = np.inf
    return torch.from_numpy(perm)


@pytest.mark.parametrize('D', [1, 7, 60])
@pytest.mark.parametrize('P', [1, 2, 23, 64])
def test_order_match_under_ties(gpe, P, D):
    """GT padded with 1, 5 and P - 1 identical all-zero panels, predictions with duplicated rows, a fully degenerate pattern: the
    permutation equals the reference loop's exactly and `fail` stays 0."""
    g = torch.Generator().manual_seed(P * 100 + D)
    zeros = sorted({min(z, P) for z in (1, 5, P - 1) if z > 0} or {1})
    B = len(zeros) + 1
    pred, gt = _grid(g, B, P, D), _grid(g, B, P, D)
    for b, z in enumerate(zeros):
        gt[b, P - z:] = 0.0                                                 # the padding panels of a real pattern
        if P >= 2:
            pred[b, P - 1] = pred[b, 0]                                     # duplicated prediction rows
        if P >= 4:
            pred[b, 2] = 0.0                                                # a predicted empty panel: ties with every padding panel
    pred[B - 1] = 1.5
    gt[B - 1] = 1.5                                                         # all entries equal: every distance 0
    perm, fail = gpe.ops.order_match(pred.cuda(), gt.cuda())
    ref = torch.stack([_greedy_order(pred[b], gt[b]) for b in range(B)])
    assert fail.item() == 0
    assert torch.equal(perm.cpu(), ref)
    assert torch.equal(ref[B - 1], torch.arange(P))                         # the degenerate pattern: identity
    assert torch.equal(torch.sort(perm.cpu(), 1).values, torch.arange(P).expand(B, P))


def test_order_match_rejects_more_than_64_panels(gpe):
    with pytest.raises(RuntimeError, match='gpe_order_match failed'):
        gpe.ops.order_match(torch.zeros(1, 65, 3).cuda(), torch.zeros(1, 65, 3).cuda())
    torch.cuda.synchronize()


@pytest.mark.parametrize('Lp', [14, 5])
def test_origin_match_known_answer(gpe, Lp):
    """The prediction is the GT loop rolled by a chosen r per panel (all edges distinct): lead == r and gt_out is that roll with the
    padding rows left in place.  n in {0, 1, 2, 3, L}, num_edges > L behaves as L, a panel of n identical edges gives lead 0.
    Outlines are the [..., :4] slice of a [B, P, L, 8] tensor (the model's own view)."""
    B, P = 2, 4
    n_list = [0, 1, 2, 3, Lp, Lp + 5, Lp, 4]
    r_list = [0, 0, 1, 2, Lp - 1, 3, 0, 0]
    g = torch.Generator().manual_seed(Lp)
    gt = _grid(g, B * P, Lp, 4)
    gt[:, :, 0] = torch.arange(Lp).float() / 8                              # distinct edges in every panel
    gt[7, :4] = gt[7, 0].clone()                                            # panel 7: its n = 4 edges identical
    full = _grid(g, B * P, Lp, 8)
    expect = gt.clone()
    for el, (n, r) in enumerate(zip(n_list, r_list)):
        n = min(n, Lp)
        for l in range(n):
            expect[el, l] = gt[el, (l + r) % n]
        full[el, :n, :4] = expect[el, :n]                                   # rows beyond n: unrelated values on both sides
    fd = full.view(B, P, Lp, 8).cuda()
    ne = torch.tensor(n_list, dtype=torch.int32).cuda()
    out, lead = gpe.ops.origin_match(fd[..., :4], gt.view(B, P, Lp, 4).cuda(), ne)
    assert lead.cpu().tolist() == r_list
    assert torch.equal(out.cpu().view(B * P, Lp, 4), expect)
    # ... and against the explicit rule on unrelated predictions: the FIRST shift with the smallest (exact) squared distance
    full2 = _grid(g, B * P, Lp, 8)
    full2[3] = 0.25                                                         # a constant prediction: shifts of a loop tie exactly
    out2, lead2 = gpe.ops.origin_match(full2.view(B, P, Lp, 8).cuda()[..., :4], gt.view(B, P, Lp, 4).cuda(), ne)
    for el, n in enumerate(n_list):
        n = min(n, Lp)
        best, best_r, best_gt = None, 0, gt[el]
        for r in range(max(n, 1)):
            rolled = gt[el].clone()
            for l in range(n):
                rolled[l] = gt[el, (l + r) % n]
            d = ((full2[el, :, :4].double() - rolled.double()) ** 2).sum().item()
            if best is None or d < best:
                best, best_r, best_gt = d, r, rolled
        assert lead2[el].item() == best_r, el
        assert torch.equal(out2.cpu().view(B * P, Lp, 4)[el], best_gt), el
    assert lead2[3].item() == 0


# ======================================================================================================================
# F. flags and pitches no wrapper passes
# ======================================================================================================================
@pytest.mark.parametrize('R', [1, 255, 256, 257])
def test_reduce_inner_accumulate_and_strides(gpe, R):
    """gpe_reduce_inner: y[r][c] (+)= sum_t x[r*so + t*si + c] with so > T*si > C, accumulate 0 and 1, ldy > C."""
    T, C = 5, 3
    si, so, ldy = C + 2, T * (C + 2) + 7, C + 1
    g = torch.Generator().manual_seed(R)
    xb = torch.randn(R * so, generator=g)
    x3 = torch.as_strided(xb, (R, T, C), (so, si, 1))
    ref = x3.double().sum(1)
    pre = torch.randn(R, C, generator=g)
    y = _padded(pre, ldy)
    xd = xb.cuda()
    gpe._lib.call('gpe_reduce_inner', xd, so, si, T, R, C, y, ldy, 1)
    assert relerr(y[:, :C], pre.double() + ref) < 1e-6 and _pad_untouched(y, C)
    gpe._lib.call('gpe_reduce_inner', xd, so, si, T, R, C, y, ldy, 0)
    assert relerr(y[:, :C], ref) < 1e-6 and _pad_untouched(y, C)


@pytest.mark.parametrize('rows', [1, 255, 256, 257])
def test_bn_apply_scaled_both_scales(gpe, rows):
    """gpe_bn_apply_scaled: y = s*(a*a_scale) + t*t_scale with both scales != 1, lda > C and ldy > C."""
    C = 7
    g = torch.Generator().manual_seed(rows)
    a = torch.randn(rows, C, generator=g)
    stats = torch.randn(4, C, generator=g)
    ab = _padded(a, C + 2)
    y = torch.full((rows, C + 3), SENTINEL, device='cuda')
    a_scale, t_scale = float(np.float32(0.2)), 5.0                          # the mean over k = 5 messages / the sum of 5
    gpe._lib.call('gpe_bn_apply_scaled', ab, C + 2, stats.cuda(), rows, C, a_scale, t_scale, y, C + 3)
    ref = stats[2].double() * (a.double() * a_scale) + stats[3].double() * t_scale
    assert relerr(y[:, :C], ref) < 1e-6 and _pad_untouched(y, C)


@pytest.mark.parametrize('H,C', [(30, 3), (30, 150), (256, 3), (256, 150)])
def test_w1_split_and_grad_are_adjoint(gpe, H, C):
    """gpe_w1_split (W1 [H][2C] -> Wpq [2H][C]) and gpe_w1_grad_from_pq (dWpq -> dW1) are a linear map and its transpose:
    <split(W), G> == <W, grad(G)> in fp64 to 1e-6 relative; padded pitches on all four matrices.  MI355X: 3.7e-7 at worst
    (H = 256, C = 150, where the inner product of 76800 terms cancels to -15.4)."""
    g = torch.Generator().manual_seed(H + C)
    W = torch.randn(H, 2 * C, generator=g)
    b1 = torch.randn(H, generator=g)
    G = torch.randn(2 * H, C, generator=g)
    Wb, Gb = _padded(W, 2 * C + 3), _padded(G, C + 1)
    wpq = torch.full((2 * H, C + 2), SENTINEL, device='cuda')
    bias = torch.full((2 * H,), SENTINEL, device='cuda')
    dw1 = torch.full((H, 2 * C + 5), SENTINEL, device='cuda')
    gpe._lib.call('gpe_w1_split', Wb, 2 * C + 3, b1.cuda(), H, C, wpq, C + 2, bias)
    gpe._lib.call('gpe_w1_grad_from_pq', Gb, C + 1, H, C, dw1, 2 * C + 5)
    assert _pad_untouched(wpq, C) and _pad_untouched(dw1, 2 * C)
    assert torch.equal(bias.cpu(), torch.cat([b1, torch.zeros(H)]))
    S, T = wpq[:, :C].cpu(), dw1[:, :2 * C].cpu()
    assert torch.equal(S, torch.cat([W[:, :C] - W[:, C:], W[:, C:]]))       # one fp32 subtraction: exact
    lhs, rhs = (S.double() * G.double()).sum().item(), (W.double() * T.double()).sum().item()
    print('w1 adjoint H=%d C=%d <S,G> %.6f rel %.2e' % (H, C, lhs, abs(lhs - rhs) / abs(lhs)))
    assert abs(lhs - rhs) < 1e-6 * abs(lhs)

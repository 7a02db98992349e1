"""Test infrastructure: the six loss-side entry points (csrc/gpe_loss.hip: gpe_pattern_loss_fwd / _bwd; csrc/gpe_stitch.hip:
gpe_stitch_loss_fwd / _bwd, gpe_stitch_renumber, gpe_panel_shift) restated one by one.

For every entry point: a case builder (`build(kernel, spec)`: the exact host buffers of one call; predictions are views into
larger tensors, everything the kernel must not read is NaN, ground-truth stitch entries past nums[b] are out-of-range ids, outputs
are a few elements longer than needed and pre-filled with a sentinel), an fp64 reference (`expected(case)`: the oracle's own
PatternStitchLoss / PanelLoopLoss / _stitch_after_permute / _gt_stitches_shift / _per_panel_shift, torch's fp64 mse_loss and
binary_cross_entropy_with_logits under autograd, composed as (similarity + negative) + sup_w * supervised + free), a closed-form
restatement of the same (`restate_*`, which tests/test_loss_host.py holds against the oracle at 1e-12 and which carries the
`variant=` switches), a checker (`check(case, kernel, got, variant=None)`) and an emulation (`emulate`: the reference rounded
once to fp32).  `VARIANTS` lists plausible mistakes applied to the REFERENCE; the host test asserts each is rejected by a case.
No GPU and no gpe_amd here.  `abi_args(case, kernel, dev)` lays out the C-ABI argument list from a {name: device tensor} map.

Bars (the project's own for these kernels): every out5 slot within 2e-6 max(1, |ref|); every gradient tensor relerr < 2e-6
(max |diff| / max |ref|), g_tags and g_mask separately, and exactly 0 wherever the reference is exactly 0; integer and copied
outputs exact.

Conventions where the kernels differ from the reference on purpose (also in include/gpe_hip.h):
  * gap exactly 0 (margin - d == 0): the pair is inactive, value unchanged, gradient 0.  The reference's autograd sends the
    full gradient there under HardNet (Python's max(t, 0) returns t) and half of it in the all-pairs term (torch.max(a, zeros)
    splits at equality).  `restate_stitch(conv='reference')` reproduces the reference, conv='kernel' the kernels; they differ in
    the case `grid-gap0` only, and `expected` uses conv='kernel' there.
  * n_b = 0: that pattern's similarity and the total are NaN as in the reference, every gradient is finite, that pattern's
    gradients are 0 apart from the supervised and free terms.
  * nums[b] outside [0, S] is clamped (the reference is given the clamped count); edge ids outside [0, P L) are clamped in the
    loss kernels (no case feeds one to the reference: entries past nums[b] are never read).
  * num_edges > L acts as L, negative as 0.
  * renumber: the LAST slot with perm[b][r] == panel wins, none gives -1, and the origin step floor-divides; a negative flat
    panel number reads lead[0] (the oracle, which would wrap to the last element, is handed a copy of element 0 there).

Branch -> case (ids as pytest prints them):
  block-stride loops below one wave / at 256 / wrapping     stitch 1-1-3-1-1-*, 2-23-14-3-24-* (P L = 322, P L D = 966);
                                                            pattern 1-1-3-4-3-*, 1-16-4-4-3-* (P L 4 = 256), 2-130-3-4-3-* (P 2, P R > 256)
  n_b = 0, and ntot over all patterns                       stitch 3-2-4-3-3-f* (nums 3, 2, 0)
  n_b = 1 (HardNet minimum +inf)                            stitch 1-1-3-1-1-f3, 2-5-30-8-64-f* (nums 64, 1)
  n_b = S = 64, D = 8                                       stitch 2-5-30-8-64-f*
  nums outside [0, S]                                       stitch 2-2-4-3-3-f* (nums S + 5, -2)
  HardNet ties, 2 and 3 members, distinct edges             grid-tie2-f3, grid-tie3-f3
  tie through an edge on two / three stitches               grid-dup2-f3 / f11, grid-dup3-f3 / f11
  duplicate with the supervised initialisation              grid-dup2-f9 / f11, grid-dup3-f9 / f11
  all tags identical                                        grid-same-f1 / f3
  gap exactly 0                                             grid-gap0-f1 / f3
  every pair beyond the margin                              grid-far-f1 / f3
  edge ids outside [0, P L) among the valid entries         grid-clamp-f1 / f3 (ids -3 and P L + 2 act as 0 and P L - 1)
  all 16 flag values                                        stitch 3-2-4-3-3-f0 .. f15; pattern 3-2-4-1-5-f0 .. f15 (f2 = the loop-only call)
  g_mask NULL with g_tags / the reverse; g_rot / g_tr NULL  every case whose id ends in -gn (only the required gradients are passed)
  strides                                                   id part own / dense / corner
  gscale NULL, 0.75, -2                                     id part gsN / gs0.75 / gs-2
  num_edges -1, 0, 2, 3, L, L + 5; pad (0.375, -1.25)       every pattern case cycles through the six values; id part pad
  renumber: last slot wins, -1, floor division              renumber *-rep; tail copied: every renumber case; perm / lead NULL: -p0 / -l0
  renumber past the 128 threads                             renumber 2-64-23-14-*, 2-70-23-14-*
  panel shift n < 3, lead 0, padding rows, n > L, D 1 / 3   every shift case cycles num_edges 0, 2, 3, L, L + 5 and lead 0, 1, n - 1"""
import types

import numpy as np
import torch

F64 = torch.float64
SENTINEL = -777.25
ISENTINEL = -7777777
TAIL = 5                        # every output is allocated this much longer than its documented extent
VALUE_BAR = 2e-6
GRAD_BAR = 2e-6
MARGIN = 0.3
SUP_W = 0.1
KERNELS = ('stitch_loss_fwd', 'stitch_loss_bwd', 'pattern_loss_fwd', 'pattern_loss_bwd', 'stitch_renumber', 'panel_shift')
LAYOUTS = ('own', 'dense', 'corner')
GSCALES = (None, 0.75, -2.0)


class Case(types.SimpleNamespace):
    """group, id, p (scalars), inp {name: array}, view {name: (base name, index)}, out0 {kernel: {name: pre-filled array}}"""

    def v(self, name):
        base, idx = self.view[name]
        return self.inp[base][idx]

    def v64(self, name):
        return self.v(name).astype(np.float64)


def f32r(x):
    """x rounded to fp32, as fp64 (what a float argument of the C ABI becomes)"""
    return float(np.float32(x))


def _out(n, dtype=np.float32):
    return np.full(n + TAIL, ISENTINEL if np.issubdtype(dtype, np.integer) else SENTINEL, dtype=dtype)


def _strides(a):
    assert all(s % a.itemsize == 0 for s in a.strides)
    return [s // a.itemsize for s in a.strides]


# ----------------------------------------------------------------------------------------------------------------------
# stitch loss: cases
# ----------------------------------------------------------------------------------------------------------------------
STITCH_SHAPES = [(1, 1, 3, 1, 1, (1,)), (3, 2, 4, 3, 3, (3, 2, 0)), (2, 23, 14, 3, 24, (24, 7)), (2, 5, 30, 8, 64, (64, 1)),
                 (2, 2, 4, 3, 3, (8, -2))]
GRID_KINDS = {'dup2': (1, 3, 9, 11), 'dup3': (1, 3, 9, 11), 'tie2': (3,), 'tie3': (3,), 'same': (1, 3), 'gap0': (1, 3), 'far': (1, 3),
              'clamp': (1, 3)}


def _stitch_specs():
    specs, i = [], 0
    for si, shape in enumerate(STITCH_SHAPES):
        for flags in (range(16) if si == 1 else (15, 13, 7, 5, 3, 1)):
            specs.append(('rand', shape, flags, LAYOUTS[i % 3], GSCALES[(i // 3) % 3], i % 2 == 0))
            i += 1
    for kind, fl in GRID_KINDS.items():
        for flags in fl:
            specs.append((kind, None, flags, LAYOUTS[i % 3], GSCALES[(i // 3) % 3], i % 2 == 0))
            i += 1
    return specs


def _panel_buffers(rng, B, P, L, D, layout):
    """-> inp, view for outlines (b,p,l,c<4), tags (b,p,l,d<D), logit (b,p,l): NaN wherever no view points"""
    W = 4 + D + 1
    inp, view = {}, {}
    box = (slice(None), slice(0, P), slice(0, L))
    if layout == 'dense':
        inp['ol_buf'] = np.full((B, P, L, 4), np.nan, np.float32)
        inp['tags_buf'] = np.full((B, P, L, max(D, 1)), np.nan, np.float32)
        inp['logit_buf'] = np.full((B, P, L), np.nan, np.float32)
        view.update(ol=('ol_buf', box), tags=('tags_buf', box + (slice(0, D),)), logit=('logit_buf', box))
    else:
        shape = (B, P, L, W) if layout == 'own' else (B, P + 1, L + 2, W)
        inp['panels'] = np.full(shape, np.nan, np.float32)
        view.update(ol=('panels', box + (slice(0, 4),)), tags=('panels', box + (slice(4, 4 + D),)), logit=('panels', box + (4 + D,)))
    return inp, view


def _conditions(tags64, st, nums, margin, grid):
    """the input conditions of the issue for one case, in fp64: every non-brother pair has |margin - d| >= 2^-16 max(1, d) and the
    second-smallest distance of every tag exceeds the smallest by as much; on the grid the exact cases (0) are allowed as well"""
    for b, n in enumerate(nums):
        if n == 0:
            continue
        T = np.concatenate([tags64[b][st[b, 0, :n]], tags64[b][st[b, 1, :n]]])
        d = ((T[:, None, :] - T[None, :, :]) ** 2).sum(-1)
        idx = np.arange(2 * n)
        other = np.ones((2 * n, 2 * n), bool)
        other[idx, idx] = False
        other[idx, (idx + n) % (2 * n)] = False
        for i in idx:
            di = np.sort(d[i][other[i]])
            gap = np.abs(margin - di)
            ok = gap >= 2.0 ** -16 * np.maximum(1, di)
            if grid:
                ok |= gap == 0
            if not ok.all():
                return False
            if len(di) > 1:
                sep = di[1] - di[0]
                if not (sep >= 2.0 ** -16 * max(1, di[1]) or (grid and sep == 0)):
                    return False
    return True


def _grid_pattern(kind):
    """-> tag positions of the 8 edges of pattern 0 (multiples of 1/8, D = 2), its stitches [(left, right)], margin"""
    e = np.zeros((8, 2))
    if kind in ('dup2', 'dup3', 'clamp'):
        # edge 0 sits on two (three) stitches: its tags are identical, so edge 3 -- closest to edge 0 -- has a tied minimum
        e[:] = [(0, 0), (-2, 0), (0, -2), (1, 1), (5, 4), (-1, 3), (5, -3), (-5, -4)]
        st = [(0, 1), (0, 2), (3, 4)] + ([(5, 0)] if kind == 'dup3' else [])
        if kind == 'clamp':                 # ids below 0 and past P L among the valid entries: the kernels read edges 0 and 7
            st = [(0, 1), (-3, 2), (3, 8 + 2)]
    elif kind in ('tie2', 'tie3'):
        # edge 0 has two (three) distinct edges of other stitches at the same distance 1/64
        e[:] = [(0, 0), (1, 0), (0, 1), (-1, 0), (6, 6), (7, -5), (-6, 7), (-7, -6)]
        st = [(0, 4), (1, 5), (2, 6)] + ([(3, 7)] if kind == 'tie3' else [])
    elif kind == 'same':
        e[:] = (1, 2)
        st = [(0, 1), (2, 3), (4, 5)]
    elif kind == 'gap0':
        # d(edge 0, edge 1) = 32/64 = the margin exactly; every other pair of different stitches is far beyond it
        e[:] = [(0, 0), (4, 4), (-9, 0), (14, 4), (0, 20), (20, 20), (-20, 20), (20, -20)]
        st = [(0, 2), (1, 3)]
    else:                                   # far: spacing 1 against a margin of 1/2
        e[:] = [(8 * i, 0) for i in range(8)]
        st = [(0, 1), (2, 3), (4, 5)]
    return e / 8.0, st, 0.5


def build_stitch(spec):
    kind, shape, flags, layout, gscale, gnull = spec
    grid = kind != 'rand'
    if grid:
        B, P, L, D, S = 2, 2, 4, 2, 4
        pos, pairs, margin = _grid_pattern(kind)
        nums_in = (len(pairs), 1)
    else:
        B, P, L, D, S, nums_in = shape
        margin = MARGIN
    nums = [min(max(n, 0), S) for n in nums_in]
    PL = P * L
    margin = f32r(margin)
    seed = 0
    while True:                              # seeds are tried until the input conditions hold: no case is dropped
        rng = np.random.default_rng([1000 + seed, B, P, L, D, S, flags, len(kind)])
        if grid:
            tags = rng.integers(-32, 33, (B, PL, D)).astype(np.float64) / 8
            tags[0] = pos
            tags[1, :2] = [(3, 0), (3, 0.5)]
            st = np.zeros((B, 2, S), np.int64)
            st[0, :, :len(pairs)] = np.array(pairs).T
            st[1, :, 0] = (0, 1)
        else:
            tags = (rng.standard_normal((B, PL, D)) * 0.3 / np.sqrt(D)).astype(np.float32).astype(np.float64)
            st = np.zeros((B, 2, S), np.int64)
            for b, n in enumerate(nums):
                ids = rng.permutation(PL)[:2 * n]
                st[b, 0, :n], st[b, 1, :n] = ids[:n], ids[n:]
        if not (flags & 1) or _conditions(tags, np.clip(st, 0, PL - 1), nums, margin, grid):
            break
        seed += 1
        assert seed < 200
    inp, view = _panel_buffers(rng, B, P, L, D, layout)
    case = Case(group='stitch', inp=inp, view=view, grid=grid, kind=kind, seed=seed)
    if flags & 9:
        case.v('tags')[...] = tags.reshape(B, P, L, D)
    if flags & 4:
        case.v('logit')[...] = rng.standard_normal((B, P, L)) * 3
    stitches = st.copy()
    st = np.clip(st, 0, PL - 1)              # what the loss kernels make of an id outside [0, P L), and what the reference is given
    for b, n in enumerate(nums):             # entries the kernels must never follow (and the renumbering must copy)
        stitches[b, 0, n:] = 10 ** 12 + 7
        stitches[b, 1, n:] = -(10 ** 6) - 3
    inp['stitches'], inp['nums'] = stitches, np.array(nums_in, np.int64)
    inp['gt_mask'] = (rng.random((B, P, L)) < 0.5).astype(np.float32) if flags & 4 else np.full((B, P, L), np.nan, np.float32)
    inp['gt_tags'] = (rng.integers(-8, 9, (B, P, L, D)) / 8).astype(np.float32) if flags & 8 else np.full((B, P, L, D), np.nan, np.float32)
    if gscale is not None:
        inp['gscale'] = np.array([gscale], np.float32)
    need_t, need_m = bool(flags & 9), bool(flags & 4)
    case.p = dict(B=B, P=P, L=L, D=D, S=S, flags=flags, margin=margin, sup_w=f32r(SUP_W), gscale=gscale, layout=layout,
                  nums=nums, st_clean=st, g_tags=need_t or not gnull, g_mask=need_m or not gnull)
    case.out0 = {'stitch_loss_fwd': {'part': _out(B * 6, np.float64), 'out5': _out(5)}, 'stitch_loss_bwd': {}}
    if case.p['g_tags']:
        case.out0['stitch_loss_bwd']['g_tags'] = _out(B * PL * D)
    if case.p['g_mask']:
        case.out0['stitch_loss_bwd']['g_mask'] = _out(B * PL)
    head = 'grid-' + kind if grid else '-'.join(str(v) for v in shape[:5])
    case.id = '%s-f%d-%s-gs%s%s' % (head, flags, layout, 'N' if gscale is None else '%g' % gscale, '-gn' if gnull else '')
    return case


# ----------------------------------------------------------------------------------------------------------------------
# stitch loss: the closed-form restatement (variants live here) and the oracle reference
# ----------------------------------------------------------------------------------------------------------------------
def restate_stitch(case, conv='kernel', variant=None):
    """-> dict(out5 [5], sim_b [B], g_tags [B,PL,D], g_mask [B,PL]) in fp64.  The stitch part is differentiated with respect to
    the staged copies of the tags (one per stitch side) and scattered by hand, as the kernel does."""
    p = case.p
    B, P, L, D, S, flags = p['B'], p['P'], p['L'], p['D'], p['S'], p['flags']
    PL, nums, st, margin = P * L, p['nums'], p['st_clean'], p['margin']
    gs = 1.0 if p['gscale'] is None else p['gscale']
    sup_w = 1.0 if variant == 'sup_w_dropped' else p['sup_w']
    dense = variant == 'dense_layout'
    tags = _read(case, 'tags', dense).reshape(B, PL, D) if flags & 9 else None
    g_tags, g_mask = np.zeros((B, PL, max(D, 1))), np.zeros((B, PL))
    sim = neg = sup = free = 0.0
    sim_b = np.zeros(B)
    if flags & 8:
        diff = tags - case.inp['gt_tags'].astype(np.float64).reshape(B, PL, D)
        cnt = B * PL if variant == 'sup_count' else B * PL * D
        sup = (diff ** 2).sum() / cnt
        g_tags += (1.0 if variant == 'gscale_dropped_sup' else gs) * sup_w * 2 * diff / cnt
    if flags & 4:
        x, y = _read(case, 'logit', dense).reshape(B, PL), case.inp['gt_mask'].astype(np.float64).reshape(B, PL)
        cnt = PL if variant == 'bce_count' else B * PL
        free = (np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).sum() / cnt
        g_mask += (1.0 if variant == 'gscale_dropped_free' else gs) * (1 / (1 + np.exp(-x)) - y) / cnt
    if flags & 1:
        hard = bool(flags & 2)
        ntot = 2 * S * B if variant == 'ntot_2S' else 2 * sum(nums)
        leaves, per_tag, sim_t = [], [], torch.zeros((), dtype=F64)
        for b, n in enumerate(nums):
            edges = np.concatenate([st[b, 0, :n], st[b, 1, :n]])
            T = torch.tensor(tags[b][edges], dtype=F64).reshape(2 * n, D).requires_grad_()
            leaves.append((b, edges, T))
            den = {'sim_div_S': S, 'sim_div_total': sum(nums)}.get(variant, n)
            s_b = ((T[:n] - T[n:]) ** 2).sum() / torch.tensor(float(den), dtype=F64)
            sim_b[b] = s_b.item()
            sim_t = sim_t + s_b
            if n == 0:
                continue
            Tj = T.detach() if variant == 'other_end_no_grad' else T
            d = ((T[:, None, :] - Tj[None, :, :]) ** 2).sum(-1)
            idx = torch.arange(2 * n)
            excl = torch.zeros(2 * n, 2 * n, dtype=torch.bool)
            if variant != 'self_included':
                excl[idx, idx] = True
            if variant != 'brother_included':
                excl[idx, (idx + n) % (2 * n)] = True
            if hard:
                dm = d.masked_fill(excl, float('inf'))
                m = dm.min(dim=1).values if variant == 'first_tied_minimum' else torch.amin(dm, dim=1)
                gap = margin - m
                term = torch.where(gap > 0 if conv == 'kernel' else gap >= 0, gap, torch.zeros_like(gap))
            else:
                gap = (margin - d).masked_fill(excl, 0.0)
                act = torch.where(gap > 0, gap, torch.zeros_like(gap)) if conv == 'kernel' else torch.max(gap, torch.zeros_like(gap))
                term = act.sum(1) / (n if variant == 'pairs_div_n' else 2 * n)
            per_tag.append(term.sum())
        sim_t = sim_t / B
        neg_t = sum(per_tag) / ntot if ntot else torch.tensor(float('nan'), dtype=F64)
        sim, neg = sim_t.item(), float(torch.as_tensor(neg_t).detach())
        # the NaN of an empty pattern is a value only: its (empty) leaf takes no gradient and the others are not touched by it
        obj = sim_t + neg_t
        if any(len(e) for _, e, _ in leaves):
            obj.backward()
        gss = 1.0 if variant == 'gscale_dropped_stitch' else gs
        for b, edges, T in leaves:
            if not len(edges):
                continue
            G = T.grad.numpy() if T.grad is not None else np.zeros((len(edges), D))
            if variant == 'dup_overwritten':
                init = g_tags[b].copy()
                for t, e in enumerate(edges):
                    g_tags[b, e] = init[e] + gss * G[t]
            elif variant == 'sup_lost_under_scatter':
                g_tags[b, edges] = 0
                np.add.at(g_tags[b], edges, gss * G)
            else:
                np.add.at(g_tags[b], edges, gss * G)
    total = 0.0
    if flags & 1:
        total = total + (sim + neg)
    if flags & 8:
        total = total + sup_w * sup
    if flags & 4:
        total = total + free
    out5 = np.array([total, sim if flags & 1 else 0, neg if flags & 1 else 0, sup if flags & 8 else 0, free if flags & 4 else 0], np.float64)
    return dict(out5=out5, sim_b=sim_b, g_tags=g_tags[:, :, :D], g_mask=g_mask)


def _read(case, name, dense=False):
    """the fp64 values of a prediction view; dense=True reads the same base pointer as if the pitches were the dense ones"""
    v = case.v(name)
    if not dense:
        return v.astype(np.float64)
    base, idx = case.view[name]
    buf = case.inp[base]
    off = (v.__array_interface__['data'][0] - buf.__array_interface__['data'][0]) // buf.itemsize
    st = _strides(v)
    inner = st[-2] if v.ndim >= 3 and name != 'logit' else st[-1]       # the pitch of the innermost index that is passed
    if name in ('rot', 'tr'):
        Bp, C = v.shape
        ix = off + np.arange(Bp)[:, None] * C + np.arange(C)
    elif name == 'logit':
        B, P, L = v.shape
        sl = st[2]
        ix = off + (np.arange(B)[:, None, None] * P * L + np.arange(P)[None, :, None] * L + np.arange(L)) * sl
    else:
        B, P, L, C = v.shape
        ix = off + (np.arange(B)[:, None, None, None] * P * L + np.arange(P)[None, :, None, None] * L
                    + np.arange(L)[None, None, :, None]) * inner + np.arange(C)
    flat = buf.reshape(-1)
    return flat[np.minimum(ix, flat.size - 1)].astype(np.float64)


def oracle_stitch(case):
    """values and gradients from the oracle's PatternStitchLoss and torch's fp64 mse_loss / binary_cross_entropy_with_logits"""
    from oracle import ref_path as O
    p = case.p
    B, P, L, D, flags = p['B'], p['P'], p['L'], p['D'], p['flags']
    gs = 1.0 if p['gscale'] is None else p['gscale']
    tags = torch.tensor(case.v64('tags'), dtype=F64).requires_grad_() if flags & 9 else None
    logit = torch.tensor(case.v64('logit'), dtype=F64).requires_grad_() if flags & 4 else None
    out5 = np.zeros(5)
    extra = 0.
    sim_b = np.zeros(B)
    if flags & 1:
        loss = O.PatternStitchLoss(p['margin'], use_hardnet=bool(flags & 2))
        nums = torch.tensor(p['nums'])
        st, parts = loss(tags, torch.tensor(p['st_clean']), nums)
        out5[1], out5[2] = (float(torch.as_tensor(parts[k]).detach()) for k in ('stitch_similarity_loss', 'stitch_neg_loss'))
        extra = extra + st
        flat = tags.detach().reshape(B, P * L, D)
        for b, n in enumerate(p['nums']):
            sq = ((flat[b][p['st_clean'][b, 0, :n]] - flat[b][p['st_clean'][b, 1, :n]]) ** 2).sum()
            sim_b[b] = float(sq / torch.tensor(float(n), dtype=F64))
    if flags & 8:
        sup = torch.nn.functional.mse_loss(tags, torch.tensor(case.inp['gt_tags'], dtype=F64))
        out5[3] = sup.item()
        extra = extra + p['sup_w'] * sup
    if flags & 4:
        free = torch.nn.functional.binary_cross_entropy_with_logits(logit, torch.tensor(case.inp['gt_mask'], dtype=F64))
        out5[4] = free.item()
        extra = extra + free
    out5[0] = float(torch.as_tensor(extra).detach())
    if torch.is_tensor(extra) and extra.requires_grad:
        (extra * gs).backward()
    g = lambda t, shape: t.grad.numpy().reshape(shape) if t is not None and t.grad is not None else np.zeros(shape)
    return dict(out5=out5, sim_b=sim_b, g_tags=g(tags, (B, P * L, D)), g_mask=g(logit, (B, P * L)))


# ----------------------------------------------------------------------------------------------------------------------
# pattern loss
# ----------------------------------------------------------------------------------------------------------------------
PATTERN_SHAPES = [(1, 1, 3, 4, 3), (3, 2, 4, 1, 5), (2, 23, 14, 4, 3), (2, 130, 3, 4, 3), (1, 16, 4, 4, 3)]


def _pattern_specs():
    specs, i = [], 0
    for si, shape in enumerate(PATTERN_SHAPES):
        for flags in (range(16) if si == 1 else (15, 2, 13)):
            specs.append((shape, flags, LAYOUTS[i % 3], GSCALES[(i // 3) % 3], (0.0, 0.0) if i % 2 else (0.375, -1.25),
                          0.7 if (i // 2) % 2 else 1.0, i % 4 == 1, i))
            i += 1
    return specs


def build_pattern(spec):
    (B, P, L, R, T), flags, layout, gscale, pad, loop_w, gnull, i = spec
    rng = np.random.default_rng([2000, B, P, L, R, T, flags])
    inp, view = _panel_buffers(rng, B, P, L, 3, layout)
    if layout == 'dense':
        inp['rot_buf'], inp['tr_buf'] = np.full((B * P, R), np.nan, np.float32), np.full((B * P, T), np.nan, np.float32)
        view.update(rot=('rot_buf', (slice(None), slice(0, R))), tr=('tr_buf', (slice(None), slice(0, T))))
    else:
        lead = 0 if layout == 'own' else 2
        inp['place'] = np.full((B * P, max(7, R + T) + (0 if layout == 'own' else 3)), np.nan, np.float32)
        view.update(rot=('place', (slice(None), slice(lead, lead + R))), tr=('place', (slice(None), slice(lead + R, lead + R + T))))
    case = Case(group='pattern', inp=inp, view=view)
    if flags & 3:
        case.v('ol')[...] = rng.standard_normal((B, P, L, 4))
    if flags & 4:
        case.v('rot')[...] = rng.standard_normal((B * P, R))
    if flags & 8:
        case.v('tr')[...] = rng.standard_normal((B * P, T))
    nan = lambda *s: np.full(s, np.nan, np.float32)
    inp['gt_ol'] = rng.standard_normal((B, P, L, 4)).astype(np.float32) if flags & 1 else nan(B, P, L, 4)
    inp['gt_rot'] = rng.standard_normal((B, P, R)).astype(np.float32) if flags & 4 else nan(B, P, R)
    inp['gt_tr'] = rng.standard_normal((B, P, T)).astype(np.float32) if flags & 8 else nan(B, P, T)
    vals = [-1, 0, 2, 3, L, L + 5]
    inp['num_edges'] = np.array([vals[(i + q) % 6] for q in range(B * P)], np.int32)
    if gscale is not None:
        inp['gscale'] = np.array([gscale], np.float32)
    case.p = dict(B=B, P=P, L=L, R=R, T=T, flags=flags, pad=(f32r(pad[0]), f32r(pad[1])), loop_w=f32r(loop_w), gscale=gscale,
                  layout=layout, g_rot=bool(flags & 4) or not gnull, g_tr=bool(flags & 8) or not gnull)
    bwd = {'g_ol': _out(B * P * L * 4)}
    if case.p['g_rot']:
        bwd['g_rot'] = _out(B * P * R)
    if case.p['g_tr']:
        bwd['g_tr'] = _out(B * P * T)
    case.out0 = {'pattern_loss_fwd': {'part': _out(B * 4, np.float64), 'loop_sums': _out(B * P * 2), 'out5': _out(5)}, 'pattern_loss_bwd': bwd}
    case.id = '%d-%d-%d-%d-%d-f%d-%s-gs%s-%s-w%g%s' % (B, P, L, R, T, flags, layout, 'N' if gscale is None else '%g' % gscale,
                                                       'pad' if pad[0] else 'nopad', loop_w, '-gn' if gnull else '')
    return case


def restate_pattern(case, variant=None):
    """closed form in fp64 -> dict(out5, g_ol [B,P,L,4], g_rot [B,P,R], g_tr [B,P,T])"""
    p = case.p
    B, P, L, R, T, flags = p['B'], p['P'], p['L'], p['R'], p['T'], p['flags']
    gs = 1.0 if p['gscale'] is None else p['gscale']
    dense = variant == 'dense_layout'
    g_ol, g_rot, g_tr = np.zeros((B, P, L, 4)), np.zeros((B, P, R)), np.zeros((B, P, T))
    shape = loop = rot = tr = 0.0
    if flags & 1:
        d = _read(case, 'ol', dense) - case.inp['gt_ol']
        shape = (d ** 2).mean()
        g_ol += gs * 2 * d / d.size
    if flags & 2:
        ol = _read(case, 'ol', dense)
        pad = np.zeros(2) if variant == 'pad_ignored' else np.array(p['pad'])
        ne = case.inp['num_edges'].reshape(B, P).astype(np.int64)
        n = np.clip(ne, 0, L)
        on = n >= (0 if variant == 'short_panels_not_skipped' else 3)
        upto = np.where(on, L if variant == 'loop_over_L' else n, 0)
        live = np.arange(L)[None, None, :] < upto[:, :, None]
        sums = ((ol[..., :2] - pad) * live[..., None]).sum(2)
        loop = (sums ** 2).sum() / (B * P * 2)
        lw = 1.0 if variant == 'loop_w_dropped' else p['loop_w']
        k = (1.0 if variant == 'gscale_dropped_loop' else gs) * (1.0 if variant == 'loop_w_dropped_bwd' else lw) * 2 / (B * P * 2)
        g = k * sums[:, :, None, :] * live[..., None]
        g_ol[..., :2] += g
        if variant == 'loop_grad_on_columns_2_3':
            g_ol[..., 2:] += g
    else:
        lw = p['loop_w']
    if flags & 4:
        d = _read(case, 'rot', dense).reshape(B, P, R) - case.inp['gt_rot']
        cnt = B * P if variant == 'rot_count' else d.size
        rot = (d ** 2).sum() / cnt
        g_rot += (1.0 if variant == 'gscale_dropped_rot' else gs) * 2 * d / cnt
    if flags & 8:
        d = _read(case, 'tr', dense).reshape(B, P, T) - case.inp['gt_tr']
        tr = (d ** 2).mean()
        g_tr += gs * 2 * d / d.size
    total = 0.0
    if flags & 1:
        total = total + shape
    if flags & 2:
        total = total + lw * loop
    if flags & 4:
        total = total + rot
    if flags & 8:
        total = total + tr
    return dict(out5=np.array([total, shape, loop, rot, tr]), g_ol=g_ol, g_rot=g_rot, g_tr=g_tr)


def oracle_pattern(case):
    """torch's fp64 mse_loss and the oracle's PanelLoopLoss under autograd, summed in ComposedPatternLoss's order"""
    from oracle import ref_path as O
    p = case.p
    B, P, L, R, T, flags = p['B'], p['P'], p['L'], p['R'], p['T'], p['flags']
    gs = 1.0 if p['gscale'] is None else p['gscale']
    mse = torch.nn.functional.mse_loss
    leaf = lambda name, shape: torch.tensor(case.v64(name), dtype=F64).reshape(shape).requires_grad_()
    ol = leaf('ol', (B, P, L, 4)) if flags & 3 else None
    rot = leaf('rot', (B, P, R)) if flags & 4 else None
    tr = leaf('tr', (B, P, T)) if flags & 8 else None
    out5, loss = np.zeros(5), 0.
    if flags & 1:
        t = mse(ol, torch.tensor(case.inp['gt_ol'], dtype=F64))
        out5[1], loss = t.item(), loss + t
    if flags & 2:
        t = O.PanelLoopLoss(torch.tensor([p['pad'][0], p['pad'][1], 0., 0.], dtype=F64))(ol, torch.tensor(case.inp['num_edges']))
        out5[2], loss = t.item(), loss + p['loop_w'] * t
    if flags & 4:
        t = mse(rot, torch.tensor(case.inp['gt_rot'], dtype=F64))
        out5[3], loss = t.item(), loss + t
    if flags & 8:
        t = mse(tr, torch.tensor(case.inp['gt_tr'], dtype=F64))
        out5[4], loss = t.item(), loss + t
    out5[0] = float(torch.as_tensor(loss).detach())
    if torch.is_tensor(loss) and loss.requires_grad:
        (loss * gs).backward()
    g = lambda t, shape: t.grad.numpy() if t is not None and t.grad is not None else np.zeros(shape)
    return dict(out5=out5, g_ol=g(ol, (B, P, L, 4)), g_rot=g(rot, (B, P, R)), g_tr=g(tr, (B, P, T)))


# ----------------------------------------------------------------------------------------------------------------------
# renumbering and panel shift (integers / copies: exact)
# ----------------------------------------------------------------------------------------------------------------------
def _renumber_specs():
    specs = []
    for shape in [(1, 1, 1, 3), (3, 5, 4, 5), (2, 64, 23, 14), (2, 70, 23, 14)]:
        for perm, lead in (('perm', True), ('rep', True), ('perm', False), (None, True), ('rep', False), (None, False)):
            if perm == 'rep' and shape[2] == 1:
                continue
            specs.append((shape, perm, lead))
    return specs


def build_renumber(spec):
    (B, S, P, L), perm, lead = spec
    rng = np.random.default_rng([3000, B, S, P, L, lead, 0 if perm is None else len(perm)])
    nums = np.array([[S, 0, S + 3, -2, max(S // 2, 1)][(b + (0 if perm is None else len(perm)) + lead) % 5] for b in range(B)], np.int64)
    if B == 1:
        nums[:] = S
    inp = {'nums': nums}
    n_edges = np.array([[3, L, L - 1, 4][q % 4] if L > 3 else 3 for q in range(B * P)], np.int32)
    st = np.empty((B, 2, S), np.int64)
    for b in range(B):
        n = min(max(int(nums[b]), 0), S)
        panel = rng.integers(0, P, (2, S))
        st[b] = panel * L + rng.integers(0, L, (2, S))
        st[b, 0, n:], st[b, 1, n:] = 10 ** 12 + 7, -(10 ** 6) - 3
    inp['stitches'] = st
    if perm:
        pm = np.stack([rng.permutation(P) for _ in range(B)]).astype(np.int64)
        if perm == 'rep':
            pm[:, -1] = pm[:, 0]             # the first panel is named twice (its last slot wins), another one never (-> -1)
        inp['perm'] = pm
    if lead:
        inp['num_edges'] = n_edges
        inp['lead'] = np.array([[0, 1, int(n_edges[q]) - 1][q % 3] for q in range(B * P)], np.int32)
    case = Case(group='renumber', inp=inp, view={}, p=dict(B=B, S=S, P=P, L=L, perm=perm, lead=lead),
                out0={'stitch_renumber': {'out': _out(B * 2 * S, np.int64)}})
    case.id = '%d-%d-%d-%d-%s-%s' % (B, S, P, L, perm or 'p0', 'lead' if lead else 'l0')
    return case


def restate_renumber(case, variant=None):
    """the oracle's _stitch_after_permute and _gt_stitches_shift on clones (variant=None), or a restatement with one mistake"""
    from oracle.ref_path import ComposedPatternLoss as C
    p, inp = case.p, case.inp
    B, S, P, L = p['B'], p['S'], p['P'], p['L']
    nums = [min(max(int(n), 0), S) for n in inp['nums']]
    if variant == 'tail_not_copied':
        out = restate_renumber(case)
        for b, n in enumerate(nums):
            out[b, :, n:] = 0
        return out
    if variant is None:
        out = torch.tensor(inp['stitches'])
        if 'perm' in inp:
            out = C._stitch_after_permute(out.clone(), nums, torch.tensor(inp['perm']), L)
        if 'lead' in inp:
            # a negative flat panel number reads element 0 (Python would wrap to the last element: a copy of element 0 is put there)
            ld, ne = list(inp['lead']) + [inp['lead'][0]], list(inp['num_edges']) + [inp['num_edges'][0]]
            out = C._gt_stitches_shift(out.clone(), nums, ld, ne, P, L)
        return out.numpy()
    out = inp['stitches'].copy()
    for b, n in enumerate(nums):
        for side in (0, 1):
            for i in range(n):
                e = int(out[b, side, i])
                panel0 = e // L
                if 'perm' in inp:
                    slots = [r for r in range(P) if inp['perm'][b, r] == panel0]
                    slot = -1 if not slots else slots[0 if variant == 'first_slot_wins' else -1]
                    e = slot * L + (e - panel0 * L)
                if 'lead' in inp:
                    panel = e // L if variant != 'truncating_division' else int(e / L)
                    inner = e - panel * L
                    g = max(b * P + (panel0 if variant == 'lead_indexed_before_perm' else panel), 0)
                    ld, ne = int(inp['lead'][g]), int(inp['num_edges'][g])
                    if variant == 'shift_wrong_direction':
                        e = panel * L + (inner + ld if inner + ld < ne else inner + ld - ne)
                    else:
                        e = panel * L + (inner - ld if inner >= ld else ne - (ld - inner))
                out[b, side, i] = e
    return out


def _shift_specs():
    return [(n, L, D) for n in (1, 7, 46) for L in (3, 14) for D in (1, 3)]


def build_shift(spec):
    npanels, L, D = spec
    rng = np.random.default_rng([4000, npanels, L, D])
    vals = [3, L + 5, 2, L, 0, 3, L]
    ne = np.array([vals[(q + L + D) % 7] for q in range(npanels)], np.int32)
    # lead cycles through 0, 1, n - 1 with n the panel's own count: n - 1 = L + 4 lies past the panel when num_edges = L + 5
    lead = np.array([[1, int(ne[q]) - 1, 0][q % 3] if ne[q] > 0 else 0 for q in range(npanels)], np.int32)
    feat = rng.standard_normal((npanels, L, D)).astype(np.float32)
    case = Case(group='shift', inp={'feat': feat, 'lead': lead, 'num_edges': ne}, view={}, p=dict(npanels=npanels, L=L, D=D),
                out0={'panel_shift': {'out': _out(npanels * L * D)}})
    case.id = '%d-%d-%d' % spec
    return case


def restate_shift(case, variant=None):
    from oracle.ref_path import ComposedPatternLoss as C
    p, inp = case.p, case.inp
    feat = inp['feat']
    if variant is None:
        return C._per_panel_shift(torch.tensor(feat)[None], list(inp['lead']), list(inp['num_edges'])).numpy()[0]
    out = feat.copy()
    for q in range(p['npanels']):
        ld, n = int(inp['lead'][q]), min(int(inp['num_edges'][q]), p['L'])
        if variant == 'padding_rotated':
            n = p['L']
        if n < (2 if variant == 'acts_on_two_edges' else 3) or not 0 < ld < n:
            continue
        if variant == 'shift_wrong_direction':
            ld = n - ld
        out[q, :n] = np.concatenate([feat[q, ld:n], feat[q, :ld]])
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the case lists, the reference of a case, the checker, the emulation, the C-ABI argument lists
# ----------------------------------------------------------------------------------------------------------------------
_BUILDERS = {'stitch': (build_stitch, _stitch_specs), 'pattern': (build_pattern, _pattern_specs),
             'renumber': (build_renumber, _renumber_specs), 'shift': (build_shift, _shift_specs)}
GROUP = {'stitch_loss_fwd': 'stitch', 'stitch_loss_bwd': 'stitch', 'pattern_loss_fwd': 'pattern', 'pattern_loss_bwd': 'pattern',
         'stitch_renumber': 'renumber', 'panel_shift': 'shift'}
_CACHE = {}


def cases(kernel):
    """the cases of an entry point, built once and shared (nothing may change them: tests compare against copies)"""
    group = GROUP[kernel]
    if group not in _CACHE:
        build, specs = _BUILDERS[group]
        _CACHE[group] = [build(s) for s in specs()]
        ids = [c.id for c in _CACHE[group]]
        assert len(set(ids)) == len(ids), ids
    return _CACHE[group]


def case_ids(kernel):
    return [c.id for c in cases(kernel)]


VARIANTS = {
    'stitch_loss_fwd': ['brother_included', 'self_included', 'pairs_div_n', 'ntot_2S', 'sim_div_S', 'sim_div_total', 'bce_count',
                        'sup_count', 'sup_w_dropped', 'dense_layout'],
    'stitch_loss_bwd': ['brother_included', 'pairs_div_n', 'ntot_2S', 'sim_div_S', 'sim_div_total', 'first_tied_minimum',
                        'other_end_no_grad', 'dup_overwritten', 'sup_lost_under_scatter', 'bce_count', 'sup_count', 'sup_w_dropped',
                        'gscale_dropped_sup', 'gscale_dropped_free', 'gscale_dropped_stitch', 'dense_layout'],
    'pattern_loss_fwd': ['loop_over_L', 'short_panels_not_skipped', 'pad_ignored', 'loop_w_dropped', 'rot_count', 'dense_layout'],
    'pattern_loss_bwd': ['loop_over_L', 'short_panels_not_skipped', 'pad_ignored', 'loop_w_dropped_bwd', 'gscale_dropped_loop',
                         'gscale_dropped_rot', 'loop_grad_on_columns_2_3', 'rot_count', 'dense_layout'],
    'stitch_renumber': ['first_slot_wins', 'shift_wrong_direction', 'lead_indexed_before_perm', 'truncating_division', 'tail_not_copied'],
    'panel_shift': ['padding_rotated', 'acts_on_two_edges', 'shift_wrong_direction'],
}


def expected(case, variant=None):
    """the fp64 reference of a case (variant=None: the oracle; else the restatement with one mistake)"""
    if case.group == 'stitch':
        if variant is None and case.kind != 'gap0':
            return oracle_stitch(case)
        return restate_stitch(case, 'kernel', variant)
    if case.group == 'pattern':
        return oracle_pattern(case) if variant is None else restate_pattern(case, variant)
    if case.group == 'renumber':
        return dict(out=restate_renumber(case, variant))
    return dict(out=restate_shift(case, variant))


def relerr(a, b):
    """the suite's relerr (tests/test_gpu_kernels.py): max |a - b| / max |b|; a NaN on either side is an error"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    r = np.abs(a - b).max() / (np.abs(b).max() + 1e-30)
    return float('inf') if np.isnan(r) else float(r)


def _tail_intact(case, kernel, name, got, n):
    orig = case.out0[kernel][name]
    assert got.shape == orig.shape and got.dtype == orig.dtype, (case.id, name, got.shape, got.dtype)
    assert got[n:].tobytes() == orig[n:].tobytes(), '%s[%s] %s: written past its %d elements: %r' % (kernel, case.id, name, n, got[n:])


def _grad(case, kernel, name, got, ref, scale, worst):
    n = ref.size
    _tail_intact(case, kernel, name, got, n)
    g, r = got[:n].astype(np.float64), ref.reshape(-1)
    zero = r == 0
    if scale == 1.0:
        assert (g[zero] == 0).all(), '%s[%s] %s: not exactly 0 where the reference is, first at %d: %r' % (
            kernel, case.id, name, np.flatnonzero(zero & (g != 0))[0], g[zero & (g != 0)][0])
    e = relerr(g, r)
    worst[name] = e / GRAD_BAR
    assert e < GRAD_BAR * scale, '%s[%s] %s: relerr %.3e (bar %.1e)' % (kernel, case.id, name, e, GRAD_BAR * scale)


def _values(case, kernel, got, ref, scale, worst):
    _tail_intact(case, kernel, 'out5', got, 5)
    for q in range(5):
        g, r = float(got[q]), float(ref[q])
        if np.isnan(r) or np.isnan(g):
            assert np.isnan(r) and np.isnan(g), '%s[%s] out5[%d]: got %r, reference %r' % (kernel, case.id, q, g, r)
            continue
        bar = VALUE_BAR * max(1.0, abs(r))
        worst['out5[%d]' % q] = abs(g - r) / bar
        assert abs(g - r) < bar * scale, '%s[%s] out5[%d]: got %r, reference %r (%.2f bars)' % (kernel, case.id, q, g, r, abs(g - r) / bar)


def check(case, kernel, got, variant=None, scale=1.0):
    """got {name: the whole output buffer, tail included} against expected(case, variant); `scale` multiplies every bar (the host
    test asks a variant to miss by ten bars).  -> {output: worst error in bars}"""
    ref, worst = expected(case, variant), {}
    p = case.p
    if kernel == 'stitch_loss_fwd':
        _values(case, kernel, got['out5'], ref['out5'], scale, worst)
        part = got['part']
        _tail_intact(case, kernel, 'part', part, p['B'] * 6)
        if p['flags'] & 1:
            part = part[:p['B'] * 6].reshape(p['B'], 6)
            assert (part[:, 2] == 2.0 * np.array(p['nums'])).all(), (case.id, part[:, 2])
            for b, n in enumerate(p['nums']):
                r = ref['sim_b'][b]
                if n == 0:
                    assert np.isnan(part[b, 0]) and np.isnan(r), (case.id, b, part[b, 0], r)
                    continue
                bar = VALUE_BAR * max(1.0, abs(r))
                worst['part[0]'] = max(worst.get('part[0]', 0.0), abs(part[b, 0] - r) / bar)
                assert abs(part[b, 0] - r) < bar * scale, '%s[%s] part[%d][0]: got %r, reference %r' % (kernel, case.id, b, part[b, 0], r)
    elif kernel == 'stitch_loss_bwd':
        for name in ('g_tags', 'g_mask'):
            assert (name in got) == p[name], (case.id, name)
            if name in got:
                _grad(case, kernel, name, got[name], ref[name], scale, worst)
    elif kernel == 'pattern_loss_fwd':
        _values(case, kernel, got['out5'], ref['out5'], scale, worst)
        _tail_intact(case, kernel, 'part', got['part'], p['B'] * 4)
        _tail_intact(case, kernel, 'loop_sums', got['loop_sums'], p['B'] * p['P'] * 2 if p['flags'] & 2 else 0)
    elif kernel == 'pattern_loss_bwd':
        for name in ('g_ol', 'g_rot', 'g_tr'):
            assert (name in got) == p.get(name, True), (case.id, name)
            if name in got:
                _grad(case, kernel, name, got[name], ref[name], scale, worst)
    else:
        name, r = 'out', ref['out'].reshape(-1)
        _tail_intact(case, kernel, name, got[name], r.size)
        g = got[name][:r.size]
        bad = np.flatnonzero(g != r.astype(g.dtype))
        assert not bad.size, '%s[%s] out: %d elements differ, first at %d: got %r, reference %r' % (kernel, case.id, bad.size, bad[0], g[bad[0]], r[bad[0]])
    return worst


def emulate(case, kernel):
    """what a correct kernel returns: the reference (with the kernels' convention at gap 0) rounded once to the output's type"""
    ref = expected(case)
    p = case.p
    out = {n: a.copy() for n, a in case.out0[kernel].items()}

    def put(name, v):
        v = np.asarray(v).reshape(-1)
        out[name][:v.size] = v.astype(out[name].dtype)

    if kernel in ('stitch_loss_fwd', 'pattern_loss_fwd'):
        put('out5', ref['out5'])
        if kernel == 'stitch_loss_fwd':
            part = np.zeros((p['B'], 6))
            if p['flags'] & 1:
                part[:, 0], part[:, 2] = ref['sim_b'], 2.0 * np.array(p['nums'])
            put('part', part)
        else:
            put('part', np.zeros(p['B'] * 4))
            if p['flags'] & 2:
                put('loop_sums', np.zeros(p['B'] * p['P'] * 2))
    else:
        for name in out:
            put(name, ref[name])
    return out


def abi_args(case, kernel, dev):
    """the argument list of include/gpe_hip.h for `gpe_<kernel>` (without the trailing stream) from dev {name: device tensor of
    case.inp / case.out0}; a view becomes a sliced tensor (its data pointer carries the offset) and its strides in elements"""
    p = case.p

    def view(name):
        base, idx = case.view[name]
        return dev[base][idx]

    if case.group == 'stitch':
        tags = view('tags') if p['flags'] & 9 else None
        logit = view('logit') if p['flags'] & 4 else None
        ts = list(tags.stride()[:3]) if tags is not None else [0, 0, 0]
        ms = list(logit.stride()) if logit is not None else [0, 0, 0]
        args = [tags, *ts, p['D'], logit, *ms, dev['stitches'], dev['nums'], p['S'], dev['gt_mask'], dev['gt_tags'], p['B'], p['P'], p['L'],
                p['flags'], p['margin'], p['sup_w'], dev['part']]
        if kernel == 'stitch_loss_fwd':
            return args + [dev['out5']]
        return args + [dev.get('gscale'), dev.get('g_tags'), dev.get('g_mask')]
    if case.group == 'pattern':
        fl = p['flags']
        ol = view('ol') if fl & 3 else None
        rot, tr = (view('rot') if fl & 4 else None), (view('tr') if fl & 8 else None)
        os_ = list(ol.stride()[:3]) if ol is not None else [0, 0, 0]
        args = [ol, *os_, rot, rot.stride(0) if rot is not None else 0, tr, tr.stride(0) if tr is not None else 0, dev['gt_ol'],
                dev['gt_rot'], dev['gt_tr'], dev['num_edges'], p['B'], p['P'], p['L'], p['R'], p['T'], fl, p['pad'][0], p['pad'][1], p['loop_w']]
        if kernel == 'pattern_loss_fwd':
            return args + [dev['part'], dev['loop_sums'], dev['out5']]
        return args + [dev['loop_sums'], dev.get('gscale'), dev['g_ol'], dev.get('g_rot'), dev.get('g_tr')]
    if case.group == 'renumber':
        return [dev['stitches'], dev['nums'], p['B'], p['S'], p['P'], p['L'], dev.get('perm'), dev.get('lead'), dev.get('num_edges'), dev['out']]
    return [dev['feat'], p['D'], dev['lead'], dev['num_edges'], p['npanels'], p['L'], dev['out']]

"""Test infrastructure: the graph search (gpe_knn; csrc/gpe_knn_plan.h, gpe_knn.hip, gpe_knn3.hip, gpe_knn_ft.hip) restated rung by
rung, in the shape of tests/redgemm_restate.py.

gpe_knn is one ladder of five paths (include/gpe_hip.h gpe_knn_path names them): 1 sorted cloud, 2 all-pairs,
3 threshold scan, 4 ordered lists, 5 fp32 filter.  The all-pairs kernel is exact by construction and the plan falls back to it
silently (a workspace that is NULL, misaligned or short), so a result alone never says which kernel produced it.  This module has

  the plan      `ws_layout`, `k2`, `plan`: gpe_knn_ws_layout, gpe_knn_k2 and gpe_knn_plan written from DESIGN.md 5.32 in plain Python,
                with the fields of gpe_knn_path's plan_out; tests/test_knn_host.py holds them against the export on every case and
                on a seeded sweep.  `instance(path, plan)` names the kernel instances a plan launches.
  the cases     `Knn` specs, one search each: (B, N, C, ldx, k, base offset in floats, ws kind, reserved CUs, switches), the path
                and the main kernel instance it was written for, and its data kinds.  GROUPS orders them by the switch set they
                need: 'default' needs none and runs in the pytest process, every other group is one child process started with
                GPE_DEBUG=1 and the group's GPE_KNN_* variables (the switches are read once per process).
  the buffers   `build(spec, kind, pad)` lays the search out on the host (below).
  the checks    `reference(spec, kind)` is oracle.ref_path.knn_local on the contiguous [B*N, C] copy — the project's definition:
                the fp32 fmaf chain over the channels, the lower index winning ties.  `check(case, out)` compares every query of
                idx and idx_glob with it bit for bit, and the order, and every sentinel; nothing is filtered.
                `wrong(case, name)` is a plausible wrong answer; the host test shows that `check` rejects each one.

BUFFERS.  x lies inside a larger allocation of NaN: GUARD_ROWS guard rows in front (then the case's base offset, which sets the
alignment the staging rules look at), the [B*N, ldx] table, GUARD_ROWS guard rows behind.  The pad columns C .. ldx-1 hold NaN (pad 'nan') or large finite
per-row garbage (pad 'garbage': multiples of the table's largest magnitude, distinct per row) — the all-pairs kernel copies what it
loads, the fp32 filter loads into the pad and must zero it, the norms, planes and recheck kernels mask their own tails: a zero pad
hides a mistake in any of them.  idx, idx_glob and order_out are pre-filled with -7 between zones of ZONE sentinel ints.  The
workspace is the bytes the case passes plus WS_TAIL sentinel bytes, and is filled before the launch with 0x00 bytes, with 0xFF bytes
and with stale keys between empty slots (`ws_image`: a slot of the scan's lists is empty when it holds ~0, and a missing
initialisation is invisible when the same shape ran just before).

DATA KINDS, seeded per case, finite everywhere: gauss; offset (|randn| 0.3 + 5 + a common row); clusters (8 centres of randn 20,
noise 1e-2: tiny distance differences on large norms); lattice (integers 0..2 in the first 8 channels: exact ties); same (all points
identical); scales (each row times 2^e, e uniform in -20..20: the recheck bound of most queries degenerates); tiny (randn 2^-64:
squared norms in the subnormal range); huge (randn 2^55: with C <= 300 the largest chain sum stays below 2^128).  Every case runs
the first five (the one N = 8192 case gauss only: the oracle takes 3 s per kind there, and the sorted cloud meets the other kinds
at 128 .. 577 points); scales, tiny and huge run on one case per rung (`Knn.kinds`).

The natural candidate split of the all-pairs kernel (the tables of the clouds in flight exceed an L2) needs tables of megabytes per
cloud: it stays out of the GPU cases.  Its rule is part of `plan` and is held against the library by the sweep of
tests/test_knn_host.py; the pieces themselves are reached through GPE_KNN_SPLIT.  The PROBE instances give wrong results by design
and are left out.

NumPy and the oracle only: no GPU and no gpe_amd."""
import collections
import functools
import zlib

import numpy as np

NOTHING, SORTED3, ALLPAIRS, SCAN, LISTS, F32FILTER = 0, 1, 2, 3, 4, 5
PATH_NAMES = {SORTED3: 'sorted', ALLPAIRS: 'allpairs', SCAN: 'scan', LISTS: 'lists', F32FILTER: 'f32filter'}
EINVAL = -22

SW_FIELDS = ('PROBE', 'PIN', 'VEC', 'SPLIT', 'EXACT', 'F32FILTER', 'SORTED', 'NOORDER', 'FT', 'RR2')
SW_DEFAULT = dict(PROBE=0, PIN=-1, VEC=0, SPLIT=0, EXACT=0, F32FILTER=0, SORTED=1, NOORDER=0, FT=1, RR2=1)
PLAN_FIELDS = ('identity', 'pin', 'tiles', 'nsplit', 'vec', 'nblocks', 'probe', 'smallc', 'K2', 'CP', 'NB', 'ce_bits', 'wide', 'qtiles',
               'rerank2', 'unsorted', 'order', 'part', 'norms', 'cmax', 'planes', 'iscale', 'xs', 'tb')

NXCD = 8
GUARD_ROWS = 64         # rows of NaN in front of and behind the table (rounded up to 256 bytes: the base offset alone sets the alignment)
ZONE = 64               # sentinel ints on either side of idx, idx_glob and order_out
ZONE_VALUE = 0x5A5A5A5A
PREFILL = -7
WS_TAIL = 4096          # sentinel bytes behind the workspace
WS_TAIL_BYTE = 0xA5


def switches(**kw):
    """the ten ints of GpeKnnSwitches, defaults where not named"""
    sw = dict(SW_DEFAULT)
    sw.update(kw)
    return tuple(int(sw[f]) for f in SW_FIELDS)


def cdiv(a, b):
    return -(-a // b)


def up256(b):
    return (b + 255) & ~255


# ----------------------------------------------------------------------------------------------------------------------
# the layout and the plan
# ----------------------------------------------------------------------------------------------------------------------
def ws_layout(B, N, C):
    nq = B * N
    norm_bytes, cmax_bytes = up256(nq * 4), up256(B * 4)
    CP = (C + 31) & ~31
    pl_bytes = up256(nq * 2 * CP * 2)
    w = {'lists_bytes': nq * 64 * 8}
    w['norms'] = w['lists_bytes']
    w['cmax'] = w['norms'] + norm_bytes
    w['planes'] = w['cmax'] + cmax_bytes
    w['iscale'] = w['planes'] + pl_bytes
    w['tb'] = nq * 16
    w['sorted_bytes'] = w['tb'] + B * cdiv(N, 64) * 8 * 4
    w['need_f32'] = w['planes'] + 256
    w['need_h3'] = w['need_f32'] + pl_bytes + norm_bytes
    w['total'] = (w['need_h3'] if 16 <= C <= 256 else w['need_f32']) + 256
    return w


def ws_bytes(B, N, C, k):
    """gpe_knn_ws_bytes"""
    if B < 0 or N <= 0 or C <= 0 or k <= 0 or k > 64:
        return EINVAL
    return ws_layout(B, N, C)['total']


def split_bytes(B, N, nsplit, k):
    return B * N * nsplit * k * 8


def k2(k, N):
    K2 = min(2 * k, 32)
    K2 = max(K2, k + 8)
    return min(K2, 64, N)


Call = collections.namedtuple('Call', 'x B N C ldx k has_idx_glob has_order_in has_order_out ws ws_bytes')    # x, ws: addresses (0 = NULL)


def _holds(c, nbytes):
    return c.ws != 0 and c.ws % 16 == 0 and c.ws_bytes >= nbytes


def _tile_blocks(pin, B, tiles):
    return NXCD * cdiv(B, NXCD) * tiles if pin else B * tiles


def _allpairs(p, c, usable_cus, sw, with_ws):
    p['nsplit'] = 1
    if p['pin']:
        table, budget = float(c.N) * c.ldx * 4, 3.2 * 1024 * 1024
        resident = 4 * usable_cus // NXCD
        while True:
            clouds = resident / (float(p['tiles']) * p['nsplit'])
            if table * max(clouds, 1.0) <= budget or clouds <= 1.0:
                break
            if p['nsplit'] >= 4 or 2 * p['nsplit'] * c.k > 64 or 2 * p['nsplit'] > p['tiles']:
                break
            p['nsplit'] *= 2
    if sw['SPLIT'] > 0 and sw['SPLIT'] * c.k <= 64 and sw['SPLIT'] <= p['tiles']:
        p['nsplit'] = sw['SPLIT']
    if p['nsplit'] > 1:
        if with_ws and _holds(c, split_bytes(c.B, c.N, p['nsplit'], c.k)):
            p['part'] = 0
        else:
            p['nsplit'] = 1
    p['nblocks'] = _tile_blocks(p['pin'], c.B, p['tiles']) * p['nsplit']
    if p['nblocks'] >= 1 << 31:
        return EINVAL, None
    p['vec'] = 4 if (c.C % 4 == 0 and c.ldx % 4 == 0 and c.x % 16 == 0) else 2 if (c.C % 2 == 0 and c.ldx % 2 == 0 and c.x % 8 == 0) else 1
    if 0 < sw['VEC'] < p['vec']:
        p['vec'] = sw['VEC']
    p['probe'] = sw['PROBE']
    p['smallc'] = int(not p['probe'] and p['vec'] == 1 and c.C <= 4)
    return ALLPAIRS, p


def plan(c, usable_cus, sw=None):
    """gpe_knn_path's answer for the call `c` on `usable_cus` compute units under the ten switches `sw` (a tuple in SW_FIELDS order):
    (return value, {PLAN_FIELDS} or None)"""
    sw = dict(zip(SW_FIELDS, switches() if sw is None else sw))
    # step 0
    if not (c.x and c.B >= 0 and c.N > 0 and c.C > 0 and c.ldx >= c.C and 0 < c.k <= 64 and c.k <= c.N and c.B * c.N * c.k < 1 << 31):
        return EINVAL, None
    if c.B == 0:
        return 0, None
    p = dict.fromkeys(PLAN_FIELDS, 0)
    for region in ('part', 'norms', 'cmax', 'planes', 'iscale', 'xs', 'tb'):
        p[region] = -1
    p['tiles'] = cdiv(c.N, 64)
    p['pin'] = int(bool(sw['PIN']) and c.B >= NXCD) if sw['PIN'] >= 0 else int(c.B >= NXCD)
    p['nsplit'] = 1
    w = ws_layout(c.B, c.N, c.C)
    # step 1
    if c.C < 16 or c.k > 48 or sw['EXACT']:
        if c.C == 3 and sw['SORTED'] != 0 and 128 <= c.N <= 8192 and _holds(c, w['sorted_bytes']) and c.B * cdiv(c.N, 16) < 1 << 31:
            p['tiles'] = cdiv(c.N, 64)
            p['qtiles'] = cdiv(c.N, 16)
            p['nblocks'] = c.B * p['qtiles']
            p['xs'], p['tb'] = 0, w['tb']
            return SORTED3, p
        p['identity'] = int(c.has_order_out)
        return _allpairs(p, c, usable_cus, sw, True)
    # step 2
    p['identity'] = int(c.has_order_out)
    p['K2'] = k2(c.k, c.N)
    if sw['SPLIT'] > 0 and sw['SPLIT'] * p['K2'] <= 64 and sw['SPLIT'] <= p['tiles']:
        p['nsplit'] = sw['SPLIT']
    h3 = (not sw['F32FILTER']) and c.C <= 256
    if h3 and (c.ws == 0 or c.ws_bytes < w['need_h3']):
        h3 = False
    if not _holds(c, w['need_h3'] if h3 else w['need_f32']):                    # 2a
        return _allpairs(p, c, usable_cus, sw, False)
    p['part'], p['norms'], p['cmax'] = 0, w['norms'], w['cmax']
    p['CP'] = (c.C + 31) & ~31
    p['NB'] = p['CP'] >> 5
    ce = (np.float32(6) * np.float32(c.C) + np.float32(32 if h3 else 16)) * np.float32(5.9604645e-8)
    p['ce_bits'] = int(np.array([ce], np.float32).view(np.uint32)[0])
    p['probe'] = sw['PROBE']
    p['nblocks'] = _tile_blocks(p['pin'], c.B, p['tiles']) * p['nsplit']
    if p['nblocks'] >= 1 << 31:
        return EINVAL, None
    if not h3:                                                                  # 2d, rule B
        p['vec'] = 4 if (c.ldx % 4 == 0 and c.x % 16 == 0 and ((c.C + 3) & ~3) <= c.ldx) else \
            2 if (c.ldx % 2 == 0 and c.x % 8 == 0 and ((c.C + 1) & ~1) <= c.ldx) else 1
        if 0 < sw['VEC'] < p['vec']:
            p['vec'] = sw['VEC']
        return F32FILTER, p
    p['planes'], p['iscale'] = w['planes'], w['iscale']
    p['order'] = int(bool(c.has_order_in) and not sw['NOORDER'])
    if sw['FT'] and p['NB'] <= 5 and c.k <= 32 and p['nsplit'] == 1:            # 2b
        p['wide'] = int(sw['FT'] == 8 or (sw['FT'] != 4 and c.B * cdiv(c.N, 128) >= usable_cus))
        p['qtiles'] = cdiv(c.N, 128 if p['wide'] else 64)
        p['nblocks'] = _tile_blocks(p['pin'], c.B, p['qtiles'])
        p['rerank2'] = int(sw['RR2'] != 0)
        p['unsorted'] = 1
        return SCAN, p
    return LISTS, p                                                             # 2c


def ce_of(p):
    return float(np.array([p['ce_bits']], np.uint32).view(np.float32)[0])


def regions(c, path, p):
    """[(name, first byte, bytes)] of the workspace regions the launch of plan `p` uses, by the layout"""
    w = ws_layout(c.B, c.N, c.C)
    nq = c.B * c.N
    size = {'norms': nq * 4, 'cmax': c.B * 4, 'planes': nq * 2 * ((c.C + 31) & ~31) * 2, 'iscale': nq * 4, 'xs': nq * 16,
            'tb': c.B * cdiv(c.N, 64) * 32}
    size['part'] = split_bytes(c.B, c.N, p['nsplit'], c.k) if path == ALLPAIRS else w['lists_bytes']
    return [(r, p[r], size[r]) for r in ('part', 'norms', 'cmax', 'planes', 'iscale', 'xs', 'tb') if p[r] >= 0]


ALL_INSTANCES = frozenset(
    ['identity', 'norms+cmax', 'planes', 'planes(order)', 'allpairs<4>', 'allpairs<2>', 'allpairs<1>', 'allpairs<smallc>', 'merge',
     'sort', 'query', 'scan<8>', 'scan<4>', 'rerank2', 'rerank(unsorted)', 'lists<2>', 'lists<5>', 'lists<8>', 'rerank', 'rerank(pieces)',
     'f32filter<4>', 'f32filter<2>', 'f32filter<1>'])


def instance(path, p):
    """the kernel instances the launch of a plan runs, in launch order; the main kernel's name is `main_instance`"""
    assert not p['probe'], 'the PROBE instances give wrong results by design'
    out = []
    if p['identity']:
        out.append('identity')
    if p['norms'] >= 0:
        out.append('norms+cmax')
    if p['planes'] >= 0:
        out.append('planes(order)' if p['order'] else 'planes')
    recheck = 'rerank(pieces)' if p['nsplit'] > 1 else 'rerank'
    if path == SORTED3:
        out += ['sort', 'query']
    elif path == ALLPAIRS:
        out.append('allpairs<smallc>' if p['smallc'] else 'allpairs<%d>' % p['vec'])
        if p['nsplit'] > 1:
            out.append('merge')
    elif path == SCAN:
        out += ['scan<8>' if p['wide'] else 'scan<4>', 'rerank2' if p['rerank2'] else 'rerank(unsorted)']
    elif path == LISTS:
        out += ['lists<%d>' % (2 if p['NB'] <= 2 else 5 if p['NB'] <= 5 else 8), recheck]
    else:
        out += ['f32filter<%d>' % p['vec'], recheck]
    return tuple(out)


def main_instance(path, p):
    return [n for n in instance(path, p) if n.split('<')[0] in ('allpairs', 'query', 'scan', 'lists', 'f32filter')][0]


# ----------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------
BASE_KINDS = ('gauss', 'offset', 'clusters', 'lattice', 'same')
EDGE_KINDS = ('scales', 'tiny', 'huge')
WS_KINDS = ('full', 'null', 'mis8', 'f32')

Knn = collections.namedtuple('Knn', 'group rung main B N C ldx k off ws res sw kinds')


def _k(group, rung, main, B, N, C, ldx, k, off=0, ws='full', res=0, edge=False, kinds=None, **sw):
    assert ws in WS_KINDS and not set(sw) - set(SW_FIELDS)
    if kinds is None:
        kinds = BASE_KINDS + (EDGE_KINDS if edge else ())
    return Knn(group, rung, main, B, N, C, ldx, k, off, ws, res, switches(**sw), tuple(kinds))


def _default_cases():
    g, A, S, F, L, X = 'default', ALLPAIRS, SCAN, F32FILTER, LISTS, SORTED3
    return [
        # all-pairs, small C: an unsorted xyz cloud (N < 128), one point, k = N, every staging width by pitch and by base address
        _k(g, A, 'allpairs<smallc>', 1, 70, 3, 3, 5),
        _k(g, A, 'allpairs<smallc>', 1, 1, 3, 3, 1),
        _k(g, A, 'allpairs<1>', 2, 40, 5, 5, 40),
        _k(g, A, 'allpairs<smallc>', 2, 70, 4, 5, 5),
        _k(g, A, 'allpairs<2>', 2, 70, 6, 6, 5, edge=True),
        _k(g, A, 'allpairs<4>', 2, 70, 8, 8, 5),
        _k(g, A, 'allpairs<4>', 2, 70, 8, 12, 5, edge=True),                   # vec 4 next to a pad of four floats
        _k(g, A, 'allpairs<2>', 2, 70, 6, 8, 5),                                # vec 2 next to a pad of two
        _k(g, A, 'allpairs<2>', 2, 70, 12, 16, 7, off=2),                       # vec 2 by the base address
        _k(g, A, 'allpairs<1>', 2, 70, 12, 16, 7, off=1),
        _k(g, A, 'allpairs<1>', 1, 70, 13, 13, 5, edge=True),
        _k(g, A, 'allpairs<1>', 2, 70, 7, 7, 64),
        # all-pairs, wide rows with k > 48
        _k(g, A, 'allpairs<2>', 2, 70, 150, 152, 50),                           # last chunk 22 channels
        _k(g, A, 'allpairs<1>', 1, 70, 33, 33, 49),                             # two chunks
        _k(g, A, 'allpairs<4>', 1, 130, 256, 256, 64),
        # query counts around a tile
        _k(g, A, 'allpairs<1>', 2, 63, 13, 13, 5),
        _k(g, A, 'allpairs<4>', 1, 64, 8, 8, 5),
        _k(g, A, 'allpairs<2>', 2, 65, 6, 6, 5),
        _k(g, A, 'allpairs<4>', 9, 70, 8, 8, 5),                                # nine clouds: pinned to XCDs
        # sorted cloud, and the same shapes with a misaligned workspace: the all-pairs kernel and the identity order
        _k(g, X, 'query', 2, 128, 3, 3, 5),
        _k(g, X, 'query', 2, 129, 3, 4, 16, edge=True),
        _k(g, X, 'query', 3, 577, 3, 3, 9),
        _k(g, X, 'query', 1, 577, 3, 4, 64),
        _k(g, X, 'query', 9, 130, 3, 3, 5),
        _k(g, X, 'query', 1, 8192, 3, 4, 16, kinds=('gauss',)),               # one kind: the oracle takes 3 s per kind at this size
        _k(g, A, 'allpairs<smallc>', 2, 128, 3, 3, 5, ws='mis8'),
        _k(g, A, 'allpairs<smallc>', 2, 129, 3, 4, 16, ws='mis8'),
        _k(g, A, 'allpairs<smallc>', 3, 577, 3, 3, 9, ws='mis8'),
        _k(g, A, 'allpairs<smallc>', 2, 129, 3, 4, 16, ws='null'),
        # threshold scan
        _k(g, S, 'scan<4>', 2, 130, 16, 16, 1),
        _k(g, S, 'scan<4>', 2, 130, 31, 31, 5, off=1),
        _k(g, S, 'scan<4>', 1, 131, 32, 32, 32),                                # an odd B N: the odd last query of rerank2
        _k(g, S, 'scan<4>', 2, 130, 33, 36, 5, edge=True),
        _k(g, S, 'scan<4>', 2, 130, 150, 152, 32, off=2),
        _k(g, S, 'scan<4>', 3, 97, 150, 150, 5),
        _k(g, S, 'scan<4>', 1, 200, 160, 160, 1),
        _k(g, S, 'scan<4>', 9, 130, 32, 32, 5),
        _k(g, S, 'scan<8>', 32, 130, 32, 36, 5, res=192, kinds=BASE_KINDS + ('scales',)),   # 64 usable CUs: wide
        # ordered lists
        _k(g, L, 'lists<2>', 2, 130, 33, 36, 40, edge=True),
        _k(g, L, 'lists<5>', 1, 200, 160, 160, 33),
        _k(g, L, 'lists<5>', 1, 130, 150, 152, 48),                             # the largest filtered k, K2 = 56
        _k(g, L, 'lists<8>', 1, 130, 161, 164, 16),
        _k(g, L, 'lists<8>', 1, 130, 200, 200, 5, off=1),
        _k(g, L, 'lists<8>', 2, 70, 256, 256, 48),
        _k(g, L, 'lists<2>', 9, 130, 33, 36, 40),
        # fp32 filter: every staging width; C <= 256 on a workspace of need_f32 bytes, where h3 is silently off
        _k(g, F, 'f32filter<1>', 1, 130, 257, 257, 5),
        _k(g, F, 'f32filter<2>', 1, 130, 257, 258, 16, edge=True),
        _k(g, F, 'f32filter<4>', 2, 70, 257, 260, 8),
        _k(g, F, 'f32filter<1>', 1, 130, 300, 300, 5, off=1),
        _k(g, F, 'f32filter<2>', 1, 130, 300, 300, 5, off=2),
        _k(g, F, 'f32filter<4>', 9, 70, 257, 260, 5),
        _k(g, F, 'f32filter<4>', 2, 130, 64, 64, 5, ws='f32'),
        _k(g, F, 'f32filter<4>', 1, 130, 24, 24, 5, ws='f32'),
        # step 2a: the filter group without a workspace
        _k(g, A, 'allpairs<4>', 2, 130, 24, 28, 5, ws='null'),
        _k(g, A, 'allpairs<2>', 2, 70, 150, 152, 9, ws='null'),
        _k(g, A, 'allpairs<4>', 2, 130, 32, 32, 5, ws='mis8'),
    ]


def _switch_cases():
    A, S, F, L = ALLPAIRS, SCAN, F32FILTER, LISTS
    out = []
    g = 'EXACT'
    out += [_k(g, A, 'allpairs<4>', 2, 130, 32, 32, 5, EXACT=1), _k(g, A, 'allpairs<2>', 2, 130, 150, 152, 16, EXACT=1),
            _k(g, A, 'allpairs<1>', 1, 130, 33, 36, 5, EXACT=1), _k(g, A, 'allpairs<4>', 1, 130, 160, 164, 9, EXACT=1, edge=True)]
    g = 'SPLIT2'
    out += [_k(g, A, 'allpairs<4>', 2, 130, 8, 8, 16, SPLIT=2), _k(g, A, 'allpairs<1>', 9, 130, 5, 5, 16, SPLIT=2),
            _k(g, L, 'lists<2>', 2, 130, 33, 36, 5, SPLIT=2, edge=True), _k(g, L, 'lists<8>', 1, 200, 161, 164, 16, SPLIT=2),
            _k(g, F, 'f32filter<4>', 1, 130, 257, 260, 5, SPLIT=2, edge=True),
            _k(g, A, 'allpairs<4>', 2, 130, 8, 8, 16, ws='null', SPLIT=2)]     # no workspace: one piece
    g = 'SPLIT3'                                                                # N = 130: the last piece has 2 candidates, fewer than k
    out += [_k(g, A, 'allpairs<4>', 2, 130, 8, 8, 16, SPLIT=3, edge=True), _k(g, L, 'lists<2>', 2, 130, 33, 36, 5, SPLIT=3),
            _k(g, L, 'lists<5>', 1, 130, 150, 152, 5, SPLIT=3), _k(g, F, 'f32filter<1>', 1, 130, 257, 257, 5, SPLIT=3)]
    g = 'SPLIT4'                                                                # N = 300: five tiles, two per piece, piece 3 is empty
    out += [_k(g, A, 'allpairs<4>', 2, 300, 8, 8, 16, SPLIT=4), _k(g, A, 'allpairs<smallc>', 1, 300, 4, 5, 16, SPLIT=4),
            _k(g, L, 'lists<2>', 1, 300, 33, 36, 5, SPLIT=4), _k(g, L, 'lists<8>', 1, 300, 161, 164, 5, SPLIT=4),
            _k(g, F, 'f32filter<2>', 1, 300, 257, 258, 5, SPLIT=4)]
    g = 'F32FILTER'                                                             # 16 <= C < 32: the chunk is (C + 15) & ~15 wide
    out += [_k(g, F, 'f32filter<4>', 2, 130, 16, 16, 5, F32FILTER=1), _k(g, F, 'f32filter<2>', 2, 130, 24, 26, 5, F32FILTER=1),
            _k(g, F, 'f32filter<1>', 2, 130, 24, 25, 5, F32FILTER=1), _k(g, F, 'f32filter<1>', 2, 130, 150, 151, 9, F32FILTER=1),
            _k(g, F, 'f32filter<4>', 1, 130, 150, 152, 9, F32FILTER=1, edge=True), _k(g, F, 'f32filter<4>', 1, 130, 17, 20, 5, F32FILTER=1)]
    g = 'SORTED0'
    out += [_k(g, A, 'allpairs<smallc>', 2, 128, 3, 3, 5, SORTED=0), _k(g, A, 'allpairs<smallc>', 1, 577, 3, 4, 9, SORTED=0, edge=True)]
    g = 'FT0'
    out += [_k(g, L, 'lists<2>', 2, 130, 32, 32, 5, FT=0), _k(g, L, 'lists<5>', 2, 130, 150, 152, 16, FT=0, edge=True),
            _k(g, L, 'lists<2>', 1, 131, 16, 16, 1, FT=0)]
    g = 'FT4'
    out += [_k(g, S, 'scan<4>', 32, 130, 32, 36, 5, res=192, FT=4),
            _k(g, S, 'scan<4>', 2, 130, 150, 152, 16, FT=4)]
    g = 'FT8'
    out += [_k(g, S, 'scan<8>', 2, 130, 32, 32, 5, FT=8, edge=True), _k(g, S, 'scan<8>', 1, 131, 150, 152, 32, FT=8),
            _k(g, S, 'scan<8>', 3, 257, 33, 36, 5, FT=8), _k(g, S, 'scan<8>', 9, 130, 16, 16, 1, FT=8)]
    g = 'RR20'
    out += [_k(g, S, 'scan<4>', 2, 130, 33, 36, 5, RR2=0, edge=True), _k(g, S, 'scan<4>', 1, 131, 150, 152, 32, RR2=0),
            _k(g, S, 'scan<8>', 32, 130, 32, 36, 5, res=192, RR2=0)]
    for v in (1, 2):                                                            # a vec-4 shape of the all-pairs kernel and of the fp32 filter
        g = 'VEC%d' % v
        out += [_k(g, A, 'allpairs<%d>' % v, 2, 70, 8, 12, 5, VEC=v), _k(g, A, 'allpairs<%d>' % v, 1, 130, 256, 256, 64, VEC=v),
                _k(g, F, 'f32filter<%d>' % v, 2, 70, 257, 260, 8, VEC=v), _k(g, A, 'allpairs<smallc>' if v == 1 else 'allpairs<2>', 2, 70, 4, 4, 5, VEC=v)]
    g = 'NOORDER'
    out += [_k(g, S, 'scan<4>', 2, 130, 33, 36, 5, NOORDER=1), _k(g, L, 'lists<2>', 2, 130, 33, 36, 40, NOORDER=1)]
    g = 'PIN0'
    out += [_k(g, A, 'allpairs<4>', 9, 70, 8, 8, 5, PIN=0), _k(g, S, 'scan<4>', 9, 130, 32, 32, 5, PIN=0),
            _k(g, L, 'lists<2>', 9, 130, 33, 36, 40, PIN=0), _k(g, F, 'f32filter<4>', 9, 70, 257, 260, 5, PIN=0)]
    return out


CASES = _default_cases() + _switch_cases()
GROUPS = collections.OrderedDict()
for _s in CASES:
    GROUPS.setdefault(_s.group, []).append(_s)
DEFAULT_BY_RUNG = collections.OrderedDict((PATH_NAMES[r], [s for s in GROUPS['default'] if s.rung == r])
                                          for r in (ALLPAIRS, SORTED3, SCAN, LISTS, F32FILTER))


def case_id(s):
    sw = ','.join('%s=%d' % (f, v) for f, v, d in zip(SW_FIELDS, s.sw, switches()) if v != d)
    return 'B%d-N%d-C%d-ld%d-k%d' % (s.B, s.N, s.C, s.ldx, s.k) + ('-off%d' % s.off if s.off else '') + \
        ('-ws_%s' % s.ws if s.ws != 'full' else '') + ('-res%d' % s.res if s.res else '') + ('-' + sw if sw else '')


def group_env(group):
    """the environment of a switch group's child process"""
    specs = GROUPS[group]
    assert len({s.sw for s in specs}) == 1, group
    env = {'GPE_DEBUG': '1'}
    env.update(('GPE_KNN_' + f, str(v)) for f, v, d in zip(SW_FIELDS, specs[0].sw, switches()) if v != d)
    return env


def passed_ws_bytes(s, total=None):
    """what the case passes as ws_bytes (0 with a NULL workspace); total: the library's gpe_knn_ws_bytes where the caller has asked it"""
    if s.ws == 'null':
        return 0
    return ws_layout(s.B, s.N, s.C)['need_f32'] if s.ws == 'f32' else ws_bytes(s.B, s.N, s.C, s.k) if total is None else total


def ws_offset(s):
    """bytes between the (256-byte aligned) allocation and the pointer the case passes"""
    return 8 if s.ws == 'mis8' else 0


def guard_floats(s):
    return (GUARD_ROWS * s.ldx + 63) & ~63


def x_offset_bytes(s):
    return 4 * (guard_floats(s) + s.off)


def call_of(s, x_base, ws_base, has_idx_glob=1, has_order_in=0, has_order_out=1, total=None):
    """the call the case makes when its x allocation starts at address x_base and its workspace allocation at ws_base"""
    ws = 0 if s.ws == 'null' else ws_base + ws_offset(s)
    return Call(x_base + x_offset_bytes(s), s.B, s.N, s.C, s.ldx, s.k, has_idx_glob, has_order_in, has_order_out, ws, passed_ws_bytes(s, total))


def case_plan(s, **flags):
    """(path, plan) of the case on the 256-CU device it was written for, allocations aligned to 256 bytes"""
    return plan(call_of(s, 1 << 20, 1 << 30, **flags), 256 - s.res, s.sw)


# ----------------------------------------------------------------------------------------------------------------------
# data, buffers, reference
# ----------------------------------------------------------------------------------------------------------------------
def seed_of(s, kind):
    return zlib.crc32(('%s/%s/%s' % (s.group, case_id(s), kind)).encode())


@functools.lru_cache(maxsize=None)
def table(s, kind):
    """the contiguous fp32 [B*N, C] table of the case"""
    N = s.N
    rng = np.random.default_rng(seed_of(s, kind))
    rows, C = s.B * N, s.C
    if kind == 'gauss':
        x = rng.standard_normal((rows, C))
    elif kind == 'offset':
        x = np.abs(rng.standard_normal((rows, C))) * 0.3 + 5.0 + rng.standard_normal((1, C))
    elif kind == 'clusters':
        x = (rng.standard_normal((8, C)) * 20)[rng.integers(0, 8, rows)] + 1e-2 * rng.standard_normal((rows, C))
    elif kind == 'lattice':
        x = rng.integers(0, 3, (rows, C)).astype(np.float64)
        x[:, 8:] = 0
    elif kind == 'same':
        x = np.full((rows, C), 0.3)
    elif kind == 'scales':
        x = rng.standard_normal((rows, C)) * 2.0 ** rng.integers(-20, 21, (rows, 1))
    elif kind == 'tiny':
        x = rng.standard_normal((rows, C)) * 2.0 ** -64
    elif kind == 'huge':
        x = rng.standard_normal((rows, C)) * 2.0 ** 55
    else:
        raise ValueError(kind)
    x = np.ascontiguousarray(x.astype(np.float32))
    assert np.isfinite(x).all()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(s, kind):
    """[B, N, k] int32: the oracle's graph of the case's table; computed once, shared, read-only"""
    import torch
    from oracle import ref_path as O
    ref = O.knn_local(torch.from_numpy(table(s, kind).copy()), s.B, s.k).numpy().astype(np.int32).reshape(s.B, s.N, s.k)
    ref.setflags(write=False)
    return ref


def garbage(s, kind):
    """the per-row values of the 'garbage' pad: large against the table, finite, distinct per row"""
    x = table(s, kind)
    amax = float(np.abs(x).max()) or 1.0
    r = np.arange(s.B * s.N)
    return (amax * (4.0 + (r * 7919 % 1013) / 64.0) * np.where(r & 1, -1.0, 1.0)).astype(np.float32)


Case = collections.namedtuple('Case', 'spec kind pad id x_buf ref')


def build(s, kind, pad='nan'):
    """the host image of the case's x allocation (flat fp32, NaN wherever a kernel must not read) and its reference"""
    assert pad in ('nan', 'garbage')
    x = table(s, kind)
    rows = s.B * s.N
    g = guard_floats(s)
    buf = np.full(g + s.off + rows * s.ldx + g, np.nan, np.float32)
    t = buf[g + s.off:g + s.off + rows * s.ldx].reshape(rows, s.ldx)
    t[:, :s.C] = x
    if pad == 'garbage' and s.ldx > s.C:
        t[:, s.C:] = garbage(s, kind)[:, None]
    return Case(s, kind, pad, '%s/%s/%s' % (case_id(s), kind, pad), buf, reference(s, kind))


def out_buffers(s):
    """{name: int32 host image}: idx, idx_glob [B N k] and order_out [B N], pre-filled, between sentinel zones"""
    def zoned(n):
        a = np.full(2 * ZONE + n, ZONE_VALUE, np.int32)
        a[ZONE:ZONE + n] = PREFILL
        return a
    return {'idx': zoned(s.B * s.N * s.k), 'idx_glob': zoned(s.B * s.N * s.k), 'order_out': zoned(s.B * s.N)}


STALE = 'stale'         # a workspace fill: 64-bit words alternating between the key (distance +0.0, point 1) and ~0, the empty slot
WS_FILLS = (0x00, 0xFF, STALE)


def ws_image(s, fill, total=None):
    """the host image of the workspace allocation: the pointer's offset, the passed bytes filled with `fill`, the sentinel tail.
    Neither uniform fill can show a scan that leaves the slots behind its keys unwritten: 0xFF bytes are the empty slot itself, and
    under any other uniform fill all 64 slots look valid, which sends the query to the exact redo.  STALE is what an earlier search
    leaves: valid keys behind empty slots."""
    n = ws_offset(s) + passed_ws_bytes(s, total)
    a = np.full(n + WS_TAIL, WS_TAIL_BYTE, np.uint8)
    if fill == STALE:
        words = np.empty(n // 8 + 2, np.uint64)
        words[0::2], words[1::2] = 1, 0xFFFFFFFFFFFFFFFF
        a[:n] = words.view(np.uint8)[8 - ws_offset(s) % 16:][:n] if ws_offset(s) % 16 else words.view(np.uint8)[:n]
    else:
        a[:n] = fill
    return a


def payload(a):
    return a[ZONE:len(a) - ZONE]


def check(case, out, path=None, ws=None, idx_glob=True, order=True):
    """every problem of a launch's output `out` ({name: host image as out_buffers lays it out}), [] when it is the defined answer.
    path: the path the launch took (the order is the identity everywhere but on the sorted cloud, a permutation per cloud there);
    ws: the workspace image after the launch."""
    s, ref = case.spec, case.ref
    bad = []
    for n, a in out.items():
        if not ((a[:ZONE] == ZONE_VALUE).all() and (a[-ZONE:] == ZONE_VALUE).all()):
            bad.append('%s: a sentinel zone of %s was written' % (case.id, n))
    idx = payload(out['idx']).reshape(s.B, s.N, s.k)
    if (idx < 0).any() or (idx >= s.N).any():
        bad.append('%s: idx holds %d values outside 0 .. N-1 (a pre-filled -7, a NaN or an empty key came through)'
                   % (case.id, int(((idx < 0) | (idx >= s.N)).sum())))
    diff = (idx != ref).any(-1)
    if diff.any():
        b, q = np.argwhere(diff)[0]
        bad.append('%s: %d / %d queries differ from the oracle, first (cloud %d, query %d): %s, oracle %s'
                   % (case.id, int(diff.sum()), s.B * s.N, b, q, idx[b, q].tolist(), ref[b, q].tolist()))
    if idx_glob:
        glob = payload(out['idx_glob']).reshape(s.B, s.N, s.k)
        if not np.array_equal(glob, ref + (np.arange(s.B, dtype=np.int32) * s.N)[:, None, None]):
            bad.append('%s: idx_glob is not the oracle + b N' % case.id)
    elif not (payload(out['idx_glob']) == PREFILL).all():
        bad.append('%s: idx_glob was written by a call that passed NULL' % case.id)
    oo = payload(out['order_out']).reshape(s.B, s.N)
    if not order:
        if not (oo == PREFILL).all():
            bad.append('%s: order_out was written by a call that passed NULL' % case.id)
    elif path == SORTED3:
        if not np.array_equal(np.sort(oo, 1), np.broadcast_to(np.arange(s.N, dtype=np.int32), (s.B, s.N))):
            bad.append('%s: order_out of the sorted cloud is not a permutation of 0 .. N-1 per cloud' % case.id)
    elif not np.array_equal(oo, np.broadcast_to(np.arange(s.N, dtype=np.int32), (s.B, s.N))):
        bad.append('%s: order_out is not the identity' % case.id)
    if ws is not None and not (ws[-WS_TAIL:] == WS_TAIL_BYTE).all():
        bad.append('%s: %d bytes behind the workspace were written' % (case.id, int((ws[-WS_TAIL:] != WS_TAIL_BYTE).sum())))
    return bad


def correct(case, path=ALLPAIRS):
    """the output images of a correct launch"""
    s = case.spec
    out = out_buffers(s)
    payload(out['idx'])[:] = case.ref.reshape(-1)
    payload(out['idx_glob'])[:] = (case.ref + (np.arange(s.B, dtype=np.int32) * s.N)[:, None, None]).reshape(-1)
    payload(out['order_out'])[:] = np.broadcast_to(np.arange(s.N, dtype=np.int32), (s.B, s.N)).reshape(-1)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# wrong variants: what a plausibly broken kernel returns.  Each gives output images, or None where it cannot change this case.
# ----------------------------------------------------------------------------------------------------------------------
def chain_sqdist(x):
    """[N, C] fp32 -> [N, N] fp32 squared distances by the defined chain (the oracle's own arithmetic)"""
    import torch
    from oracle import ref_path as O
    return O.sqdist_one_cloud(torch.from_numpy(np.array(x, np.float32))).numpy()


def topk_of(d, k):
    """[Nq, N] distances -> [Nq, k] indices ascending by (distance, index)"""
    return np.argsort(d, axis=1, kind='stable')[:, :k].astype(np.int32)


def _from_idx(case, idx, glob=None):
    s = case.spec
    out = correct(case)
    payload(out['idx'])[:] = idx.reshape(-1)
    payload(out['idx_glob'])[:] = (idx + (np.arange(s.B, dtype=np.int32) * s.N)[:, None, None] if glob is None else glob).reshape(-1)
    return out


def gemm_form_topk(x, k):
    """top-k by the fp32 GEMM-form distance |q|^2 + |p|^2 - 2 q.p, without a recheck"""
    n = (x * x).sum(1, dtype=np.float32)
    d = (n[:, None] + n[None, :]) - np.float32(2) * (x @ x.T).astype(np.float32)
    return topk_of(d.astype(np.float32), k)


def wrong(case, name):
    s, ref, N = case.spec, case.ref, case.spec.N
    x = table(s, case.kind).reshape(s.B, N, s.C)
    idx = ref.copy()
    if name == 'swap_ties':                                 # two equal-distance neighbours swapped (the higher index first)
        for b in range(s.B):
            d = chain_sqdist(x[b])
            dd = np.take_along_axis(d, ref[b].astype(np.int64), 1)
            q, j = np.nonzero(dd[:, 1:] == dd[:, :-1])
            if len(q):
                idx[b, q[0], [j[0], j[0] + 1]] = idx[b, q[0], [j[0] + 1, j[0]]]
                return _from_idx(case, idx)
        return None
    if name == 'kth_is_next':                               # the k-th neighbour replaced by the (k+1)-th
        if s.k >= N:
            return None
        full = topk_of(chain_sqdist(x[0]), s.k + 1)
        assert np.array_equal(full[:, :s.k], ref[0])
        idx[0, :, s.k - 1] = full[:, s.k]
        return _from_idx(case, idx)
    if name == 'row_unsorted':
        if s.k < 2:
            return None
        q = N // 2
        idx[s.B - 1, q] = idx[s.B - 1, q, ::-1]
        return _from_idx(case, idx)
    if name == 'next_cloud':                                # cloud 0's queries searched in the next cloud's table
        if s.B < 2:
            return None
        idx[0] = topk_of(chain_sqdist(np.concatenate([x[0], x[1]]))[:N, N:], s.k)
        return _from_idx(case, idx) if (idx[0] != ref[0]).any() else None
    if name == 'glob_no_offset':
        if s.B < 2:
            return None
        return _from_idx(case, idx, glob=idx)
    if name == 'pad_column':                                # the reference over C + 1 columns of the garbage-padded buffer
        if s.ldx <= s.C:
            return None
        import torch
        from oracle import ref_path as O
        xx = np.concatenate([x.reshape(-1, s.C), garbage(s, case.kind)[:, None]], 1)
        got = O.knn_local(torch.from_numpy(xx), s.B, s.k).numpy().astype(np.int32).reshape(s.B, N, s.k)
        return _from_idx(case, got)
    if name == 'no_recheck':
        return _from_idx(case, np.stack([gemm_form_topk(x[b], s.k) for b in range(s.B)]))
    raise ValueError(name)


WRONG = ('swap_ties', 'kth_is_next', 'row_unsorted', 'next_cloud', 'glob_no_offset', 'pad_column', 'no_recheck')

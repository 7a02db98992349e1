"""not-gpu: the host restatement of the balanced batch schedule (tests/batch_schedule_restate.py, the yardstick of
tests/test_gpu_epoch_feed.py) — its invariants, the reference's quota expression, its distribution against the counts recorded from
the reference's BalancedBatchSampler (tests/golden/batch_schedule_small.pt, scripts/make_batch_schedule_golden.py) — and what
include/gpe_hip_feed.h promises without a GPU: the header binds through _lib.FEED_HEADERS, the symbols are exported, the host-only
sizes, and -22 on every documented bad argument.

The statistical bars are the 0.9999 chi-square quantiles (Wilson-Hilferty, stitch_sample_restate.chi2_quantile), one per table
(batch_schedule_restate.statistics).  Both sides are deterministic — recorded counts; seed 0, epochs 0 .. 1999, fixed before the
first run — so a test either always passes or always fails, and a failure means the restatement differs from the reference."""
import ctypes
import os

import numpy as np
import pytest
import torch

import batch_schedule_restate as R
import stitch_sample_restate as S

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
SIZES = [7, 5, 1, 11]
# (class sizes, batch size, drop_last): the shapes tests/test_gpu_epoch_feed.py draws on the device as well
CASES = [(SIZES, B, dl) for B in (4, 5, 24) for dl in (True, False)] + [([13, 10], 23, True), ([24], 5, False)]


def class_lists(sizes, first=0, step=1):
    """the ids of every class: consecutive multiples of `step` from `first` on, in class order"""
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [[first + step * g for g in range(int(off[c]), int(off[c + 1]))] for c in range(len(sizes))]


@pytest.fixture(scope='module')
def recorded():
    return torch.load(os.path.join(GOLDEN, 'batch_schedule_small.pt'), weights_only=False)


@pytest.mark.parametrize('sizes, B, drop_last', CASES)
def test_restatement_invariants(sizes, B, drop_last):
    lists = class_lists(sizes, first=3, step=2)
    G, quota = sum(sizes), R.quotas(sizes, B)
    class_of = {g: c for c, l in enumerate(lists) for g in l}
    d = R.draw(lists, quota, B, drop_last, 0x5eed, 3)
    table, blen = d['table'], d['batch_len']
    rows = G // B + (1 if (not drop_last and G % B) else 0)
    assert table.shape == (rows, B) and blen.tolist() == [B] * (G // B) + ([G % B] if rows > G // B else [])
    seen = [int(g) for t in range(rows) for g in table[t, :blen[t]]]
    assert len(set(seen)) == len(seen) and set(seen) <= set(class_of)              # at most once per epoch
    if not drop_last or G % B == 0:
        assert sorted(seen) == sorted(class_of)                                      # exactly once when the remainder is kept
    assert all((table[t, blen[t]:] == -1).all() for t in range(rows))
    left = list(sizes)
    for t in range(G // B):
        assert len(set(table[t].tolist())) == B                                      # full rows hold B distinct ids
        counts = [0] * len(sizes)
        for g in table[t]:
            counts[class_of[int(g)]] += 1
        assert (d['classes'][t] == [class_of[int(g)] for g in table[t]]).all()
        for c in range(len(sizes)):
            left[c] -= counts[c]
            assert counts[c] >= quota[c] or left[c] == 0, (t, c, counts, quota)       # the quota, unless the class ran out
    assert sorted(d['pre'][0].tolist()) == sorted(table[0].tolist())
    again, other = R.draw(lists, quota, B, drop_last, 0x5eed, 3), R.draw(lists, quota, B, drop_last, 0x5eed, 4)
    assert (again['table'] == table).all() and (again['batch_len'] == blen).all()     # the same (seed, epoch) reproduces
    assert (other['table'] != table).any()                                            # two epochs differ
    assert (R.draw(lists, quota, B, drop_last, 0x5eee, 3)['table'] != table).any()


def test_exhausted_class_path_is_taken():
    """quotas (1, 1, 0, 2) at B = 5: class 1 has five garments and every batch takes at least one, so some epochs leave it empty
    before the last batch, whose quota it then cannot fill (the reference's `break`; its recorded run shows the same)"""
    lists, quota = class_lists(SIZES), R.quotas(SIZES, 5)
    short = 0
    for epoch in range(200):
        cls = R.draw(lists, quota, 5, True, 0, epoch)['classes']
        short += sum(1 for t in range(4) for c in range(4) if (cls[t] == c).sum() < quota[c])
    assert short > 0


def test_quotas_are_the_references_expression(recorded):
    from gpe_amd import staging
    for sizes, B, _ in CASES:
        G = sum(sizes)
        want = [int((n / G) * B) for n in sizes]
        assert staging.balanced_quotas(sizes, B) == want == R.quotas(sizes, B)
        assert sum(want) <= B
    assert staging.balanced_quotas([13, 10], 23) == [12, 10] and 13 * 23 // 23 == 13           # not the integer expression
    for B, rec in recorded['settings'].items():
        assert staging.balanced_quotas(recorded['sizes'], B) == list(rec['quotas'])               # what the reference computed


def _restated_counts(rec, B):
    lists = class_lists(SIZES)
    class_of = {g: c for c, l in enumerate(lists) for g in l}
    counts = R.Counts(len(SIZES), B, int(rec['rows']))
    quota = R.quotas(SIZES, B)
    for epoch in range(int(rec['N'])):
        table = R.draw(lists, quota, B, True, 0, epoch)['table']
        counts.add([r.tolist() for r in table], class_of, [l[0] for l in lists])
    return counts


@pytest.mark.parametrize('B', [5, 4])
def test_restatement_follows_the_references_recorded_counts(recorded, B):
    assert recorded['sizes'] == SIZES and recorded['watched'] == [l[0] for l in class_lists(SIZES)]
    rec = recorded['settings'][B]
    assert int(rec['N']) == 2000 and int(rec['rows']) == sum(SIZES) // B
    ref = R.Counts.from_recorded(rec)
    assert sum(ref.comp.values()) == ref.N * ref.rows and (ref.batch_of.sum(axis=1) == ref.N).all()
    stats = R.statistics(_restated_counts(rec, B), ref)
    assert len(stats) >= ref.rows + 2 * 3
    failed = []
    for k, (x, df) in stats.items():
        bar = S.chi2_quantile(df, 0.9999)
        print('B = %d  %-24s chi-square %8.2f on %3d degrees of freedom, bar %8.2f' % (B, k, x, df, bar))
        if not x < bar:
            failed.append(k)
    assert failed == []


def test_two_sample_statistic():
    assert R.two_sample([100, 200, 300], [100, 200, 300]) == (0.0, 2)
    x, df = R.two_sample([100, 200, 300, 1, 2], [110, 190, 300, 3, 0])               # the two small cells are pooled into one
    assert df == 3 and abs(x - (100 / 210 + 100 / 390 + 0.0)) < 1e-12
    x, df = R.two_sample([50, 50], [100, 300])                                        # unequal totals: K = 2
    assert df == 1 and abs(x - ((100 - 50) ** 2 / 150 + (100 - 150) ** 2 / 350)) < 1e-9


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------------

def test_feed_header_binds():
    from gpe_amd import _lib
    assert _lib.FEED_HEADERS == (_lib.FEED_HEADER_PATH,) and os.path.basename(_lib.FEED_HEADER_PATH) == 'gpe_hip_feed.h'
    sigs = _lib.parse_header(_lib.FEED_HEADER_PATH)
    assert sigs == {'gpe_batch_schedule_rows': ('l', ['l', 'i', 'i']),
                    'gpe_batch_schedule_ws_bytes': ('l', ['l']),
                    'gpe_batch_schedule_draw': ('i', ['p'] * 5 + ['i'] * 4 + ['p', 'p', 'l', 'p', 'p', 'p']),
                    'gpe_feed_jobs': ('i', ['i', 'p', 'p', 'p', 'p']),
                    'gpe_feed_next': ('i', ['p', 'l', 'i', 'p', 'i', 'p', 'i', 'l', 'p', 'p', 'p'])}
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in sigs:
        assert hasattr(raw, name), 'libgpe_hip.so does not export %s' % name
    for h in _lib.HEADERS + _lib.FEATURE_HEADERS + _lib.EVAL_HEADERS + _lib.PLACE_HEADERS + _lib.FRAMEWORK_HEADERS:
        assert not set(sigs) & set(_lib.parse_header(h))                              # declared once
    l = _lib.lib()
    assert l.gpe_feed_next.argtypes[1] is ctypes.c_long and l.gpe_batch_schedule_rows.restype is ctypes.c_long
    assert l.gpe_abi_version() == 7


def test_host_only_sizes():
    from gpe_amd import _lib
    l = _lib.lib()
    for G, B in ((24, 5), (24, 4), (24, 24), (23, 23), (3, 5), (19236, 30), (1 << 20, 1024), (1, 1)):
        assert l.gpe_batch_schedule_rows(G, B, 1) == G // B
        assert l.gpe_batch_schedule_rows(G, B, 0) == G // B + (1 if G % B else 0)
    for G, B in ((0, 5), ((1 << 20) + 1, 5), (24, 0), (24, 1025), (-1, 5)):
        assert l.gpe_batch_schedule_rows(G, B, 1) == -22
    for G in (1, 24, 19236, 1 << 20):
        n = l.gpe_batch_schedule_ws_bytes(G)
        assert n >= 4 * G + 16 and n % 16 == 0 and n <= 4 * G + 64
    assert l.gpe_batch_schedule_ws_bytes(0) == -22 and l.gpe_batch_schedule_ws_bytes((1 << 20) + 1) == -22


def test_schedule_draw_rejects_bad_arguments_without_a_gpu():
    from gpe_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    i32 = lambda v: np.asarray(v, dtype=np.int32)                                    # noqa: E731
    off, quota = i32([0, 7, 12, 13, 24]), i32([1, 1, 0, 2])
    good = dict(class_off=p, ids=p, quota=p, off_h=off, quota_h=quota, C=4, G=24, B=5, drop_last=1, state=p, ws=p, ws_bytes=1 << 15,
                table=p, batch_len=p)

    def call(**kw):
        a = dict(good, **kw)
        h = lambda v: None if v is None else v.ctypes.data                           # noqa: E731
        return l.gpe_batch_schedule_draw(a['class_off'], a['ids'], a['quota'], h(a['off_h']), h(a['quota_h']), a['C'], a['G'], a['B'],
                                         a['drop_last'], a['state'], a['ws'], a['ws_bytes'], a['table'], a['batch_len'], None)
    for name in ('class_off', 'ids', 'quota', 'off_h', 'quota_h', 'state', 'ws', 'table', 'batch_len'):
        assert call(**{name: None}) == -22, name
    assert call(B=3) == -22                                                           # C > B: the reference's NotImplementedError
    assert call(quota_h=i32([1, 1, 1, 3])) == -22                                     # quota sum 6 > B = 5
    assert call(quota_h=i32([1, 1, -1, 2])) == -22
    assert call(G=0) == -22 and call(G=(1 << 20) + 1) == -22 and call(G=25) == -22    # (class_off[C] != G)
    assert call(B=0) == -22 and call(B=1025) == -22 and call(C=0) == -22
    assert call(off_h=i32([0, 7, 6, 13, 24])) == -22 and call(off_h=i32([1, 7, 12, 13, 24])) == -22
    assert call(drop_last=2) == -22
    assert call(ws_bytes=l.gpe_batch_schedule_ws_bytes(24) - 1) == -22 and call(ws=p + 4) == -22 and call(state=p + 4) == -22


def test_feed_rejects_bad_arguments_without_a_gpu():
    from gpe_amd import _lib
    l = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    jobs = np.zeros((17, 3), dtype=np.int64)

    def fill(T, nb, src=p, dst=p + 512):
        ptrs = lambda a: (ctypes.c_void_p * max(T, 1))(*([a] * max(T, 1)))          # noqa: E731
        return l.gpe_feed_jobs(T, ptrs(src), ptrs(dst), (ctypes.c_long * max(T, 1))(*([nb] * max(T, 1))), jobs.ctypes.data)
    assert fill(3, 2576) == 0 and jobs[:3].tolist() == [[p, p + 512, 2576]] * 3 and not jobs[3:].any()
    assert fill(16, 4) == 0
    assert fill(17, 4) == -22 and fill(0, 4) == -22                                   # T > 16
    for nb in (0, 2, 6, 23, -4, (1 << 24) + 4):                                       # misaligned row_bytes
        assert fill(1, nb) == -22, nb
    assert fill(1, 8, src=p + 2) == -22 and fill(1, 8, dst=p + 1) == -22 and fill(1, 8, src=None) == -22
    assert l.gpe_feed_jobs(1, None, None, None, None) == -22

    good = dict(table=p, rows=4, B=5, cursor=p, G=24, jobs=p, T=3, nb=2576, index=p, status=p)

    def call(**kw):
        a = dict(good, **kw)
        return l.gpe_feed_next(a['table'], a['rows'], a['B'], a['cursor'], a['G'], a['jobs'], a['T'], a['nb'], a['index'], a['status'], None)
    for name in ('table', 'cursor', 'jobs', 'index', 'status'):
        assert call(**{name: None}) == -22, name
    assert call(T=17) == -22 and call(T=-1) == -22
    assert call(nb=2578) == -22 and call(nb=0) == -22
    assert call(rows=0) == -22 and call(B=0) == -22 and call(B=1025) == -22 and call(G=0) == -22
    assert call(cursor=p + 4) == -22 and call(jobs=p + 4) == -22


def test_schedule_and_feeder_check_before_the_device():
    from gpe_amd import staging
    ids = {'a': torch.arange(0, 7), 'b': [7, 8, 9, 10, 11], 'c': np.asarray([12]), 'd': torch.arange(13, 24)}
    with pytest.raises(NotImplementedError):
        staging.BalancedBatchSchedule(ids, 3)
    with pytest.raises(ValueError, match='do not fill one batch'):
        staging.BalancedBatchSchedule({'a': [0, 1, 2]}, 5)
    with pytest.raises(ValueError):
        staging.BalancedBatchSchedule({'a': [0.5, 1.0]}, 1)
    with pytest.raises(ValueError, match='2\\^31'):
        staging.BalancedBatchSchedule({'a': [0, -1]}, 1)
    with pytest.raises(RuntimeError, match='no CPU path'):
        staging.BalancedBatchSchedule(ids, 5, device='cpu')

"""-m gpu: the graph search rung by rung through the C ABI (gpe_knn, never ops.knn: its cached workspace and its own size query are
what this file must not depend on) against the oracle's graph.  Cases, buffers, the reference and the checker are in
tests/knn_restate.py, and tests/test_knn_host.py checks them on the CPU first (the restated plan is the library's, the list reaches
every path and kernel instance, the data would expose a missing recheck, every wrong variant is rejected).

Per case and data kind, with the pad columns of x once NaN and once large finite garbage, guard floats of NaN around the table and
the table at the case's base offset:
  - gpe_knn_path, asked with the device's own pointers and switches = NULL, names the rung and the kernel instance the case was
    written for, and its plan is the restated one;
  - the search runs on a workspace filled with 0x00 bytes, on one filled with 0xFF bytes and on one that holds stale keys between empty
    slots (what an earlier search leaves), the outputs pre-filled afresh each time: idx equals the oracle on every query,
    idx_glob = idx + b N, the runs are bit-identical in both;
  - order_out is the identity on every path but the sorted cloud, where it is a permutation of 0 .. N-1 per cloud (its bits are not
    compared between runs: the order inside a Morton cell follows the atomics);
  - a call with idx_glob = NULL and order_out = NULL gives the same idx and leaves both buffers alone;
  - on the scan and list rungs a call with a random permutation per cloud as order_in gives the same idx;
  - every sentinel is intact: around idx, idx_glob and order_out and behind the bytes of workspace the call was given; no pre-filled
    value, NaN-born or negative index comes through.
The CU reservation is restored in `finally`.  Each switch group is one test and one child process (GPE_DEBUG=1 and the group's
GPE_KNN_* variables, read once per process) that runs the group's cases with the same checks, prints one line per case and exits
non-zero at the first failure; after a failed child no other is started.

Rungs, instances, timings and findings on an MI355X: profiles/knn_tests.md."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import knn_restate as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpe():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    import gpe_amd
    return gpe_amd


def _plan(L, s, c):
    out = (ctypes.c_long * len(R.PLAN_FIELDS))()
    path = L.query('gpe_knn_path', c.x, c.B, c.N, c.C, c.ldx, c.k, c.has_idx_glob, c.has_order_in, c.has_order_out, c.ws or None, c.ws_bytes,
                   None, ctypes.addressof(out))
    return path, dict(zip(R.PLAN_FIELDS, out))


def _launch(L, s, case, xd, fill, usable, glob=True, order=True, hint=None):
    """one gpe_knn call on freshly pre-filled outputs and a freshly filled workspace -> (path, plan, output images, workspace tail)"""
    dev = {n: torch.from_numpy(a).cuda() for n, a in R.out_buffers(s).items()}
    total = L.query('gpe_knn_ws_bytes', s.B, s.N, s.C, s.k)         # the library's own answer sizes the workspace, as a caller's would
    ws_t = torch.from_numpy(R.ws_image(s, fill, total)).cuda()
    assert xd.data_ptr() % 256 == 0 and ws_t.data_ptr() % 256 == 0
    ptr = lambda n: dev[n].data_ptr() + 4 * R.ZONE
    c = R.call_of(s, xd.data_ptr(), ws_t.data_ptr(), has_idx_glob=int(glob), has_order_in=int(hint is not None), has_order_out=int(order),
                  total=total)
    path, pl = _plan(L, s, c)
    assert (path, pl) == R.plan(c, usable, s.sw), '%s: gpe_knn_path and the restated plan differ: %r' % (case.id, (path, pl))
    L.call('gpe_knn', c.x, s.B, s.N, s.C, s.ldx, s.k, ptr('idx'), ptr('idx_glob') if glob else None, hint, ptr('order_out') if order else None,
           c.ws or None, c.ws_bytes)
    torch.cuda.synchronize()
    return path, pl, {n: t.cpu().numpy() for n, t in dev.items()}, ws_t[-R.WS_TAIL:].cpu().numpy()


def run_case(gpe, s, kind):
    """every check of the module docstring on one case and data kind -> the line to report"""
    L = gpe._lib
    usable = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count - s.res
    saved = L.get_reserved_cus()
    try:
        L.query('gpe_reserve_cus_set', s.res)
        first = None
        for pad in (('nan', 'garbage') if s.ldx > s.C else ('nan',)):
            case = R.build(s, kind, pad)
            xd = torch.from_numpy(case.x_buf).cuda()
            for fill in R.WS_FILLS:
                what = '%s, workspace filled with %s' % (case.id, fill if fill == R.STALE else '0x%02X' % fill)
                path, pl, out, tail = _launch(L, s, case, xd, fill, usable)
                assert path == s.rung, '%s: gpe_knn_path says path %d, the case was written for %d' % (what, path, s.rung)
                assert R.main_instance(path, pl) == s.main, '%s: %s runs, the case was written for %s' % (what, R.instance(path, pl), s.main)
                bad = R.check(case, out, path=path, ws=tail)
                assert not bad, what + ': ' + '; '.join(bad)
                if first is None:
                    first = out
                assert all(out[n].tobytes() == first[n].tobytes() for n in ('idx', 'idx_glob')), what + ': differs from the first run'
            p2, _, out, tail = _launch(L, s, case, xd, 0xFF, usable, glob=False, order=False)
            bad = R.check(case, out, path=p2, ws=tail, idx_glob=False, order=False)
            assert p2 == path and not bad, '%s without idx_glob and order_out: %s' % (case.id, '; '.join(bad))
            if path in (R.SCAN, R.LISTS):
                rng = np.random.default_rng(R.seed_of(s, kind) ^ 0x5bd1)
                hint = torch.from_numpy(np.stack([rng.permutation(s.N) for _ in range(s.B)]).astype(np.int32)).cuda()
                p3, pl3, out, tail = _launch(L, s, case, xd, 0xFF, usable, hint=hint)
                assert p3 == path and pl3['order'] == (0 if s.group == 'NOORDER' else 1), case.id
                bad = R.check(case, out, path=p3, ws=tail)
                assert not bad, '%s with an order hint: %s' % (case.id, '; '.join(bad))
    finally:
        L.query('gpe_reserve_cus_set', saved)
    return 'knn[%s/%s] path %d (%s): %s' % (R.case_id(s), kind, path, R.PATH_NAMES[path], ' + '.join(R.instance(path, pl)))


def _cases(rung):
    return pytest.mark.parametrize('spec', R.DEFAULT_BY_RUNG[rung], ids=R.case_id)


def _all_kinds(gpe, spec):
    for kind in spec.kinds:
        print(run_case(gpe, spec, kind))


@_cases('allpairs')
def test_knn_all_pairs(gpe, spec):
    """path 2 (gpe_knn_kernel<4 | 2 | 1> and its C <= 4 instance): every staging width by C, by the pitch and by the base address, next
    to NaN and garbage pads; N = 1, k = N, k = 64, wide rows with k > 48 in one, two and eight chunks; 63, 64, 65 and 130 queries; the
    fall-backs from the sorted cloud (misaligned or NULL workspace) and from the filter group (step 2a)."""
    _all_kinds(gpe, spec)


@_cases('sorted')
def test_knn_sorted_cloud(gpe, spec):
    """path 1 (gpe_knn3_sort_kernel + gpe_knn3_query_kernel): 128, 129, 577 and 8192 points at pitches 3 and 4, k up to 64, nine clouds."""
    _all_kinds(gpe, spec)


@_cases('scan')
def test_knn_threshold_scan(gpe, spec):
    """path 3 (gpe_knn_ft_kernel<4 | 8> + gpe_knn_rerank2_kernel): C = 16 .. 160 with k = 1, 5 and 32, an odd number of queries, base
    offsets 1 and 2, the 128-query workgroup on 64 usable CUs."""
    _all_kinds(gpe, spec)


@_cases('lists')
def test_knn_ordered_lists(gpe, spec):
    """path 4 (gpe_knn_h3_kernel<2 | 5 | 8> + gpe_knn_rerank_kernel): k = 33 .. 48 on narrow rows, C = 161, 200 and 256."""
    _all_kinds(gpe, spec)


@_cases('f32filter')
def test_knn_fp32_filter(gpe, spec):
    """path 5 (gpe_knn_mfma_kernel<4 | 2 | 1> + gpe_knn_rerank_kernel): C = 257 at pitches 257, 258 and 260, C = 300 at base offsets 1
    and 2, and C <= 256 on a workspace of need_f32 bytes, where the fp16-pipe filters are silently off."""
    _all_kinds(gpe, spec)


# ----------------------------------------------------------------------------------------------------------------------
# switch groups: one child process each
# ----------------------------------------------------------------------------------------------------------------------
def child_main(group):
    import gpe_amd
    for s in R.GROUPS[group]:
        for kind in s.kinds:
            try:
                print(run_case(gpe_amd, s, kind), flush=True)
            except Exception as e:                          # the first failure ends the child
                print('FAILED knn[%s/%s]: %s: %s' % (R.case_id(s), kind, type(e).__name__, e), flush=True)
                sys.exit(1)
    print('group %s ok' % group, flush=True)


_CHILD = '''
import sys
sys.path[:0] = [%r, %r]
import test_gpu_knn
test_gpu_knn.child_main(%r)
'''
_child_failed = []


@pytest.mark.parametrize('group', [g for g in R.GROUPS if g != 'default'])
def test_knn_switch_group(gpe, group, tmp_path):
    """the group's cases under its GPE_KNN_* variables; gpe_knn_path with switches = NULL must name each case's rung in that process"""
    if _child_failed:
        pytest.fail('not started: the child of group %s failed before' % _child_failed[0])
    here = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / 'child.py'
    script.write_text(_CHILD % (os.path.dirname(here), here, group))
    try:
        r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, **R.group_env(group)), capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _child_failed.append(group)
        raise
    print(r.stdout)
    if r.returncode != 0 or 'group %s ok' % group not in r.stdout:
        _child_failed.append(group)
    assert r.returncode == 0 and 'group %s ok' % group in r.stdout, 'exit %d\n%s\n%s' % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])

"""A numpy restatement of the reference's evaluation rule (nn/metrics/eval_utils.py:35-76, `_eval_metrics_per_loader`) and of the gate
table that decides a quality key's None (composed_loss.py:365-424, as gpe_amd.metrics applies it).  Not a test: a helper of
tests/test_eval_host.py and tests/test_gpu_eval.py.

The rule: 'full_loss' and every key of a batch's loss dict get a list; a value that is None is not appended; the result per key is
sum(list) / len(list), None for an empty list (a key that was never present with a value).  The values are 0-d float32 arrays, so
`sum` is a sequential float32 add in list order starting from the integer 0, and the division a float32 one."""
import numpy as np

# key -> which of the quality kernels' contributor counts (counts[0] patterns with the right panel count, [1] panels in them, [2]
# those with detected stitches, [3] all panels with a shape) must be positive for the key to have a value in a batch
GATES = {'corr_panel_shape_l2': 1, 'corr_rotation_l2': 0, 'corr_translation_l2': 0, 'corr_stitch_precision': 2,
         'corr_stitch_recall': 2}


def f32(v):
    """a batch's value as the reference sees it: value.cpu().numpy() of a float32 tensor, or the number itself"""
    if hasattr(v, 'detach'):
        v = v.detach().cpu().numpy()
    return np.float32(v)


def gate(key, value, counts, gates=GATES):
    """the value of `key` in a batch whose contributor counts are `counts` (None: no gated key has a value)"""
    j = gates.get(key)
    if j is None:
        return value
    return value if counts is not None and counts[j] > 0 else None


def aggregate(batches):
    """batches: per batch (full_loss, loss dict) -> the dict _eval_metrics_per_loader returns, keys in its order"""
    lists = {'full_loss': []}
    for full_loss, loss_dict in batches:
        lists['full_loss'].append(f32(full_loss))
        for key, value in loss_dict.items():
            lists.setdefault(key, [])
            if value is not None:
                lists[key].append(f32(value))
    out = {}
    with np.errstate(all='ignore'):
        for key, values in lists.items():
            if not values:
                out[key] = None
                continue
            s = np.float32(0)
            for v in values:
                s = np.float32(s + v)
            out[key] = np.float32(s / np.float32(len(values)))
    return out


def sums(batches):
    """-> ({key: float32 running sum}, {key: count}) of aggregate's lists (what the accumulator keeps on the device)"""
    s, n = {}, {}
    with np.errstate(all='ignore'):
        for full_loss, loss_dict in batches:
            for key, value in [('full_loss', full_loss)] + list(loss_dict.items()):
                s.setdefault(key, np.float32(0))
                n.setdefault(key, 0)
                if value is not None:
                    s[key] = np.float32(s[key] + f32(value))
                    n[key] += 1
    return s, n


def same(a, b):
    """bit equality of two results of the rule (None matches None only; a NaN matches any NaN: which payload an add hands on is
    the processor's choice, not the rule's)"""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.float32(a), np.float32(b)
    return bool(a.view(np.int32) == b.view(np.int32) or (np.isnan(a) and np.isnan(b)))


def assert_same(got, want, what=''):
    assert list(got) == list(want), (what, list(got), list(want))
    for k in want:
        assert same(got[k], want[k]), (what, k, got[k], want[k])

"""fp64 restatement of stitch recovery from the edge-pair classifier — what the reference does at prediction time with
NNSewingPattern.all_edge_pairs + stitches_from_pair_classifier (nn/data/pattern_converter.py:411-499) — as plain numpy / python:
the specification ops.stitch_pairs is tested against (tests/test_gpu_stitch_pairs.py) and, with reference_indexing=True, a
transcription that must reproduce the reference's recorded output exactly (tests/test_stitch_pairs_host.py).

A garment is (edges [P, L, Fe], num_edges [P]); panel slots with num_edges == 0 are absent and the panel order is the slot order
of the present ones.  A pair is the tuple (i, j, r, c): edge r of panel slot i with edge c of panel slot j, i < j.

reference_indexing: pattern_converter.py:432 reads pairs_mapping[stitch_idx] where pairs_mapping[stitched_ids[stitch_idx]] is
meant, so the reference names its n-th positive after the n-th pair of the enumeration (and selects on those names).  True
reproduces that, False is the intended indexing = the product's specification.
"""
import numpy as np
import torch


def enumerate_pairs(num_edges):
    """the reference's enumeration (:471-490): panels i < j in panel order, then rows, then columns"""
    present = [p for p, n in enumerate(num_edges) if n > 0]
    out = []
    for a, i in enumerate(present):
        for j in present[a + 1:]:
            for r in range(int(num_edges[i])):
                for c in range(int(num_edges[j])):
                    out.append((i, j, r, c))
    return out


def pair_rows(edges, pairs):
    """[N, 2 Fe] fp64 un-standardised rows [e_i | e_j]"""
    e = np.asarray(edges, dtype=np.float64)
    if not pairs:
        return np.zeros((0, 2 * e.shape[-1]))
    idx = np.asarray(pairs)
    return np.concatenate([e[idx[:, 0], idx[:, 2]], e[idx[:, 1], idx[:, 3]]], axis=1)


def logits64(state_dict, rows, f_shift, f_scale):
    """eval-mode MLP = [Linear -> ReLU -> BatchNorm1d(running statistics)] x blocks (nn/net_blocks.py:43-47) on the standardised
    rows, in fp64"""
    x = (np.asarray(rows, dtype=np.float64) - np.asarray(f_shift, dtype=np.float64)) / np.asarray(f_scale, dtype=np.float64)
    sd = {k: v.detach().cpu().double().numpy() for k, v in state_dict.items() if torch.is_tensor(v) and v.dim() > 0}
    l = 0
    while 'mlp.%d.0.weight' % l in sd:
        x = np.maximum(x @ sd['mlp.%d.0.weight' % l].T + sd['mlp.%d.0.bias' % l], 0.0)
        x = (x - sd['mlp.%d.2.running_mean' % l]) / np.sqrt(sd['mlp.%d.2.running_var' % l] + 1e-5) * sd['mlp.%d.2.weight' % l] \
            + sd['mlp.%d.2.bias' % l]
        l += 1
    return x[:, 0]


def positives(logits):
    """indices with round(sigmoid(logit)) == 1 in fp32 (:425-429)"""
    t = torch.as_tensor(np.asarray(logits), dtype=torch.float32)
    return torch.round(torch.sigmoid(t)).nonzero(as_tuple=False).view(-1).tolist()


def named_positives(pairs, logits, reference_indexing):
    """the stitch list before the selection, in list order: [((i, j, r, c), score)]"""
    ids = positives(logits)
    return [(tuple(pairs[n if reference_indexing else k]), float(logits[k])) for n, k in enumerate(ids)]


def _edges_of(pair):
    i, j, r, c = pair
    return (i, r), (j, c)


def select_argmax(entries):
    """an entry survives iff on both of its edges it is the maximum of (score, earlier list position) over the entries touching
    that edge"""
    best = {}
    for pos, (pair, score) in enumerate(entries):
        for e in _edges_of(pair):
            if e not in best or score > entries[best[e]][1]:
                best[e] = pos
    return [en for pos, en in enumerate(entries) if all(best[e] == pos for e in _edges_of(en[0]))]


def select_loop(entries):
    """the reference's double loop (:440-456), literally: marks against the full list, the lower score loses, the later one on equal
    scores"""
    to_remove = set()
    for base in range(len(entries)):
        for base_edge in _edges_of(entries[base][0]):
            for other in range(base + 1, len(entries)):
                o0, o1 = _edges_of(entries[other][0])
                if base_edge == o0 or base_edge == o1:
                    to_remove.add(base if entries[base][1] < entries[other][1] else other)
    return [en for pos, en in enumerate(entries) if pos not in to_remove]


def stitches(pairs, logits, reference_indexing=False, loop=False):
    """-> surviving [((i, j, r, c), score)] in list order (= ascending order key with the intended indexing)"""
    entries = named_positives(pairs, logits, reference_indexing)
    return select_loop(entries) if loop else select_argmax(entries)


def as_tensors(survivors, P, L):
    """the product's output format for one garment: stitches int32 [2, S] of edge ids panel * L + edge, count, scores [S]"""
    S = P * L // 2
    st = np.zeros((2, S), dtype=np.int32)
    sc = np.zeros(S, dtype=np.float64)
    for n, ((i, j, r, c), score) in enumerate(survivors):
        st[0, n], st[1, n], sc[n] = i * L + r, j * L + c, score
    return st, len(survivors), sc


def dense_to_list(dense, pairs, L):
    """the product's dense logits [E, E] read in enumeration order"""
    idx = np.asarray(pairs)
    return np.asarray(dense)[idx[:, 0] * L + idx[:, 2], idx[:, 1] * L + idx[:, 3]]


def margins(pairs, logits):
    """(smallest |logit|, smallest gap between the two best positives of an edge); inf where there is nothing to compare"""
    lg = np.asarray(logits, dtype=np.float64)
    m0 = float(np.abs(lg).min()) if len(lg) else float('inf')
    per_edge = {}
    for k in np.nonzero(lg > 0)[0]:
        for e in _edges_of(pairs[k]):
            per_edge.setdefault(e, []).append(lg[k])
    gap = float('inf')
    for v in per_edge.values():
        if len(v) > 1:
            v = sorted(v)
            gap = min(gap, v[-1] - v[-2])
    return m0, gap


def tol_of(logits):
    """the logit bar of test_stitch_model_known_answer (tests/test_gpu_kernels.py): 1e-4 * max(1, max |logit|)"""
    lg = np.asarray(logits, dtype=np.float64)
    return 1e-4 * max(1.0, float(np.abs(lg).max()) if len(lg) else 1.0)

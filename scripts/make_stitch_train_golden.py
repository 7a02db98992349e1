#!/usr/bin/env python3
"""Generates tests/golden/stitch_train_small.pt: three TRAINING steps of the reference's own edge-pair classifier —
nets.StitchOnEdge3DPairs with its ComposedLoss (nn/nets.py:303-353, nn/metrics/composed_loss.py:11-126), CPU fp32, train mode,
metrics on, stepped by torch.optim.Adam(lr=2e-3) — on a shape off the fused 200-wide menu and off every tile size:
element_size 12, stitch_hidden_size 72, stitch_mlp_n_layers 2, pair rows [3, 271, 12] = 813 rows.

The rows are standard-normal draws from a seed; the labels are a fixed function of the rows (r0 + r1 r2 / 2 > 0.75: about a quarter
positives), so the model has something to learn.  Per step the file holds the state dict before the step, the train-mode logits,
the full loss, the loss-dict values and their Python types, the five counts and every parameter gradient; then the state dict after
the last step and the configurations.  Data only.

Decision margins are a CONDITION of the stored seed: seeds are tried in order and the first one is kept for which, at every step,
  * the fp32 numbers lie within a quarter of the device tests' bars (tests/test_gpu_stitch_train.py: logits 1e-4 max(1, max|ref|),
    loss 1e-5, gradients 5e-3 max|grad|, BatchNorm statistics rtol 1e-4 / atol 1e-6) of the same step re-run in float64,
  * no logit lies within 1e-3 of 0 (the class decisions are safe), and
  * no pre-activation of the last Linear (one unit) lies within 1e-3 max|pre| of 0: its ReLU is the only place where one row
    changing sides moves a gradient by about 1 / rows of its scale.

Only runnable where the reference checkout exists (like scripts/make_stitch_eval_golden.py).

    python scripts/make_stitch_train_golden.py [REFERENCE_DIR]
"""
import copy
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('GPE_REFERENCE', '/root/reference')
sys.path[:0] = [os.path.join(REPO, 'oracle', 'refgen', 'stubs'), os.path.join(REF, 'nn'), REPO]

import nets as ref_nets  # noqa: E402  (the reference's module)

torch.set_num_threads(1)
GOLDEN = os.path.join(REPO, 'tests', 'golden')
DATA_CONFIG = {'element_size': 12}
NN_CONFIG = {'stitch_hidden_size': 72, 'stitch_mlp_n_layers': 2}
SHAPE = (3, 271, 12)
STEPS, LR = 3, 2e-3
BARS = {'logits': 1e-4, 'loss': 1e-5, 'grad': 5e-3, 'bn_rtol': 1e-4, 'bn_atol': 1e-6}
MARGIN = 1e-3


def labels_of(rows):
    return rows[..., 0] + 0.5 * rows[..., 1] * rows[..., 2] > 0.75


def _num(v):
    """the reference returns tensors, or the Python int 0 on an empty denominator"""
    return float(v.detach()) if isinstance(v, torch.Tensor) else float(v)


def one_step(model, rows, labels):
    """forward + loss + backward of the reference's classes -> what the fixture keeps of it, and the last Linear's pre-activations"""
    pre = []
    hook = model.mlp[-1][0].register_forward_hook(lambda mod, inp, out: pre.append(out.detach().clone()))
    model.zero_grad()
    logits = model(rows)
    full, loss_dict, _ = model.loss(logits, labels)
    full.backward()
    hook.remove()
    cls = torch.round(torch.sigmoid(logits.detach())).bool()
    counts = {'pairs': int(labels.numel()), 'correct': int((cls == labels).sum()), 'true_positives': int((cls & labels).sum()),
              'predicted_positives': int(cls.sum()), 'gt_positives': int(labels.sum())}
    return {'logits': logits.detach().clone(), 'full_loss': float(full.detach()), 'loss_dict': {k: _num(v) for k, v in loss_dict.items()},
            'loss_types': {k: type(v).__name__ for k, v in loss_dict.items()}, 'counts': counts,
            'grads': {n: p.grad.detach().clone() for n, p in model.named_parameters()}}, pre[0]


def distances(rec, rec64, after, after64):
    """fp32 step against its float64 re-run, each as a fraction of its bar"""
    d = {'logits': float((rec['logits'].double() - rec64['logits']).abs().max()) / (BARS['logits'] * max(1.0, float(rec['logits'].abs().max()))),
         'loss': abs(rec['full_loss'] - rec64['full_loss']) / BARS['loss'],
         'grad': max(float((g.double() - rec64['grads'][n]).abs().max()) / (BARS['grad'] * float(g.abs().max()))
                     for n, g in rec['grads'].items())}
    bn = 0.0
    for k, v in after.items():
        if v.is_floating_point() and ('running_' in k):
            bn = max(bn, float(((v.double() - after64[k]).abs() / (BARS['bn_atol'] + BARS['bn_rtol'] * after64[k].abs())).max()))
    d['bn'] = bn
    return d


def attempt(seed):
    torch.manual_seed(seed)
    model = ref_nets.StitchOnEdge3DPairs(dict(DATA_CONFIG), dict(NN_CONFIG), {})
    model.train()
    model.loss.train()
    gen = torch.Generator().manual_seed(seed)
    rows = torch.randn(*SHAPE, generator=gen)
    labels = labels_of(rows)
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    steps, worst = [], {}
    for s in range(STEPS):
        before = copy.deepcopy(model.state_dict())
        twin = copy.deepcopy(model).double()
        rec64, _ = one_step(twin, rows.double(), labels)
        rec, pre = one_step(model, rows, labels)
        for k, v in distances(rec, rec64, model.state_dict(), twin.state_dict()).items():
            worst[k] = max(worst.get(k, 0.0), v)
        worst['logit_margin'] = min(worst.get('logit_margin', 1e9), float(rec['logits'].abs().min()))
        worst['pre_margin'] = min(worst.get('pre_margin', 1e9), float(pre.abs().min() / pre.abs().max()))
        if min(worst['logit_margin'], worst['pre_margin']) <= MARGIN:
            return False, worst, None                      # (most seeds end here: about six rows in 2439 are expected inside the margin)
        opt.step()
        rec['state_before'] = before
        steps.append(rec)
    ok = all(worst[k] < 0.25 for k in ('logits', 'loss', 'grad', 'bn')) and worst['logit_margin'] > MARGIN and worst['pre_margin'] > MARGIN
    fx = {'seed': seed, 'data_config': dict(DATA_CONFIG), 'nn_config': dict(NN_CONFIG),
          'loss_config': {k: list(v) if isinstance(v, (list, tuple)) else v for k, v in model.loss.config.items()},
          'optimizer': {'name': 'Adam', 'lr': LR}, 'pairs': rows, 'labels': labels, 'steps': steps,
          'state_after': copy.deepcopy(model.state_dict()), 'fp32_vs_fp64_in_bars': {k: worst[k] for k in ('logits', 'loss', 'grad', 'bn')},
          'logit_margin': worst['logit_margin'], 'pre_margin': worst['pre_margin']}
    return ok, worst, fx


if __name__ == '__main__':
    for seed in range(9200, 9200 + 20000):
        ok, worst, fx = attempt(seed)
        if ok:
            print('seed %d kept after %d skipped:  %s' % (seed, seed - 9200, '  '.join('%s=%.3g' % kv for kv in sorted(worst.items()))))
            break
    else:
        raise RuntimeError('no seed keeps the reference inside the conditions')
    dst = os.path.join(GOLDEN, 'stitch_train_small.pt')
    torch.save(fx, dst)
    c = fx['steps'][0]['counts']
    print('stitch_train_small: seed %d, %d rows, %d positives, losses %s, %.1f KB'
          % (fx['seed'], c['pairs'], c['gt_positives'], ['%.6f' % s['full_loss'] for s in fx['steps']], os.path.getsize(dst) / 1024))

"""fp64 restatement of the guarded Adam step (include/gpe_hip_ext.h; gpe_amd.optim.FusedAdam with max_grad_norm / skip_nonfinite /
guard_overflow): the global gradient norm as the norm of the per-segment norms, the clip factor, the skip rule and the update.
Plain torch on CPU, no rounding to fp32 anywhere: tests/test_adam_guard_host.py pins it to torch's clip_grad_norm_ + Adam in
float64, the GPU tests compare the device against it.

Step numbers: a skipped step keeps its number — `t` advances on every call of step(), applied or not."""
import math

import torch

LIMIT = 65504.0


def norms(grads, gscale=1.0):
    """-> (total, [per-segment]) L2 norms of gscale * g in float64; the total is the norm of the vector of segment norms."""
    seg = [(float(gscale) * g.detach().double().reshape(-1)).norm() for g in grads]
    return torch.stack(seg).norm(), seg


def factor(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)); exactly 1 when clipping is off (max_norm None or <= 0)"""
    if max_norm is None or max_norm <= 0:
        return 1.0
    c = float(max_norm) / (float(norm) + 1e-6)
    return c if c < 1.0 else 1.0


def skip_rule(norm, nonfinite_skip, words=(), limit=LIMIT):
    """set iff (nonfinite_skip and the norm is not finite) or a watched word is >= limit or NaN"""
    if nonfinite_skip and not math.isfinite(float(norm)):
        return True
    return any(not (float(w) < limit) for w in words)


class GuardedAdam64:
    """torch.optim.Adam (amsgrad off) over float64 copies of `params`, each step under the guard."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 skip_nonfinite=False, lr_of_step=None):
        self.p = [q.detach().double().clone() for q in params]
        self.m = [torch.zeros_like(q) for q in self.p]
        self.v = [torch.zeros_like(q) for q in self.p]
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, skip_nonfinite
        self.lr_of_step = lr_of_step           # 0-based step -> learning rate (a OneCycle schedule), None = constant
        self.t = 0
        self.skipped = 0
        self.norm = self.coef = None
        self.last_skipped = False

    def step(self, grads, gscale=1.0, words=()):
        lr = self.lr if self.lr_of_step is None else self.lr_of_step(self.t)
        self.t += 1                            # the number of THIS step, skipped or not
        self.norm, self.seg_norms = norms(grads, gscale)
        self.coef = factor(self.norm, self.max_grad_norm)
        self.last_skipped = skip_rule(self.norm, self.skip_nonfinite, words)
        if self.last_skipped:
            self.skipped += 1
            return
        b1, b2 = self.betas
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        for p, m, v, g in zip(self.p, self.m, self.v, grads):
            gr = g.detach().double().reshape(p.shape) * (float(gscale) * self.coef) + self.wd * p
            m.mul_(b1).add_(gr, alpha=1.0 - b1)
            v.mul_(b2).addcmul_(gr, gr, value=1.0 - b2)
            p.sub_((lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + self.eps))

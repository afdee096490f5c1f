"""LAMB in float64, per tensor, straight from the definition (timm's ``Lamb``
with ``always_adapt=False``, ``trust_clip=False``, after ``clip_grad_norm_``):
the oracle of tests/test_gpu_lamb.py and tests/test_lamb_cpu.py."""
import math

import torch

LR, BETAS, EPS, WD = 1e-2, (0.9, 0.99), 1e-6, 0.1
HP = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
SCALES = (0.1, 1.0, 10.0)  # of the weights, tensor by tensor: neighbouring trust ratios differ about tenfold


class Oracle:
    def __init__(self, ws, adapted, max_norm=0.0):
        self.w = [w.detach().double().clone() for w in ws]
        self.m = [torch.zeros_like(w) for w in self.w]
        self.v = [torch.zeros_like(w) for w in self.w]
        self.adapted, self.max_norm, self.t = list(adapted), max_norm, 0

    def step(self, grads):
        """One step; returns float64 [T, 3]: trust, |w| before the step, |u|."""
        gs = [g.detach().double().reshape(w.shape) for g, w in zip(grads, self.w)]
        c = 1.0
        if self.max_norm > 0:
            c = min(1.0, self.max_norm / (math.sqrt(sum(float(g.pow(2).sum()) for g in gs)) + 1e-6))
        self.t += 1
        (b1, b2), out = BETAS, []
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        for w, m, v, g, a in zip(self.w, self.m, self.v, gs, self.adapted):
            g = c * g
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).add_(g * g, alpha=1 - b2)
            u = (m / bc1) / (v.sqrt() / math.sqrt(bc2) + EPS) + (WD * w if a else 0)
            wn, un = float(w.norm()), float(u.norm())
            trust = wn / un if a and wn != 0 and un != 0 else 1.0
            w.sub_(u, alpha=LR * trust)
            out.append((trust, wn, un))
        return torch.tensor(out, dtype=torch.float64)

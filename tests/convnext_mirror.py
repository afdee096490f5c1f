"""A plain-torch mirror of models/convnext.py for the tests: ``nn.Conv2d`` /
``nn.LayerNorm`` / ``nn.Linear`` on NCHW tensors with the explicit
``gamma *`` (no folding, no fused op, no token layout), with the same
parameter names, so it loads the model's state dict as it is."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class MirrorBlock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.fc2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(torch.ones(dim))

    def forward(self, x, scale=None):
        h = self.norm(self.dwconv(x).permute(0, 2, 3, 1))
        h = (self.gamma * self.fc2(F.gelu(self.fc1(h)))).permute(0, 3, 1, 2)
        if scale is not None:
            h = scale.to(h.dtype).view(-1, 1, 1, 1) * h
        return x + h


def _ln2d(ln, x):
    return ln(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


class Mirror(nn.Module):
    def __init__(self, depths, dims, num_classes=1000, in_chans=3):
        super().__init__()
        self.stem = nn.Conv2d(in_chans, dims[0], 4, stride=4)
        self.stem_norm = nn.LayerNorm(dims[0], eps=1e-6)
        self.down_norms = nn.ModuleList(nn.LayerNorm(dims[i - 1], eps=1e-6) for i in range(1, len(dims)))
        self.downs = nn.ModuleList(nn.Conv2d(dims[i - 1], dims[i], 2, stride=2) for i in range(1, len(dims)))
        self.stages = nn.ModuleList(nn.ModuleList(MirrorBlock(d) for _ in range(n)) for n, d in zip(depths, dims))
        self.norm = nn.LayerNorm(dims[-1], eps=1e-6)
        self.head = nn.Linear(dims[-1], num_classes)

    def forward(self, x, scales=None):
        """scales: one per-sample drop-path scale vector (or None) per block, in order."""
        x = _ln2d(self.stem_norm, self.stem(x))
        k = 0
        for i, stage in enumerate(self.stages):
            if i > 0:
                x = self.downs[i - 1](_ln2d(self.down_norms[i - 1], x))
            for blk in stage:
                x = blk(x, None if scales is None else scales[k])
                k += 1
        return self.head(self.norm(x.mean((2, 3))))


def mirror_of(model):
    """fp32 Mirror with `model`'s weights, on its device."""
    m = Mirror(model.depths, model.dims, model.head.out_features, model.stem.in_channels)
    m.load_state_dict({k: v.detach().float() for k, v in model.state_dict().items()})
    return m.to(next(model.parameters()).device)


def grads(model, x, y, **kw):
    model.zero_grad(set_to_none=True)
    loss = F.cross_entropy(model(x, **kw).float(), y)
    loss.backward()
    return loss.item(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()}

"""The training step's model (include/qttt_train.h): examples/selfplay_train.py's Net and loss_terms
restated on plain tensors with loss = L.mean() + J.mean(), differentiated by torch autograd on the CPU, once in float64
and once in float32, and torch.optim.Adam(amsgrad=True)'s update restated in the five lines of the header.

The float32 run is not the expected value: max |g32 - g64| per parameter tensor is what a change of summation order does
to these inputs (the method of DESIGN.md §10's numerics contract), and the device is held to MARGIN times that, with a
floor of one f32 ulp of the tensor's largest element.  No device, no library."""
import math

import torch

KEYS = ("fc.0.weight", "fc.0.bias", "fc.2.weight", "fc.2.bias", "fc.4.weight", "fc.4.bias",
        "V_head.1.weight", "V_head.1.bias", "pi_head.1.weight", "pi_head.1.bias")
MARGIN = 8.0
ULP = 2.0 ** -23
CHUNK = 256                                  # QTTT_TRAIN_CHUNK
BLOB_FLOATS = 180 * 256 + 2 * 256 * 256 + 256 * 48 + 3 * 256 + 48


def workspace_bytes(n):
    """The plan of qtttgym_amd/csrc/qttt_train_host.h: six f32[n, 256] arrays, dOut f32[n, 48], a blob per chunk, the count;
    every array at a 256-byte-aligned offset."""
    al = lambda b: (b + 255) // 256 * 256  # noqa: E731
    chunks = (n + CHUNK - 1) // CHUNK
    return 6 * al(n * 256 * 4) + al(n * 48 * 4) + al(chunks * BLOB_FLOATS * 4) + 256


def forward(w, s):
    z = s.flatten(-2, -1)
    for i in (0, 2, 4):
        z = torch.relu(z @ w["fc.%d.weight" % i].t() + w["fc.%d.bias" % i])
    return (z @ w["V_head.1.weight"].t() + w["V_head.1.bias"]).squeeze(-1), z @ w["pi_head.1.weight"].t() + w["pi_head.1.bias"]


def loss_terms(w, s, pi, mask, v_target, done):
    """examples/selfplay_train.py loss_terms (self_play.py:226-236): L per sample, J per sample that is not terminal."""
    v, logits = forward(w, s)
    keep = ~done
    logp = torch.log_softmax(logits[keep].masked_fill(~mask[keep], -float("inf")), dim=-1)
    p, legal = pi[keep], mask[keep]
    J = torch.zeros_like(p)
    J[legal] = p[legal] * (torch.log(p[legal] + 1e-7) - logp[legal])
    return 0.5 * (v - v_target).pow(2), J.sum(-1)


def gradients(sd, batch, dtype):
    """(grads under KEYS, L [n], J [n] with 0 at the terminal samples, loss) of the model in `dtype` on the CPU."""
    s, pi, mask, v, done = (t.cpu() for t in batch)
    w = {k: sd[k].detach().cpu().to(dtype).clone().requires_grad_(True) for k in KEYS}
    L, Jk = loss_terms(w, s.to(dtype), pi.to(dtype), mask, v.to(dtype), done)
    loss = L.mean() + Jk.mean()
    loss.backward()
    J = torch.zeros_like(L)
    J[~done] = Jk.detach()
    return {k: w[k].grad for k in KEYS}, L.detach(), J, loss.detach()


def bound(ref32, ref64):
    """MARGIN * max(what float32 does to these inputs, one f32 ulp of the largest element)."""
    d_ref = (ref32.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    top = ref64.abs().max().item() if ref64.numel() else 0.0
    return MARGIN * max(d_ref, ULP * top)


class Adam:
    """torch.optim.Adam(lr, betas, eps, weight_decay, amsgrad=True) on a dict of tensors, in the tensors' dtype."""

    def __init__(self, sd, dtype, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3):
        self.w = {k: sd[k].detach().cpu().to(dtype).clone() for k in KEYS}
        self.m, self.v2, self.vmax = ({k: torch.zeros_like(t) for k, t in self.w.items()} for _ in range(3))
        self.lr, self.betas, self.eps, self.wd, self.t = lr, betas, eps, weight_decay, 0

    def step(self, grads):
        self.t += 1
        b1, b2 = self.betas
        step_size, bc2_sqrt = self.lr / (1 - b1 ** self.t), math.sqrt(1 - b2 ** self.t)
        for k in KEYS:
            g = grads[k] + self.wd * self.w[k]
            self.m[k] = b1 * self.m[k] + (1 - b1) * g
            self.v2[k] = b2 * self.v2[k] + (1 - b2) * g * g
            self.vmax[k] = torch.maximum(self.vmax[k], self.v2[k])
            self.w[k] = self.w[k] - step_size * (self.m[k] / (self.vmax[k].sqrt() / bc2_sqrt + self.eps))

"""Importance weights in the training step (include/qttt_train_weighted.h, Trainer.gradients(..., weight=)) on the MI355X:
weight 1.0f is qttt_train_gradients bit for bit; general weights against the float64 autograd model of
tests/train_model.py under the weighted loss, by the project's rule (every tensor within 8 * max(what float32 does to the
same inputs, one f32 ulp of its largest element)); and a sample of weight 0 contributes nothing.

Measured on an MI355X (largest error in allowance units, the margin being 8): see DESIGN.md §28."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_model as M  # noqa: E402
from nn_reference64 import KEYS  # noqa: E402
from test_train_gpu import _batch, _bits, _state_dict, _trainer  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 65, M.CHUNK + 1]


@functools.lru_cache(maxsize=None)
def _weight(n):
    """Weights in [0.1, 1] with an exact 0 on the last sample that is not sample 0 (n > 1)."""
    w = torch.rand(n, generator=torch.Generator().manual_seed(31 * n)) * 0.9 + 0.1
    if n > 1:
        w[n - 1] = 0.0
    return w.to(torch.float32)


def weighted_gradients(sd, batch, weight, dtype, n=None, n_keep=None):
    """(grads under KEYS, L, J) of tests/train_model.py's model under loss = sum_i w_i L_i / n + sum over the non-terminal
    i of w_i J_i / n_keep, in `dtype` on the CPU.  n and n_keep default to the batch's own counts."""
    s, pi, mask, v, done = (t.cpu() for t in batch)
    w = {k: sd[k].detach().cpu().to(dtype).clone().requires_grad_(True) for k in KEYS}
    wt = weight.cpu().to(dtype)
    L, Jk = M.loss_terms(w, s.to(dtype), pi.to(dtype), mask, v.to(dtype), done)
    n = len(L) if n is None else n
    n_keep = int((~done).sum()) if n_keep is None else n_keep
    loss = (wt * L).sum() / n + (wt[~done] * Jk).sum() / n_keep
    loss.backward()
    J = torch.zeros_like(L)
    J[~done] = Jk.detach()
    return {k: w[k].grad for k in KEYS}, L.detach(), J


def worst_ratio(got, ref32, ref64, keys):
    ratios = {}
    for k in keys:
        err, allowed = (got[k] - ref64[k]).abs().max().item(), M.bound(ref32[k], ref64[k])
        ratios[k] = M.MARGIN * err / allowed if allowed else (0.0 if err == 0 else float("inf"))
    worst = max(ratios, key=ratios.get)
    return ratios[worst], worst


@pytest.mark.parametrize("n", SIZES)
def test_weight_one_is_the_unweighted_entry_bit_for_bit(n):
    batch = _batch(n)
    a, b = _trainer(), _trainer()
    La, Ja = a.gradients(*batch)
    Lb, Jb = b.gradients(*batch, weight=torch.ones(n, device=DEV))
    assert torch.equal(_bits(a.grads), _bits(b.grads))
    assert torch.equal(_bits(La), _bits(Lb)) and torch.equal(_bits(Ja), _bits(Jb))


@pytest.mark.parametrize("n", SIZES)
def test_weighted_gradients_against_float64(n):
    batch, weight = _batch(n), _weight(n)
    sd = _state_dict("random")
    g64, L64, J64 = weighted_gradients(sd, batch, weight, torch.float64)
    g32, L32, J32 = weighted_gradients(sd, batch, weight, torch.float32)
    tr = _trainer()
    L, J = tr.gradients(*batch, weight=weight.to(DEV))
    got = {k: t.double().cpu() for k, t in tr.grad_dict().items()}
    got["L"], got["J"] = L.double().cpu(), J.double().cpu()
    ratio, worst = worst_ratio(got, dict(g32, L=L32, J=J32), dict(g64, L=L64, J=J64), KEYS + ("L", "J"))
    print("weighted n=%d: largest error / allowance unit = %.3f at %s (the margin is %g)" % (n, ratio, worst, M.MARGIN))
    assert ratio <= M.MARGIN
    # L and J are the unweighted terms: the bits of the unweighted entry
    plain = _trainer()
    L0, J0 = plain.gradients(*batch)
    assert torch.equal(_bits(L), _bits(L0)) and torch.equal(_bits(J), _bits(J0))
    if n > 1:
        assert not torch.equal(_bits(tr.grads), _bits(plain.grads))


@pytest.mark.parametrize("n", [65, M.CHUNK + 1])
def test_a_sample_of_weight_zero_contributes_nothing(n):
    """Sample j = n - 1 has weight 0.  (a) Against float64: the gradients are those of the batch WITHOUT j, under the n and
    n_keep of the batch with it (the contract divides by the counts of the samples, not by the sum of the weights).  (b)
    Exactly: whatever stands in j's rows, the gradients keep their bits, because every term of j is a product with 0."""
    batch, weight = _batch(n), _weight(n)
    j = n - 1
    assert float(weight[j]) == 0.0
    done = batch[4]
    tr = _trainer()
    tr.gradients(*batch, weight=weight.to(DEV))
    got = {k: t.double().cpu() for k, t in tr.grad_dict().items()}
    rest = tuple(t[:j] for t in batch)
    sd = _state_dict("random")
    n_keep = int((~done).sum())
    g64, _, _ = weighted_gradients(sd, rest, weight[:j], torch.float64, n=n, n_keep=n_keep)
    g32, _, _ = weighted_gradients(sd, rest, weight[:j], torch.float32, n=n, n_keep=n_keep)
    ratio, worst = worst_ratio(got, g32, g64, KEYS)
    print("weight 0, n=%d: largest error / allowance unit = %.3f at %s" % (n, ratio, worst))
    assert ratio <= M.MARGIN
    # (b) another position, policy and value in row j (its done byte stays: n_keep is a count of the samples)
    s, pi, mask, v, _ = (t.clone() for t in batch)
    src = 0 if bool(done[0]) == bool(done[j]) else int((done == done[j]).nonzero()[0])
    assert src != j
    s[j], pi[j], mask[j], v[j] = s[src], pi[src], mask[src], -v[src] + 0.5
    other = _trainer()
    other.gradients(s, pi, mask, v, done, weight=weight.to(DEV))
    assert torch.equal(_bits(other.grads), _bits(tr.grads))

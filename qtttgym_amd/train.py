"""Trainer — the training step of the policy/value network on the device (include/qttt_train.h): the
reference's loss (self_play.py:226-236), its gradients and its Adam(amsgrad=True) step, with the parameters, the
gradients and the optimiser state all in the layout of the packed f32 weight blob that the search evaluates.

    net = PolicyValueNet(model)                          # what SelfPlay / TreeSearch / VecEnv.evaluate read
    trainer = Trainer(model, net=net)                    # an f32 net: trainer.weights IS net.blob
    L, J = trainer.step(*ring.sample(4096, "random"))    # six launches, no host synchronisation, no repack
    L, J = trainer.step(*batch, weight=ring.weights(1.0))   # a prioritised ring's importance weights in the loss (§28)
    torch.save(trainer.state_dict(), "model.pt")

Training is f32.  A bf16 `net` gets its blob rewritten from the new weights by the optimiser's own launch.
"""
import torch

from . import _native
from ._host import LibCaller, check_net, check_tensor, resolve_device
from .policy_value import pack_weights, unpack_weights

_IN = (("s", torch.float32, (18, 10)), ("pi", torch.float64, (36,)), ("mask", torch.bool, (36,)), ("v", torch.float32, ()),
       ("done", torch.bool, ()))


class Trainer(LibCaller):
    """The network's f32 parameters as a packed blob (`weights`), with `grads`, `m`, `v2` and `vmax` beside it in the same
    layout.  gradients(s, pi, mask, v, done) fills `grads` from a minibatch as SelfPlayBatch.flat() and ReplayBuffer.sample
    return it; step(...) is gradients and then torch.optim.Adam(lr, betas, eps, weight_decay, amsgrad=True)'s update, in
    place.  Both return the per-sample loss terms (L, J), f32[n] each: loss = L.mean() + J[~done].mean().  The defaults are
    the reference's optimiser (nn.py:27).  net: a PolicyValueNet on the same device that is to follow the training — an f32
    net's blob becomes `weights` itself (same storage, same address: captured graphs stay valid), a bf16 net's blob is
    rewritten by every step; either way the next search sees the new weights without a load_state_dict."""

    def __init__(self, source, device="cuda", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3, net=None):
        self._open(resolve_device(device, "Trainer"))
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        packed = pack_weights(source, torch.float32).to(self.device)
        self.net = net
        if net is not None:
            check_net(net, self.device)
        if net is not None and net.dtype == torch.float32:
            self.weights = net.blob
            self.weights.copy_(packed)
        else:
            self.weights = packed
            if net is not None:
                net.load_state_dict(unpack_weights(packed, torch.float32))
        self.grads, self.m, self.v2, self.vmax = (torch.zeros_like(self.weights) for _ in range(4))
        self.step_count = 0
        self._workspace = None

    def gradients(self, s, pi, mask, v, done, weight=None):
        """Fills `grads` with d loss / d weights for the minibatch and returns (L, J) (qttt_train_gradients).  weight
        (f32[n], optional): importance weights, loss = mean(w L) + sum(w J over the non-terminal) / n_keep
        (qttt_train_gradients_weighted, include/qttt_train_weighted.h); L and J come back unweighted either way."""
        n, dev = int(s.shape[0]) if s.dim() else 0, self.device
        if not 1 <= n <= _native.TRAIN_MAX_SAMPLES:
            raise ValueError("a minibatch has 1..%d samples" % _native.TRAIN_MAX_SAMPLES)
        for t, (name, dt, shp) in zip((s, pi, mask, v, done), _IN):
            check_tensor(t, dt, (n,) + shp, dev, name)
        need = int(self._lib.qttt_train_workspace_bytes(n))
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        L, J = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        if weight is not None:
            check_tensor(weight, torch.float32, (n,), dev, "weight")
            self._call("qttt_train_gradients_weighted", s.data_ptr(), pi.data_ptr(), mask.data_ptr(), v.data_ptr(),
                       done.data_ptr(), weight.data_ptr(), n, self.weights.data_ptr(), self.grads.data_ptr(), L.data_ptr(),
                       J.data_ptr(), self._workspace.data_ptr())
            return L, J
        self._call("qttt_train_gradients", s.data_ptr(), pi.data_ptr(), mask.data_ptr(), v.data_ptr(), done.data_ptr(), n,
                   self.weights.data_ptr(), self.grads.data_ptr(), L.data_ptr(), J.data_ptr(), self._workspace.data_ptr())
        return L, J

    def step(self, s, pi, mask, v, done, weight=None):
        """gradients(...), then one AMSGrad step on `weights` (qttt_train_adam); returns (L, J) of the weights before it."""
        out = self.gradients(s, pi, mask, v, done, weight)
        self.step_count += 1
        bf16 = self.net.blob.data_ptr() if self.net is not None and self.net.dtype == torch.bfloat16 else 0
        self._call("qttt_train_adam", self.weights.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(), self.v2.data_ptr(),
                   self.vmax.data_ptr(), self.step_count, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                   bf16)
        return out

    def state_dict(self):
        """The weights as the reference's state dict (nn.Model's ten keys), new f32 tensors on the device."""
        return unpack_weights(self.weights, torch.float32)

    def grad_dict(self):
        """The gradients of the last gradients() / step() under the same ten keys."""
        return unpack_weights(self.grads, torch.float32)

    def __repr__(self):
        return "Trainer(step_count=%d, device=%s)" % (self.step_count, self.device)

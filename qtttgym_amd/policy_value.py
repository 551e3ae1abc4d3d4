"""PolicyValueNet — the reference's policy/value network (nn.py:7-72) as a packed weight blob that
libqttt_hip.so evaluates for a batch of boards in one kernel (include/qttt_nn.h qttt_evaluate, VecEnv.evaluate).

The network itself is the reference's: 180 -> 256 -> 256 -> 256 ReLU trunk, a value head (-> 1) and a policy head
(-> 36), taken from a state dict with nn.Model's ten keys (e.g. torch.load("model.pt")).  Packing lays the weights out
as the kernel's MFMA B fragments; the layout is documented in include/qttt_nn.h."""
import torch

from . import _native
from ._host import resolve_device

HIDDEN = 256
HEAD_COLS = 48                       # 36 logits, the value, 11 zero columns
SHAPES = {
    "fc.0.weight": (HIDDEN, 180), "fc.0.bias": (HIDDEN,),
    "fc.2.weight": (HIDDEN, HIDDEN), "fc.2.bias": (HIDDEN,),
    "fc.4.weight": (HIDDEN, HIDDEN), "fc.4.bias": (HIDDEN,),
    "V_head.1.weight": (1, HIDDEN), "V_head.1.bias": (1,),
    "pi_head.1.weight": (36, HIDDEN), "pi_head.1.bias": (36,),
}
_PRECISION = {torch.float32: _native.NN_F32, torch.bfloat16: _native.NN_BF16}
_K1 = {torch.float32: 180, torch.bfloat16: 192}            # layer-1 K, padded to the MFMA's K


def _state_dict(source):
    sd = source.state_dict() if hasattr(source, "state_dict") else source
    if not hasattr(sd, "keys"):
        raise ValueError("source must be a state dict or a module that has one")
    missing = [k for k in SHAPES if k not in sd]
    if missing:
        raise ValueError("state dict lacks %s (nn.Model's keys)" % ", ".join(missing))
    for k, shape in SHAPES.items():
        t = sd[k]
        if not torch.is_tensor(t) or not t.is_floating_point():
            raise ValueError("%s must be a floating-point tensor" % k)
        if tuple(t.shape) != shape:
            raise ValueError("%s has shape %s, expected %s (only width %d exists)" % (k, tuple(t.shape), shape, HIDDEN))
    return sd


def _check_dtype(dtype):
    if dtype not in _PRECISION:
        raise ValueError("dtype must be torch.float32 or torch.bfloat16")


def weights_bytes(dtype):
    """Size of the packed blob in bytes (= include/qttt_nn.h qttt_nn_weights_bytes, computed here without the library)."""
    _check_dtype(dtype)
    elems = _K1[dtype] * HIDDEN + 2 * HIDDEN * HIDDEN + HIDDEN * HEAD_COLS
    return elems * (4 if dtype == torch.float32 else 2) + (3 * HIDDEN + HEAD_COLS) * 4


def _fragments(B, dtype):
    """B[K][C] -> the kernel's fragment order (include/qttt_nn.h): f32 [k/4][c/16][k%4][c%16],
    bf16 [k/32][c/16][k%32/8][c%16][k%8]."""
    K, C = B.shape
    if dtype == torch.float32:
        return B.reshape(K // 4, 4, C // 16, 16).permute(0, 2, 1, 3).reshape(-1)
    return B.reshape(K // 32, 4, 8, C // 16, 16).permute(0, 3, 1, 4, 2).reshape(-1)


def pack_weights(sd, dtype=torch.float32):
    """The packed blob of include/qttt_nn.h for a state dict with nn.Model's ten keys, as a uint8 tensor of
    weights_bytes(dtype) bytes on the state dict's device (CPU tensors work: torch ops only).  bf16 weights are
    torch's round-to-nearest-even conversion of the f32 values; biases stay f32."""
    _check_dtype(dtype)
    sd = _state_dict(sd)
    dev = sd["fc.0.weight"].device
    f = {k: sd[k].detach().to(device=dev, dtype=torch.float32) for k in SHAPES}
    w1 = torch.zeros((_K1[dtype], HIDDEN), dtype=torch.float32, device=dev)
    w1[:180] = f["fc.0.weight"].t()
    wh = torch.zeros((HIDDEN, HEAD_COLS), dtype=torch.float32, device=dev)
    wh[:, :36] = f["pi_head.1.weight"].t()
    wh[:, 36] = f["V_head.1.weight"][0]
    mats = [w1, f["fc.2.weight"].t(), f["fc.4.weight"].t(), wh]
    weights = torch.cat([_fragments(m.contiguous(), dtype) for m in mats]).to(dtype)
    hb = torch.zeros(HEAD_COLS, dtype=torch.float32, device=dev)
    hb[:36] = f["pi_head.1.bias"]
    hb[36] = f["V_head.1.bias"][0]
    biases = torch.cat([f["fc.0.bias"], f["fc.2.bias"], f["fc.4.bias"], hb])
    return torch.cat([weights.view(torch.uint8), biases.contiguous().view(torch.uint8)])


def _matrix(frag, K, C, dtype):
    """The inverse of _fragments: the fragment-ordered elements of one matrix -> B[K][C]."""
    if dtype == torch.float32:
        return frag.reshape(K // 4, C // 16, 4, 16).permute(0, 2, 1, 3).reshape(K, C)
    return frag.reshape(K // 32, C // 16, 4, 16, 8).permute(0, 2, 4, 1, 3).reshape(K, C)


def unpack_weights(blob, dtype=torch.float32):
    """The inverse of pack_weights: the state dict (nn.Model's ten keys, f32 tensors on the blob's device) of a packed
    blob of weights_bytes(dtype) bytes, given as a uint8 tensor or any contiguous tensor of that many bytes.  Torch ops
    only; CPU tensors work.  A bf16 blob gives its weights widened to f32 (exactly), so
    pack_weights(unpack_weights(blob, dtype), dtype) is the blob again as long as its pad elements are zero."""
    _check_dtype(dtype)
    raw = blob.detach().contiguous().view(torch.uint8).reshape(-1)
    if raw.numel() != weights_bytes(dtype):
        raise ValueError("a %s blob has %d bytes, not %d" % (dtype, weights_bytes(dtype), raw.numel()))
    size = 4 if dtype == torch.float32 else 2
    k1, mats, at = _K1[dtype], [], 0
    for K, C in ((k1, HIDDEN), (HIDDEN, HIDDEN), (HIDDEN, HIDDEN), (HIDDEN, HEAD_COLS)):
        mats.append(_matrix(raw[at:at + K * C * size].view(dtype), K, C, dtype).float())
        at += K * C * size
    biases = raw[at:].view(torch.float32)
    w1, w2, w3, wh = mats
    hb = biases[3 * HIDDEN:]
    return {
        "fc.0.weight": w1[:180].t().contiguous(), "fc.0.bias": biases[:HIDDEN].clone(),
        "fc.2.weight": w2.t().contiguous(), "fc.2.bias": biases[HIDDEN:2 * HIDDEN].clone(),
        "fc.4.weight": w3.t().contiguous(), "fc.4.bias": biases[2 * HIDDEN:3 * HIDDEN].clone(),
        "V_head.1.weight": wh[:, 36:37].t().contiguous(), "V_head.1.bias": hb[36:37].clone(),
        "pi_head.1.weight": wh[:, :36].t().contiguous(), "pi_head.1.bias": hb[:36].clone(),
    }


class PolicyValueNet:
    """The network of nn.py, packed once for the device: VecEnv.evaluate(net) runs it on every board of an
    environment in one kernel.  dtype torch.float32 (exact-f32 MFMA, the reference's numerics) or torch.bfloat16
    (bf16 weights and activations, f32 accumulation).  There is no CPU path: device "cpu" raises QtttNativeError."""

    def __init__(self, source, device="cuda", dtype=torch.float32):
        _check_dtype(dtype)
        sd = _state_dict(source)
        self.dtype = dtype
        self.precision = _PRECISION[dtype]
        self.device = resolve_device(device, "PolicyValueNet")
        nbytes = int(_native.lib().qttt_nn_weights_bytes(self.precision))
        if nbytes != weights_bytes(dtype):
            raise _native.QtttNativeError("libqttt_hip.so blob size %d != %d (stale build?)" % (nbytes, weights_bytes(dtype)))
        self.blob = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.load_state_dict(sd)

    def load_state_dict(self, source):
        """Repacks new weights (e.g. after an optimiser step) into the same device blob: its address does not change,
        so graphs that captured an evaluate() stay valid.  The copy is ordered on the current stream."""
        sd = _state_dict(source)
        packed = pack_weights({k: sd[k].detach().to(self.device) for k in SHAPES}, self.dtype)
        self.blob.copy_(packed)
        return self

    def __repr__(self):
        return "PolicyValueNet(dtype=%s, device=%s)" % (self.dtype, self.device)

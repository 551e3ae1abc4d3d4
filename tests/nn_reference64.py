"""A float64 torch restatement of the reference's Model.forward (nn.py:31-61) on to_vector encodings, for the tests of
PolicyValueNet / VecEnv.evaluate.  tests/test_policy_value_cpu.py pins it to the reference's own outputs
(tests/golden/model_eval.npz); the GPU tests compare the kernel with it."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_eval.npz")
KEYS = ("fc.0.weight", "fc.0.bias", "fc.2.weight", "fc.2.bias", "fc.4.weight", "fc.4.bias",
        "V_head.1.weight", "V_head.1.bias", "pi_head.1.weight", "pi_head.1.bias")


def load_golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


def golden_state_dict(g):
    return {k: torch.from_numpy(g[k.replace(".", "_")].copy()) for k in KEYS}


def random_state_dict(seed):
    """nn.Linear's default initialisation (uniform in +-1/sqrt(fan_in)) of nn.Model's shapes, seeded."""
    gen = torch.Generator().manual_seed(seed)
    shapes = {"fc.0": (256, 180), "fc.2": (256, 256), "fc.4": (256, 256), "V_head.1": (1, 256), "pi_head.1": (36, 256)}
    sd = {}
    for k, (o, i) in shapes.items():
        b = 1.0 / i ** 0.5
        sd[k + ".weight"] = (torch.rand((o, i), generator=gen) * 2 - 1) * b
        sd[k + ".bias"] = (torch.rand((o,), generator=gen) * 2 - 1) * b
    return sd


# ind2move (nn.py:70-74): action a <-> squares (i, j), i < j, in row-major order of the upper triangle
PAIRS = torch.tensor([(i, j) for i in range(9) for j in range(i + 1, 9)], dtype=torch.int64)


def forward64(sd, vec):
    """vec [N,18,10] (any float dtype, any device) -> (value f64[N], logits f64[N,36] with -inf at masked actions,
    probs f64[N,36] = softmax, NaN rows where all 36 are masked)."""
    dev = vec.device
    w = {k: sd[k].to(device=dev, dtype=torch.float64) for k in KEYS}
    s = vec.to(torch.float64)
    occupied = s[:, :9, :9].ne(0).any(-1)                                     # nn.py:45
    pairs = PAIRS.to(dev)
    mask = occupied[:, pairs[:, 0]] | occupied[:, pairs[:, 1]]               # nn.py:56-58
    z = s.flatten(1)
    for i in (0, 2, 4):
        z = torch.relu(z @ w["fc.%d.weight" % i].t() + w["fc.%d.bias" % i])
    v = (z @ w["V_head.1.weight"].t() + w["V_head.1.bias"])[:, 0]
    logits = z @ w["pi_head.1.weight"].t() + w["pi_head.1.bias"]
    logits = logits.masked_fill(mask, -float("inf"))
    return v, logits, torch.softmax(logits, -1)


def forward64_chunked(sd, vec, chunk=1 << 18):
    outs = [forward64(sd, vec[i:i + chunk]) for i in range(0, vec.shape[0], chunk)]
    return tuple(torch.cat([o[k] for o in outs]) for k in range(3))

"""A float64 torch restatement of the reference's Model.forward (nn.py:31-61) on to_vector encodings, for the tests of
PolicyValueNet / VecEnv.evaluate.  tests/test_policy_value_cpu.py pins it to the reference's own outputs
(tests/golden/model_eval.npz); the GPU tests compare the kernel with it.

forward_contract restates the precision contract of include/qttt_nn.h (bf16 weights, input and activations, f32 biases,
accumulation in a chosen dtype), and zero / greedy / counting / sharp_counting_state_dict are networks whose outputs are
exact in every precision and summation order; tests/test_policy_value_numerics_cpu.py checks both without a device.
forward_reference32 is the reference's own chain of torch f32 operations (nn.py:30-42, alphazero.py:296-298)."""
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


def _mask(vec):
    occupied = vec[:, :9, :9].ne(0).any(-1)                                  # nn.py:45
    pairs = PAIRS.to(vec.device)
    return occupied[:, pairs[:, 0]] | occupied[:, pairs[:, 1]]               # nn.py:56-58


def _product(x, w, acc):
    """x [N,K] . w[C,K]^T in dtype acc.  float64: the library's product (its order does not matter at 2^-53).  float32: one
    rounded product and one rounded addition per k, in ascending k: every machine's library sums f32 in an order of its
    own, which would make the float32 result, and every figure derived from it, differ from host to host."""
    if acc == torch.float64:
        return x @ w.t()
    out = torch.zeros((x.shape[0], w.shape[0]), dtype=acc)
    for k in range(x.shape[1]):
        out = out + x[:, k, None] * w[None, :, k]
    return out


def contract_hidden(sd, vec, dtype, acc):
    """The three hidden activations [N,256] (dtype acc) of forward_contract, as the next layer reads them."""
    bf = dtype == torch.bfloat16
    if not bf and dtype != torch.float32:
        raise ValueError("dtype must be torch.float32 or torch.bfloat16")
    # what the kernel stores as T: through f32 (the accumulator's type) to bf16, round-to-nearest-even
    q = (lambda t: t.to(torch.float32).to(torch.bfloat16).to(acc)) if bf else (lambda t: t.to(acc))
    z = q(vec.flatten(1))
    hidden = []
    for i in (0, 2, 4):
        w, b = q(sd["fc.%d.weight" % i]), sd["fc.%d.bias" % i].to(torch.float32).to(acc)
        z = torch.relu(_product(z, w, acc) + b)
        z = q(z) if bf else z
        hidden.append(z)
    return hidden


def forward_contract(sd, vec, dtype, acc):
    """include/qttt_nn.h's precision contract on the CPU: for torch.bfloat16 the weights and the to_vector input go
    through .to(torch.bfloat16), every ReLU output is rounded f32 -> bf16, biases stay f32, the head output is not
    rounded; for torch.float32 it is the plain forward.  acc (torch.float64 / torch.float32) is the dtype of the four
    products (_product: the float32 one in a fixed order) and of the outputs.  Returns forward64's triple: value [N], masked logits [N,36], probs [N,36]."""
    bf = dtype == torch.bfloat16
    q = (lambda t: t.to(torch.float32).to(torch.bfloat16).to(acc)) if bf else (lambda t: t.to(acc))
    z = contract_hidden(sd, vec, dtype, acc)[-1]
    v = (_product(z, q(sd["V_head.1.weight"]), acc) + sd["V_head.1.bias"].to(torch.float32).to(acc))[:, 0]
    logits = _product(z, q(sd["pi_head.1.weight"]), acc) + sd["pi_head.1.bias"].to(torch.float32).to(acc)
    logits = logits.masked_fill(_mask(vec), -float("inf"))
    return v, logits, torch.softmax(logits, -1)


WEIGHTS = tuple(k for k in KEYS if k.endswith(".weight"))


def scaled_state_dict(sd, s):
    """The four weight matrices (the two heads are one matrix to the kernel) times s; the biases as they are."""
    return {k: (sd[k] * s if k in WEIGHTS else sd[k].clone()) for k in KEYS}


# ---------------------------------------------------------------- three networks with exact outputs
_SHAPES = {"fc.0": (256, 180), "fc.2": (256, 256), "fc.4": (256, 256), "V_head.1": (1, 256), "pi_head.1": (36, 256)}


def zero_state_dict():
    """All ten tensors zero: value +0, every legal logit +0, uniform probabilities."""
    sd = {}
    for k, (o, i) in _SHAPES.items():
        sd[k + ".weight"] = torch.zeros((o, i))
        sd[k + ".bias"] = torch.zeros((o,))
    return sd


GREEDY_GAP = 128.0
GREEDY_VALUE = 0.625


def greedy_state_dict(seed=0):
    """Zero weights, pi_head.1.bias = 128 * (a seeded permutation of 0..35), V_head.1.bias = 0.625: the logits are the
    biases, and a gap of 128 makes expf of every non-maximal legal term exactly 0 in f32, so the probabilities are an
    exact one-hot row at the largest legal bias."""
    sd = zero_state_dict()
    perm = torch.randperm(36, generator=torch.Generator().manual_seed(seed))
    sd["pi_head.1.bias"] = GREEDY_GAP * perm.to(torch.float32)
    sd["V_head.1.bias"] = torch.tensor([GREEDY_VALUE])
    return sd


# the input columns that only ever hold 0 or 1: the 90 classical one-hot columns and column 9 of each quantum row
# (mcts.py:67-85); the other 81 hold 0 or 1/3
BINARY_COLUMNS = tuple(range(90)) + tuple(90 + 10 * v + 9 for v in range(9))
COUNTING_MAX = 256


def counting_state_dict(seed=0):
    """Small signed integer weights, placed so that every hidden activation of the float64 forward is an integer of at
    most 256 (exact in bf16, and exact under f32 accumulation in any order) and every head output a small integer:
      layer 1  dense 0/1 over BINARY_COLUMNS (18 of them are 1 at most), zero rows for the 1/3 columns;  <= 18 + 3
      layer 2  8 taps of +1 per output;                                                                   <= 8 * 21 + 3
      layer 3  one +1 and one -1 tap per output;                                                          <= 171 + 3
      heads    4 taps of +-1 per column;                                                                  |.| <= 4 * 174 + 8
    with integer biases.  Every output of a layer has a tap (every column tile), and the taps of layers 2, 3 and the
    heads reach every group of four inputs (every k-step of both MFMA shapes); layer 1's reach every k-step that
    holds a 0/1 column."""
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)  # noqa: E731
    sd = zero_state_dict()
    cols = torch.tensor(BINARY_COLUMNS)
    sd["fc.0.weight"][:, cols] = ri(0, 1, (256, len(cols)))
    sd["fc.0.bias"] = ri(-6, 3, (256,))
    w2 = sd["fc.2.weight"]
    for o in range(256):                                   # tap t of output o lies in the t-th 32 inputs
        w2[o, torch.arange(8) * 32 + torch.randint(0, 32, (8,), generator=gen)] = 1.0
    sd["fc.2.bias"] = ri(-40, 3, (256,))
    plus = torch.randperm(256, generator=gen)              # every input is some output's +1 tap
    minus = plus.roll(1 + int(torch.randint(0, 254, (1,), generator=gen)))
    w3 = sd["fc.4.weight"]
    w3[torch.arange(256), plus] = 1.0
    w3[torch.arange(256), minus] = -1.0
    sd["fc.4.bias"] = ri(-3, 3, (256,))
    head = torch.zeros((37, 256))
    for c in range(37):                                    # tap t of column c lies in group (4c + t) mod 64 of four inputs
        for t in range(4):
            k = (4 * c + t) % 64 * 4 + int(torch.randint(0, 4, (1,), generator=gen))
            head[c, k] = float(2 * int(torch.randint(0, 2, (1,), generator=gen)) - 1)
    sd["pi_head.1.weight"] = head[:36].clone()
    sd["V_head.1.weight"] = head[36:].clone()
    sd["pi_head.1.bias"] = ri(-8, 8, (36,))
    sd["V_head.1.bias"] = ri(-8, 8, (1,))
    return sd


SHARP_FACTOR = 128.0
SHARP_TIED = 12


def sharp_counting_state_dict(seed=0):
    """counting_state_dict with the policy head (weight and bias) times 128 and its rows tied in threes (row a is row
    a mod 12): the logits are integer multiples of 128 below 2^17 (exact in f32 and bf16 under any accumulation order),
    two legal logits are equal or at least 128 apart, so every expf(logit - max) is exactly 1 or exactly 0 in f32 and
    the probabilities are float32(1) / float32(m) on the m largest legal logits and 0 elsewhere, a set that depends on
    the position: on the network's outputs for which triple is largest, on the board for which of its three actions
    are legal.  The factor alone leaves the counting network's 36 distinct rows tied at the maximum on 2 % of the
    positions of random play; with the tied rows about a sixth of them have m = 1 and the rest m = 2, 3 or 6
    (tests/test_policy_value_numerics_cpu.py asserts the shares)."""
    sd = counting_state_dict(seed)
    rows = torch.arange(36) % SHARP_TIED
    sd["pi_head.1.weight"] = sd["pi_head.1.weight"][rows] * SHARP_FACTOR
    sd["pi_head.1.bias"] = sd["pi_head.1.bias"][rows] * SHARP_FACTOR
    return sd


EXACT_NETS = {"zero": zero_state_dict, "greedy": greedy_state_dict, "sharp": sharp_counting_state_dict}


def forward_reference32(sd, vec):
    """The reference's own operations in torch f32 on the CPU: Model.forward (nn.py:30-42: get_mask, .float(), the
    Sequentials with the heads' leading ReLU, `logits[mask] -= inf`) and Categorical(logits=logits).probs
    (alphazero.py:297-298) row by row as the reference calls it.  vec [N,18,10] -> (value f32[N], logits f32[N,36],
    probs f32[N,36]; a row with no legal action, which the reference never evaluates, is NaN)."""
    from torch.distributions import Categorical
    from torch.nn.functional import linear
    w = {k: sd[k].to(torch.float32) for k in KEYS}
    mask = _mask(vec)
    z = vec.to(torch.float64).flatten(-2, -1).float()
    for i in (0, 2, 4):
        z = torch.relu(linear(z, w["fc.%d.weight" % i], w["fc.%d.bias" % i]))
    v = linear(torch.relu(z), w["V_head.1.weight"], w["V_head.1.bias"]).squeeze(-1)
    logits = linear(torch.relu(z), w["pi_head.1.weight"], w["pi_head.1.bias"])
    logits[mask] -= torch.inf
    probs = torch.full_like(logits, float("nan"))
    for i in torch.nonzero(~mask.all(1)).flatten().tolist():
        probs[i] = Categorical(logits=logits[i]).probs
    return v, logits, probs


def random_play_vectors(n, seed):
    """to_vector rows f32[n,18,10] of n positions of random play on the host (the C oracle): board i has played
    i mod 12 plies with auto-reset, so every depth and finished games are among them."""
    import oracle
    out = []
    for d in range(12):
        m = len(range(d, n, 12))
        if not m:
            continue
        ob = oracle.OracleBoards(m)
        for t in range(d):
            ob.step(ob.sample_actions(seed + d, t, 0, True), None, seed + d, t, 0, True)
        out.append(torch.from_numpy(oracle.to_vector(ob)).to(torch.float32))
    return torch.cat(out)


# ---------------------------------------------------------------- positions on the device (GPU tests only)
def concat_envs(envs, device="cuda:0"):
    """One VecEnv holding the boards of several, in order (the two packed planes, copied)."""
    from qtttgym_amd import VecEnv, _native
    n = sum(e.num_envs for e in envs)
    st = torch.zeros(int(_native.lib().qttt_state_bytes(n)), dtype=torch.uint8, device=device)
    dst, at = st.view(torch.int64).view(2, -1), 0
    for e in envs:
        dst[:, at:at + e.num_envs] = e.state.view(torch.int64).view(2, -1)[:, :e.num_envs]
        at += e.num_envs
    return VecEnv.from_state(st, n, seed=1)


def random_play_env(n, seed, device="cuda:0"):
    """n boards of random play with auto-reset, board i after i mod 12 plies: every depth, finished games included."""
    from qtttgym_amd import VecEnv
    parts = []
    for d in range(12):
        m = len(range(d, n, 12))
        env = VecEnv(m, device=device, seed=seed + d, auto_reset=True)
        if d:
            env.step_random_many(d)
        parts.append(env)
    return concat_envs(parts, device)

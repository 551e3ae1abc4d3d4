"""The numerics of evaluate_kernel on the MI355X, pinned without a bound taken from the kernel: four networks whose
outputs are exact (zero, greedy, counting, sharp counting: bit for bit in both precisions), the precision contract of include/qttt_nn.h
(within 8 x the disagreement of two CPU accumulation dtypes, at weight scales 2^-20, 1 and 4), argmax / masks / row sums
at scale, and non-finite weights (torch's propagation).  Positions: the fixture's 800 and 257 of random play; every
network runs on the whole pool and on batches of 1, 63, 64, 65, 127, 128, 129 and 257 of it (the tile tails of M = 64
and M = 128), whose rows must be the pool's rows bit for bit."""
import pytest
import torch

from nn_reference64 import (GREEDY_VALUE, KEYS, concat_envs, contract_hidden, counting_state_dict, forward64,
                            forward_contract, golden_state_dict, greedy_state_dict, load_golden, random_play_env,
                            random_state_dict, scaled_state_dict, sharp_counting_state_dict, zero_state_dict)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ("value", "logits", "probs")
DTYPES = [torch.float32, torch.bfloat16]
SIZES = (1, 63, 64, 65, 127, 128, 129, 257)
F64, F32 = torch.float64, torch.float32
MARGIN = 8.0                    # kernel deviation <= MARGIN * d_ref: a third summation order, and the maximum of rare
#                                 discrete bf16 rounding flips over ~4e4 outputs varies by a small factor between orders


def _bits(t):
    return t.contiguous().view(torch.int32)


class Pool:
    def __init__(self, g):
        from qtttgym_amd import VecEnv
        fx = VecEnv(len(g["value"]), device=DEV)
        fx.import_boards(g["moves"], g["n_moves"], g["board"], g["qmask"].astype("int16"), g["n_q"])
        self.env = concat_envs([fx, random_play_env(257, 31)])
        self.n = self.env.num_envs
        self.vec = self.env.encode(with_mask=False).cpu()
        assert torch.equal(self.vec[:800], torch.from_numpy(g["vector"]).to(F32))
        self.perm = torch.randperm(self.n, generator=torch.Generator().manual_seed(9))
        self.subs = [self.env.take(self.perm[:n].to(DEV)) for n in SIZES]
        self.legal = torch.isfinite(forward64(zero_state_dict(), self.vec)[1])       # bool [n,36], from the encoding
        self.golden_sd = golden_state_dict(g)
        self._refs = {}

    def evaluate(self, sd, dtype):
        """The kernel's three rows on the whole pool (CPU tensors), after checking that every batch size gives the
        same rows bit for bit."""
        from qtttgym_amd import PolicyValueNet
        net = PolicyValueNet(sd, device=DEV, dtype=dtype)
        out = {k: t.cpu() for k, t in self.env.evaluate(net, rows=ALL).items()}
        for n, sub in zip(SIZES, self.subs):
            part = sub.evaluate(net, rows=ALL)
            for k in ALL:
                assert part[k].shape[0] == n
                assert torch.equal(_bits(part[k].cpu()), _bits(out[k][self.perm[:n]])), (n, k)
        return out

    def weights(self, name, s=1.0):
        sd = self.golden_sd if name == "fixture" else random_state_dict(2024)
        return scaled_state_dict(sd, s)

    def refs(self, name, s, dtype):
        """(ref64, ref32, d_ref): the contract on the CPU accumulated in f64 and in f32, and their largest
        disagreement per output kind."""
        key = (name, s, dtype)
        if key not in self._refs:
            sd = self.weights(name, s)
            r64, r32 = forward_contract(sd, self.vec, dtype, F64), forward_contract(sd, self.vec, dtype, F32)
            self._refs[key] = (r64, r32, deviation(r32, r64))
        return self._refs[key]


def deviation(out, ref):
    """max |Δ| (value, finite logits, non-NaN probs); masked positions and NaN rows must be the same."""
    v, lg, p = (t.double() for t in out)
    rv, rl, rp = (t.double() for t in ref)
    assert torch.equal(torch.isneginf(lg), torch.isneginf(rl)), "masked positions differ"
    assert not torch.isposinf(lg).any() and not torch.isnan(lg).any()
    assert torch.equal(torch.isnan(p), torch.isnan(rp)), "NaN rows differ"
    fin, ok = torch.isfinite(rl), ~torch.isnan(rp)
    return (v - rv).abs().max().item(), (lg[fin] - rl[fin]).abs().max().item(), (p[ok] - rp[ok]).abs().max().item()


@pytest.fixture(scope="module")
def pool():
    return Pool(load_golden())


def _triple(out):
    return tuple(out[k] for k in ALL)


# ---------------------------------------------------------------- exact networks, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_network_is_exactly_uniform(pool, dtype):
    v, lg, p = _triple(pool.evaluate(zero_state_dict(), dtype))
    legal = pool.legal
    k = legal.sum(1)
    assert k.min() == 0 and k.max() == 36 and len(k.unique()) >= 6
    assert not _bits(v).any()                                            # +0.0, not -0.0
    assert not _bits(lg)[legal].any() and torch.isneginf(lg[~legal]).all()
    want = torch.ones(pool.n, dtype=F32) / k.to(F32)                     # float32(1) / float32(k); inf where k = 0
    want = torch.where(legal, want[:, None].expand(-1, 36), torch.zeros(()))
    live = k > 0
    assert torch.equal(_bits(p[live]), _bits(want[live]))
    assert torch.isnan(p[~live]).all() and int((~live).sum()) >= 47


@pytest.mark.parametrize("dtype", DTYPES)
def test_greedy_network_is_an_exact_one_hot(pool, dtype):
    sd = greedy_state_dict()
    v, lg, p = _triple(pool.evaluate(sd, dtype))
    legal, bias = pool.legal, sd["pi_head.1.bias"]
    assert torch.equal(_bits(v), _bits(torch.full((pool.n,), GREEDY_VALUE)))
    assert torch.equal(_bits(lg), _bits(torch.where(legal, bias[None, :].expand(pool.n, -1), torch.tensor(-float("inf")))))
    live = legal.any(1)
    best = torch.where(legal, bias[None, :], torch.tensor(-1.0)).argmax(1)
    want = torch.zeros((pool.n, 36)).scatter_(1, best[:, None], 1.0)
    assert torch.equal(_bits(p[live]), _bits(want[live]))                # exactly 1.0 and exactly +0.0
    assert torch.isnan(p[~live]).all()
    assert len(best[live].unique()) >= 10


def test_counting_network_equals_float64_bit_for_bit(pool):
    sd = counting_state_dict()
    r64, r32 = forward64(sd, pool.vec), forward_contract(sd, pool.vec, torch.float32, F32)
    d_ref = deviation(r32, r64)
    assert d_ref[0] == 0 and d_ref[1] == 0
    outs = {}
    for dtype in DTYPES:
        v, lg, p = outs[dtype] = _triple(pool.evaluate(sd, dtype))
        assert torch.equal(_bits(v), _bits(r64[0].to(F32))), dtype
        assert torch.equal(_bits(lg), _bits(r64[1].to(F32))), dtype
        dp = deviation((v, lg, p), r64)[2]
        print("counting %s: prob d_ref %.3g kernel %.3g" % (dtype, d_ref[2], dp))
        assert dp <= MARGIN * d_ref[2], (dtype, dp, d_ref[2])
    for a, b in zip(outs[torch.float32], outs[torch.bfloat16]):
        assert torch.equal(_bits(a), _bits(b))
    assert len(r64[1][torch.isfinite(r64[1])].unique()) >= 50


@pytest.mark.parametrize("dtype", DTYPES)
def test_sharp_counting_network_is_exactly_uniform_over_the_largest_logits(pool, dtype):
    """Value and logits are the float64 forward's bit for bit, and the probabilities exactly float32(1) / float32(m) on
    the m largest legal logits and +0.0 elsewhere (tests/test_policy_value_numerics_cpu.py proves that the float64
    forward gives exactly these)."""
    sd = sharp_counting_state_dict()
    r64 = forward64(sd, pool.vec)
    v, lg, p = _triple(pool.evaluate(sd, dtype))
    assert torch.equal(_bits(v), _bits(r64[0].to(F32))) and torch.equal(_bits(lg), _bits(r64[1].to(F32)))
    live = pool.legal.any(1)
    tied = r64[1] == r64[1].max(1, keepdim=True).values
    m = tied.sum(1)
    want = torch.where(tied, (torch.ones(pool.n, dtype=F32) / m.to(F32))[:, None], torch.zeros((), dtype=F32))
    assert torch.equal(_bits(p[live]), _bits(want[live])) and torch.equal(_bits(p[live]), _bits(r64[2][live].to(F32)))
    assert torch.isnan(p[~live]).all()
    assert len(m[live].unique()) >= 3 and int((m[live] == 1).sum()) >= 50 and int((m[live] > 1).sum()) >= 50


# ---------------------------------------------------------------- the precision contract, at three weight scales
SCALES = [2.0 ** -20, 1.0, 4.0]
CASES = [(w, s, d) for w in ("fixture", "random") for s in SCALES for d in DTYPES]


def _case_id(c):
    return "%s-s%g-%s" % (c[0], c[1], str(c[2]).split(".")[1])


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_kernel_is_within_the_contract_tolerance(pool, case):
    """ref64 / ref32 = the contract accumulated in f64 / f32 on the CPU; d_ref = their largest disagreement (the size,
    for these inputs, of accumulation-order noise and of the bf16 rounding flips it causes).  The kernel, a third
    order, is within 8 x d_ref of ref64 for each output kind; nothing here is measured on the kernel.  Figures on the
    MI355X: DESIGN.md §10."""
    name, s, dtype = case
    r64, _, d_ref = pool.refs(name, s, dtype)
    dev = deviation(_triple(pool.evaluate(pool.weights(name, s), dtype)), r64)
    fin = torch.isfinite(r64[1])
    rng = (r64[1][fin].max() - r64[1][fin].min()).item()
    print("contract %-7s s=%-9.3g %-8s logit range %9.4g | d_ref value %.3g logit %.3g prob %.3g | kernel value %.3g "
          "logit %.3g prob %.3g" % ((name, s, str(dtype).split(".")[1], rng) + d_ref + dev))
    assert all(d > 0 for d in d_ref)
    assert MARGIN * d_ref[1] < 0.02 * rng, "the logit bound does not bind"
    for kind, d, r in zip(ALL, dev, d_ref):
        assert d <= MARGIN * r, (kind, d, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["fixture", "random"])
def test_argmax_masks_and_row_sums_at_scale_4(pool, name, dtype):
    r64, _, d_ref = pool.refs(name, 4.0, dtype)
    v, lg, p = _triple(pool.evaluate(pool.weights(name, 4.0), dtype))
    assert torch.equal(torch.isneginf(lg), ~pool.legal) and torch.equal(torch.isneginf(r64[1]), ~pool.legal)
    assert not torch.isposinf(lg).any() and not torch.isnan(lg).any() and torch.isfinite(v).all()
    live = pool.legal.any(1)
    assert torch.equal(torch.isnan(p), (~live)[:, None].expand(-1, 36))
    top = torch.topk(r64[1], 2, dim=1).values
    sel = live & ((top[:, 0] - top[:, 1]) > 16 * d_ref[1])              # a single legal action cannot occur (>= 2 squares)
    assert int(sel.sum()) > 100
    assert torch.equal(lg[sel].argmax(1), r64[1][sel].argmax(1))
    assert ((p[live].double().sum(1) - 1).abs() <= 36 * 2.0 ** -23).all()
    assert (p[live] >= 0).all() and (p[live][~pool.legal[live]] == 0).all()


# ---------------------------------------------------------------- non-finite weights: torch's propagation
def _kinds(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    return torch.isnan(t) * 1 + torch.isposinf(t) * 2 + torch.isneginf(t) * 3


def _nan_in_fc2(sd):
    sd["fc.2.weight"][17, 200] = float("nan")


def _inf_in_pi_bias(sd):
    sd["pi_head.1.bias"][8] = float("inf")           # action 8 = squares (1, 2)


def _overflowing_pair(sd):
    # columns 99 and 109 (squares 0 and 1 in no qstruct) are both 1 on most early positions: 3e38 + 3e38 = +inf in f32
    sd["fc.0.weight"][40, 99] = 3e38
    sd["fc.0.weight"][40, 109] = 3e38


def _finite_sums_cannot_overflow(sd, vec, dtype):
    """With f32 accumulation an overflow may depend on the summation order only if the absolute values of a sum's
    finite terms add up beyond the f32 range.  Here they do not (float64 bound, layer by layer, on the contract's own
    activations), except for the pair itself, whose two terms overflow in any order."""
    hid = contract_hidden(sd, vec, dtype, F64)
    lim = float(torch.finfo(F32).max)
    for h, k in zip(hid, ("fc.2", "fc.4", "heads")):
        w = (torch.cat([sd["pi_head.1.weight"], sd["V_head.1.weight"]]) if k == "heads" else sd[k + ".weight"]).double()
        fin = torch.where(torch.isfinite(h.to(F32)), h, torch.zeros((), dtype=F64)).abs()     # f32 infinities apart
        w = torch.where(torch.isfinite(w), w, torch.zeros((), dtype=F64)).abs()
        assert (fin @ w.t()).max().item() + 1.0 < lim, k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutate", [_nan_in_fc2, _inf_in_pi_bias, _overflowing_pair], ids=lambda f: f.__name__.strip("_"))
def test_non_finite_weights_propagate_as_in_torch(pool, mutate, dtype):
    """include/qttt_nn.h: a NaN or an infinity propagates as in torch (relu(NaN) = NaN, 0 * inf = NaN, overflow to inf);
    masked logits stay -inf.  Every NaN / +inf / -inf of the float64-accumulated contract appears in the kernel's
    value and logits at the same positions, and the kernel's pattern is the f32-accumulated contract's (torch's own
    f32 arithmetic: an overflow of the f32 accumulator is not an overflow in float64)."""
    sd = {k: t.clone() for k, t in random_state_dict(2024).items()}
    mutate(sd)
    assert set(sd) == set(KEYS)
    _finite_sums_cannot_overflow(sd, pool.vec, dtype)
    r64, r32 = forward_contract(sd, pool.vec, dtype, F64), forward_contract(sd, pool.vec, dtype, F32)
    out = pool.evaluate(sd, dtype)
    legal = pool.legal
    assert torch.isneginf(out["logits"][~legal]).all() and torch.isneginf(r32[1][~legal]).all()
    hit = 0
    for got, a, b in ((out["value"], r64[0], r32[0]), (out["logits"], r64[1], r32[1])):
        k, k64, k32 = _kinds(got), _kinds(a), _kinds(b)
        bad = (k64 != 0) & (k != k64)
        assert not bad.any(), (int(bad.sum()), k[bad][:8], k64[bad][:8])
        assert torch.equal(k, k32), (int((k != k32).sum()), k[k != k32][:8], k32[k != k32][:8])
        hit += int(((k32 == 1) | (k32 == 2)).sum())
    assert hit > 0, "the case produced no NaN or +inf"
    if mutate is _nan_in_fc2:
        assert torch.isnan(out["value"]).all() and torch.isnan(out["logits"][legal]).all()
    if mutate is _inf_in_pi_bias:
        assert torch.equal(torch.isposinf(out["logits"]), legal & (torch.arange(36) == 8)[None, :])
        assert torch.isfinite(out["value"]).all()
    # probs: NaN at the legal actions of a row that torch makes NaN; masked actions of a row with a legal one stay 0
    p, live = out["probs"], legal.any(1)
    nan_row = torch.isnan(r32[2]).all(1)
    assert torch.equal(torch.isnan(p), torch.where(live[:, None], legal & nan_row[:, None], torch.ones((), dtype=torch.bool)))

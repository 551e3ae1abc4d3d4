"""The references of tests/test_policy_value_numerics_gpu.py, checked without a device: forward_contract (the precision
contract of include/qttt_nn.h on the CPU) against the device run on record in DESIGN.md §10 and against the fixture, and
the conditions that make the zero / greedy / counting / sharp counting networks exact."""
import numpy as np
import pytest
import torch

from nn_reference64 import (BINARY_COLUMNS, COUNTING_MAX, EXACT_NETS, GREEDY_GAP, SHARP_FACTOR, SHARP_TIED,
                            contract_hidden, counting_state_dict, forward64, forward_contract, forward_reference32,
                            golden_state_dict, greedy_state_dict, load_golden, random_play_vectors, scaled_state_dict,
                            sharp_counting_state_dict, zero_state_dict)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def _deviation(out, ref):
    """max |Δ| (value, finite logits, non-NaN probs) of two forward triples."""
    (v, lg, p), (rv, rl, rp) = ([t.double() for t in out], [t.double() for t in ref])
    assert torch.equal(torch.isneginf(lg), torch.isneginf(rl)) and torch.equal(torch.isnan(p), torch.isnan(rp))
    fin, ok = torch.isfinite(rl), ~torch.isnan(rp)
    return (v - rv).abs().max().item(), (lg[fin] - rl[fin]).abs().max().item(), (p[ok] - rp[ok]).abs().max().item()


def test_bf16_emulation_reproduces_the_device_run_on_record(golden):
    """the bf16 kernel on the MI355X differed from the fixture's reference outputs by 0.0071 (value),
    0.022 (logit), 0.0029 (prob).  The CPU emulation of the contract gives the same figures to two significant digits
    (a figure that lies on the boundary between two roundings may show either), so the kernel's whole deviation from
    float64 is the documented rounding, and the emulation is the kernel's arithmetic up to summation order."""
    g = golden
    sd, vec = golden_state_dict(g), torch.from_numpy(g["vector"])
    out = forward_contract(sd, vec, BF16, F64)
    ref = tuple(torch.from_numpy(g[k]) for k in ("value", "logits", "probs"))
    dv, dl, dp = _deviation(out, ref)
    print("bf16 contract emulation against the fixture: value %.4g logit %.4g prob %.4g" % (dv, dl, dp))
    for got, recorded in ((dv, 0.0071), (dl, 0.022), (dp, 0.0029)):
        unit = 10.0 ** (np.floor(np.log10(recorded)) - 1)                # one unit of the second significant digit
        assert abs(got - recorded) <= 0.5 * unit * (1 + 1e-9), (got, recorded)
    # the same emulation accumulated in f32 instead of f64: two orders of magnitude closer than either is to float64
    d32 = _deviation(forward_contract(sd, vec, BF16, F32), out)
    print("bf16 contract emulation, f32 against f64 accumulation: value %.3g logit %.3g prob %.3g" % d32)
    assert d32[0] <= 0.1 * dv and d32[1] <= 0.1 * dl


def test_f32_emulation_is_the_float64_forward_and_reproduces_the_fixture(golden):
    g = golden
    sd, vec = golden_state_dict(g), torch.from_numpy(g["vector"])
    out, ref = forward_contract(sd, vec, F32, F64), forward64(sd, vec)
    for a, b in zip(out, ref):
        assert a.dtype == F64 and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))
    fix = tuple(torch.from_numpy(g[k]) for k in ("value", "logits", "probs"))
    assert max(_deviation(out, fix)) <= 1e-5
    assert max(_deviation(forward_contract(sd, vec, F32, F32), fix)) <= 1e-5
    with pytest.raises(ValueError):
        forward_contract(sd, vec, torch.float16, F64)


def test_scaled_state_dict_scales_the_four_matrices_only(golden):
    sd = golden_state_dict(golden)
    s4 = scaled_state_dict(sd, 4.0)
    for k in sd:
        assert torch.equal(s4[k], sd[k] * 4.0 if k.endswith(".weight") else sd[k]), k
        assert s4[k].data_ptr() != sd[k].data_ptr()
    # a power of two commutes with every rounding of the contract: with zero biases the outputs scale by s^4 exactly
    nb = {k: (t if k.endswith(".weight") else torch.zeros_like(t)) for k, t in sd.items()}
    vec = torch.from_numpy(golden["vector"])[:64]
    a = forward_contract(nb, vec, BF16, F64)
    b = forward_contract(scaled_state_dict(nb, 2.0 ** -20), vec, BF16, F64)
    assert torch.equal(a[0] * 2.0 ** -80, b[0]) and torch.equal((a[1] * 2.0 ** -80), b[1])


@pytest.fixture(scope="module")
def positions(golden):
    """The fixture's 800 positions and 2 000 of random play."""
    return torch.cat([torch.from_numpy(golden["vector"]).to(F32), random_play_vectors(2000, 77)])


def test_binary_columns_hold_only_zero_or_one(positions):
    x = positions.flatten(1)
    cols = torch.tensor(BINARY_COLUMNS)
    assert len(BINARY_COLUMNS) == 99 and ((x[:, cols] == 0) | (x[:, cols] == 1)).all()
    assert x[:, cols].sum(1).max() <= 18
    rest = torch.tensor(sorted(set(range(180)) - set(BINARY_COLUMNS)))
    assert (x[:, rest] == np.float32(1.0 / 3.0)).any() and not (x[:, rest] == 1).any()


def test_counting_network_is_exact_in_bfloat16_and_float32(positions):
    """The condition the GPU test's bit-for-bit comparison rests on, asserted on the construction itself: every hidden
    activation of the float64 forward is an integer in 0..256 that survives bfloat16, every head output survives
    float32, and the outputs are not trivial."""
    sd = counting_state_dict()
    for k, t in sd.items():
        assert torch.equal(t, t.round()) and t.abs().max() <= 40, k
        assert torch.equal(t.to(BF16).to(F32), t), k
    hidden = contract_hidden(sd, positions, F32, F64)
    for h in hidden:
        assert torch.equal(h, h.round()) and h.min() >= 0 and h.max() <= COUNTING_MAX
        assert torch.equal(h.to(BF16).to(F64), h)
        assert (h > 0).float().mean() > 0.2                              # and the layer is alive
    v, lg, p = forward64(sd, positions)
    fin = torch.isfinite(lg)
    for t in (v, lg[fin]):
        assert torch.equal(t, t.round()) and torch.equal(t.to(F32).to(F64), t)
    assert len(torch.unique(lg[fin])) >= 50 and len(torch.unique(v)) >= 20
    # so the contract's forward is float64's in every precision and accumulation dtype
    for dtype in (F32, BF16):
        for acc in (F64, F32):
            out = forward_contract(sd, positions, dtype, acc)
            assert torch.equal(out[0].double(), v) and torch.equal(out[1].double(), lg), (dtype, acc)


def test_counting_network_taps_cover_every_k_step_and_column_tile():
    """k-steps are 4 inputs (f32 MFMA) or 32 (bf16), column tiles 16 outputs: no fragment of the packed matrices that
    can be non-zero is all zero, so a wrong fragment offset or a skipped k-step changes an output."""
    sd = counting_state_dict()
    head = torch.cat([sd["pi_head.1.weight"], sd["V_head.1.weight"]])
    for k in ("fc.2.weight", "fc.4.weight"):
        w = sd[k]
        assert (w != 0).any(1).all(), k                                  # every output column has a tap
        frag = (w != 0).reshape(16, 16, 64, 4).any(3).any(1)             # [column tile, k-step of 4]
        assert frag.any(0).all() and frag.any(1).all(), k
    assert (head != 0).any(1).all() and (head != 0).sum(1).max() <= 4
    assert (head != 0).reshape(37, 64, 4).any(2).any(0).all()
    assert set(head.unique().tolist()) == {-1.0, 0.0, 1.0}
    w1 = sd["fc.0.weight"]
    cols = torch.tensor(BINARY_COLUMNS)
    assert (w1[:, cols] != 0).reshape(16, 16, 99).any(1).all()           # every column tile uses every 0/1 input
    rest = torch.tensor(sorted(set(range(180)) - set(BINARY_COLUMNS)))
    assert not w1[:, rest].any()
    assert (sd["fc.2.weight"] == 1).sum(1).eq(8).all() and not (sd["fc.2.weight"] < 0).any()
    assert (sd["fc.4.weight"] == 1).sum(1).eq(1).all() and (sd["fc.4.weight"] == -1).sum(1).eq(1).all()


def test_greedy_network_is_an_exact_one_hot_in_float32():
    sd = greedy_state_dict()
    bias = sd["pi_head.1.bias"]
    assert sorted((bias / GREEDY_GAP).tolist()) == list(range(36)) and sd["V_head.1.bias"].item() == 0.625
    assert all(not t.any() for k, t in sd.items() if k.endswith(".weight"))
    assert np.exp(np.float32(-GREEDY_GAP)) == np.float32(0.0) and np.exp(np.float32(0.0)) == np.float32(1.0)
    b = bias.numpy()
    rng = np.random.default_rng(5)
    for _ in range(200):                                                 # any set of legal actions
        legal = np.flatnonzero(rng.random(36) < rng.random())
        if not len(legal):
            continue
        e = np.exp((b[legal] - b[legal].max()).astype(np.float32))
        assert e.dtype == np.float32 and e.sum(dtype=np.float32) == np.float32(1.0)
        assert sorted(e.tolist()) == [0.0] * (len(legal) - 1) + [1.0]


def test_zero_network_is_uniform_in_float32(positions):
    sd = zero_state_dict()
    assert len(sd) == 10 and all(not t.any() for t in sd.values())
    v, lg, p = forward_contract(sd, positions[:800], BF16, F32)
    assert not v.any() and not lg[torch.isfinite(lg)].any()
    k = torch.isfinite(lg).sum(1)
    assert k.min() == 0 and k.max() == 36
    for row, kk in zip(p[k > 0][:50], k[k > 0][:50]):
        assert torch.equal(row[row > 0], torch.full((int(kk),), 1.0) / float(kk))


def test_sharp_counting_network_gives_exact_uniform_probabilities_over_the_largest_logits():
    """On random play: the logits are integer multiples of 128 below 2^17, every expf(logit - max) is exactly 1 or 0 in
    f32, the probabilities are float32(1) / float32(m) on the m largest legal logits, and a fair share of the positions
    has m = 1 and a fair share m > 1."""
    sd, base = sharp_counting_state_dict(), counting_state_dict()
    rows = torch.arange(36) % SHARP_TIED
    assert SHARP_FACTOR == 128.0 and np.exp(np.float32(-SHARP_FACTOR)) == np.float32(0.0)
    for k in sd:
        head = k.startswith("pi_head")
        assert torch.equal(sd[k], base[k][rows] * SHARP_FACTOR if head else base[k]), k
        assert torch.equal(sd[k].to(BF16).to(F32), sd[k]) or k.endswith(".bias"), k      # biases stay f32
    vec = random_play_vectors(2000, 77)
    v, lg, p = forward64(sd, vec)
    fin = torch.isfinite(lg)
    live = fin.any(1)
    assert torch.equal(lg[fin], (lg[fin] / 128).round() * 128) and lg[fin].abs().max() < 2 ** 17
    top = torch.where(fin, lg, torch.tensor(-float("inf"), dtype=F64)).max(1, keepdim=True).values
    e = np.exp((lg[live] - top[live]).to(F32).numpy())
    assert e.dtype == np.float32 and set(np.unique(e).tolist()) == {0.0, 1.0}
    tied = torch.from_numpy(e == 1)
    m = tied.sum(1)
    want = torch.where(tied, (torch.ones(len(m), dtype=F32) / m.to(F32))[:, None], torch.zeros((), dtype=F32))
    share_one, share_more = (m == 1).float().mean().item(), (m > 1).float().mean().item()
    print("sharp counting network on %d positions: m = 1 on %.3f, m > 1 on %.3f, m in %s; %d distinct largest actions"
          % (len(m), share_one, share_more, sorted(m.unique().tolist()), len(lg[live].argmax(1).unique())))
    assert share_one >= 0.15 and share_more >= 0.15 and len(m.unique()) >= 3
    assert len(lg[live].argmax(1).unique()) >= 12                                        # the set moves with the position
    # the float64 forward, the contract in both dtypes and accumulations, and the reference's own f32 operations
    # (the f32-accumulated contract on a part of them: it sums term by term in Python)
    n = 300
    outs = [((v, lg, p), len(vec)), (forward_reference32(sd, vec), len(vec))]
    outs += [(forward_contract(sd, vec[:n], dtype, acc), n) for dtype in (F32, BF16) for acc in (F64, F32)]
    for o, n in outs:
        assert torch.equal(o[0].to(F32).view(torch.int32), v[:n].to(F32).view(torch.int32))
        assert torch.equal(o[1].to(F32).view(torch.int32), lg[:n].to(F32).view(torch.int32))
        assert torch.equal(o[2][live[:n]].to(F32).view(torch.int32), want[:int(live[:n].sum())].view(torch.int32))
        assert torch.isnan(o[2][~live[:n]]).all()


@pytest.mark.parametrize("name", sorted(EXACT_NETS))
def test_exact_networks_agree_bit_for_bit_in_every_forward(name):
    """What lets a tree searched by the reference's own class be reproduced without a tolerance: the float64 forward
    rounded to f32, the contract in f32 and bf16, and the reference's chain of torch f32 operations give the same value,
    logits and probabilities bit for bit, and every expf(logit - max) the sampling rule forms is exactly 0 or 1."""
    sd = EXACT_NETS[name]()
    vec = random_play_vectors(240, 5)
    ref = forward64(sd, vec)
    live = torch.isfinite(ref[1]).any(1)
    assert live.any() and not live.all() and torch.isnan(ref[2][~live]).all() and not torch.isnan(ref[2][live]).any()
    outs = [forward_reference32(sd, vec)] + [forward_contract(sd, vec, dtype, F32) for dtype in (F32, BF16)]
    for o in outs:
        for a, b in zip(o, ref):
            a, b = a.to(F32), b.to(F32)
            assert torch.equal(torch.isnan(a), torch.isnan(b))
            assert torch.equal(a.nan_to_num(7.0).view(torch.int32), b.nan_to_num(7.0).view(torch.int32))
    top = ref[1][live].max(1, keepdim=True).values
    e = np.exp((ref[1][live] - top).to(F32).numpy())
    assert set(np.unique(e).tolist()) <= {0.0, 1.0}

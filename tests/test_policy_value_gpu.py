"""VecEnv.evaluate / PolicyValueNet on the MI355X: the reference network's outputs (tests/golden/model_eval.npz, made
from nn.py + model.pt) for f32 and bf16, every batch size shape, argmax agreement, the out / rows conventions, expand()'s
children, weight refresh in place, one kernel per call, and the example that uses it."""
import itertools
import os
import subprocess
import sys

import pytest
import torch

from hip_graph_nodes import kernels_enqueued
from nn_reference64 import forward64, forward64_chunked, golden_state_dict, load_golden, random_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ALL = ("value", "logits", "probs")
# max |Δ| (value, logit, prob) against float64 on any positions, and against the fixture's reference outputs (the MI355X
# run measured f32 7.7e-7 / 6.2e-6 / 1.3e-6 and bf16 0.0071 / 0.022 / 0.0029 there: DESIGN.md §10)
BOUNDS = {torch.float32: (1e-4, 1e-4, 1e-5), torch.bfloat16: (0.04, 0.1, 0.02)}
FIXTURE_BOUNDS = {torch.float32: (5e-6, 2e-5, 5e-6), torch.bfloat16: (0.025, 0.06, 0.01)}
# the default-init weights of random_state_dict give logits within a range of about 0.2, where BOUNDS' bf16 0.1 binds
# nothing.  The CPU emulation of the bf16 contract (nn_reference64.forward_contract, 30 000 random-play positions, five
# of the seeds below) differs from float64 by at most 2.9e-4 / 3.0e-4 / 6.7e-5; four times that allows for the larger
# maximum over 1 M boards and is still below 1 % of the logit range.  tests/test_policy_value_numerics_gpu.py holds the
# kernel to the contract itself.
RANDOM_BOUNDS = {torch.float32: BOUNDS[torch.float32], torch.bfloat16: (1.2e-3, 1.2e-3, 3e-4)}
ARGMAX_GAP = {torch.float32: 1e-3, torch.bfloat16: 0.2}
DTYPES = [torch.float32, torch.bfloat16]


def _net(sd, dtype):
    from qtttgym_amd import PolicyValueNet
    return PolicyValueNet(sd, device=DEV, dtype=dtype)


def _golden_env(g):
    from qtttgym_amd import VecEnv
    env = VecEnv(len(g["value"]), device=DEV)
    env.import_boards(g["moves"], g["n_moves"], g["board"], g["qmask"].astype("int16"), g["n_q"])
    return env


def _compare(out, ref, dtype, bounds=BOUNDS):
    """out: the kernel's dict (all three rows); ref: (value, logits, probs) of float64 or of the fixture."""
    bv, bl, bp = bounds[dtype]
    v, lg, p = (out[k].double().cpu() for k in ALL)
    rv, rl, rp = (t.double().cpu() for t in ref)
    assert torch.equal(torch.isneginf(lg), torch.isneginf(rl)), "masked positions differ"
    assert not torch.isposinf(lg).any() and not torch.isnan(lg).any()
    assert torch.equal(torch.isnan(p), torch.isnan(rp)), "NaN rows differ"
    assert torch.equal(torch.isnan(p).all(1), torch.isnan(p).any(1))
    fin, ok = torch.isfinite(rl), ~torch.isnan(rp)
    dv = (v - rv).abs().max().item() if len(v) else 0.0
    dl = (lg[fin] - rl[fin]).abs().max().item() if fin.any() else 0.0
    dp = (p[ok] - rp[ok]).abs().max().item() if ok.any() else 0.0
    assert dv <= bv and dl <= bl and dp <= bp, (dtype, dv, dl, dp)
    return dv, dl, dp


def _argmax_agrees(lg, rl, dtype):
    top = torch.topk(rl.double().cpu(), 2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    sel = gap > ARGMAX_GAP[dtype]                      # NaN gaps (all masked) are not selected
    assert torch.equal(lg.cpu()[sel].argmax(1), rl.cpu()[sel].argmax(1))
    return int(sel.sum())


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.mark.parametrize("dtype", DTYPES)
def test_fixture_parity_with_the_reference_network(golden, dtype):
    g = golden
    env = _golden_env(g)
    vec = env.encode(with_mask=False)
    assert torch.equal(vec.cpu(), torch.from_numpy(g["vector"]))   # the boards are the fixture's
    out = env.evaluate(_net(golden_state_dict(g), dtype), rows=ALL)
    torch.cuda.synchronize()
    ref = tuple(torch.from_numpy(g[k]) for k in ALL)
    _compare(out, ref, dtype, FIXTURE_BOUNDS)
    assert int(torch.isnan(out["probs"]).all(1)[:260].sum().item()) == 11       # the terminal parents
    assert _argmax_agrees(out["logits"], ref[1], dtype) > 400


@pytest.mark.parametrize("weights", ["fixture", "random"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 65537, 1048576])
def test_sizes_against_float64(golden, n, dtype, weights):
    from qtttgym_amd import VecEnv
    sd = golden_state_dict(golden) if weights == "fixture" else random_state_dict(1000 + n)
    env = VecEnv(n, device=DEV, seed=n, auto_reset=True)
    env.step_random_many(3 + n % 11)                   # mixed depths: auto-reset restarts finished games
    out = env.evaluate(_net(sd, dtype), rows=ALL)
    ref = forward64_chunked(sd, env.encode(with_mask=False))
    torch.cuda.synchronize()
    _compare(out, ref, dtype, BOUNDS if weights == "fixture" else RANDOM_BOUNDS)
    _argmax_agrees(out["logits"], ref[1], dtype)


def test_state_is_not_modified_and_out_is_reused(golden):
    from qtttgym_amd import VecEnv
    env = VecEnv(5000, device=DEV, seed=3, auto_reset=True)
    env.step_random_many(5)
    before = env.state.clone()
    net = _net(golden_state_dict(golden), torch.float32)
    out = env.evaluate(net, rows=ALL)
    first = {k: t.clone() for k, t in out.items()}
    ptrs = {k: t.data_ptr() for k, t in out.items()}
    for t in out.values():
        t.fill_(12345.0)
    again = env.evaluate(net, out=out)
    torch.cuda.synchronize()
    assert again is out and {k: t.data_ptr() for k, t in again.items()} == ptrs
    for k in ALL:
        assert torch.equal(again[k].nan_to_num(7.0), first[k].nan_to_num(7.0)), k
    assert torch.equal(env.state, before)
    with pytest.raises(ValueError):
        env.evaluate(net, rows=("value", "q"))
    with pytest.raises(ValueError):
        env.evaluate(net, out={"logits": torch.empty((4999, 36), device=DEV)})
    with pytest.raises(ValueError):
        env.evaluate(object())


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_rows_subset_gives_the_same_numbers(golden, dtype):
    from qtttgym_amd import VecEnv
    env = VecEnv(3000, device=DEV, seed=4, auto_reset=True)
    env.step_random_many(6)
    net = _net(golden_state_dict(golden), dtype)
    full = env.evaluate(net, rows=ALL)
    for r in range(1, 4):
        for rows in itertools.combinations(ALL, r):
            part = env.evaluate(net, rows=rows)
            assert sorted(part) == sorted(rows)
            for k in rows:
                assert torch.equal(part[k].nan_to_num(7.0), full[k].nan_to_num(7.0)), (rows, k)
    assert sorted(env.evaluate(net)) == ["logits", "value"]


def test_expand_children_evaluate_like_their_copies(golden):
    from qtttgym_amd import VecEnv
    n = 4096
    env = VecEnv(n, device=DEV, seed=5, auto_reset=True)
    env.step_random_many(4)
    net = _net(golden_state_dict(golden), torch.float32)
    a = torch.randint(0, 36, (n,), generator=torch.Generator().manual_seed(5)).to(torch.uint8)
    ex = env.expand(a.to(DEV))
    idx = torch.arange(n, device=DEV)
    for c in ("child0", "child1"):
        child = ex[c]
        got = child.evaluate(net, rows=ALL)
        want = child.take(idx).evaluate(net, rows=ALL)
        for k in ALL:
            assert torch.equal(got[k].nan_to_num(7.0), want[k].nan_to_num(7.0)), (c, k)
    ref = forward64(golden_state_dict(golden), ex["child0"].encode(with_mask=False))
    _compare(ex["child0"].evaluate(net, rows=ALL), ref, torch.float32)


def test_load_state_dict_refreshes_in_place(golden):
    from qtttgym_amd import VecEnv
    env = VecEnv(2048, device=DEV, seed=6, auto_reset=True)
    env.step_random_many(3)
    net = _net(golden_state_dict(golden), torch.float32)
    ptr = net.blob.data_ptr()
    a = env.evaluate(net, rows=ALL)
    a = {k: t.clone() for k, t in a.items()}
    sd2 = random_state_dict(7)
    assert net.load_state_dict(sd2) is net
    b = env.evaluate(net, rows=ALL)
    torch.cuda.synchronize()
    assert net.blob.data_ptr() == ptr
    assert not torch.equal(a["value"], b["value"])
    _compare(b, forward64(sd2, env.encode(with_mask=False)), torch.float32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_kernel_per_call(golden, dtype):
    from qtttgym_amd import VecEnv
    env = VecEnv(10000, device=DEV, seed=8, auto_reset=True)
    env.step_random_many(3)
    net = _net(golden_state_dict(golden), dtype)
    out = env.evaluate(net, rows=ALL)
    kernels, nodes = kernels_enqueued(lambda: env.evaluate(net, out=out), DEV)
    assert kernels == 1 and nodes == 1


def test_az_puct_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "az_puct_selfplay.py"), "--games", "256",
                          "--iters", "8", "--sims", "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "P1 (root PUCT, network priors) wins" in out.stdout

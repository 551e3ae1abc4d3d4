"""VecEnv.rollout_policy on the MI355X: every draw is the documented rule's draw (replayed ply by ply against the float64
network), the leaf outputs equal evaluate() bit for bit, the simulation / board_offset layout, sizes and tile tails,
the outcome frequencies of the reference's own AlphaZero._simulate (tests/golden/policy_playout_stats.npz), one kernel
per call, weight refresh, and the AlphaZero example.  With the zero and the greedy network (tests/nn_reference64.py) the
sampler is deterministic in f32 arithmetic, and a host model on the C oracle replays whole launches byte for byte; with
non-finite weights every move stays legal and the fallback is the largest legal action."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import policy_playout_model
from hip_graph_nodes import kernels_enqueued
from nn_reference64 import (forward64, golden_state_dict, greedy_state_dict, load_golden, random_play_env,
                            random_state_dict, zero_state_dict)
from policy_playout_model import legal_list as _legal_list
from policy_playout_model import uniform_choice

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
# how far outside its float64 CDF interval a drawn u may fall: f32 sums in another order, bf16 runs a rounded network
U_SLACK = {torch.float32: 1e-5, torch.bfloat16: 0.02}
STATS = os.path.join(ROOT, "tests", "golden", "policy_playout_stats.npz")


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def _net(sd, dtype):
    from qtttgym_amd import PolicyValueNet
    return PolicyValueNet(sd, device=DEV, dtype=dtype)


def _positions(n, seed=3, plies=5):
    """n boards at mixed depths: random play with auto-reset (finished games included)."""
    from qtttgym_amd import VecEnv
    env = VecEnv(n, device=DEV, seed=seed, auto_reset=True)
    if n:
        env.step_random_many(plies)
    return VecEnv.from_state(env.state.clone(), n, seed=seed + 1)


def _hashes(seed, ids, steps):
    """qttt_hash(seed, id, step) for arrays of ids and steps (host)."""
    import oracle
    return np.array([oracle.hash64(seed, int(i), int(t)) for i, t in zip(ids, steps)], dtype=np.uint64)


def _live(env):
    info = env.node_info(python_key=False)
    return (~info["terminal"]) & (info["legal"] != 0), info


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_choice_is_the_rules_choice(golden, dtype):
    """4 096 boards x 4 simulations with the trace: replayed with step_raw(actions, bits), every ply's bit is h1 >> 31,
    its action is legal, and u lies in that action's interval of the float64 network's CDF; the replay's final boards
    give result and plies exactly."""
    from qtttgym_amd import VecEnv
    from qtttgym_amd.actions import action36_to_pairs
    n, S, t0 = 4096, 4, 1000
    sd = golden_state_dict(golden)
    env = _positions(n)
    out = env.rollout_policy(_net(sd, dtype), n_sims=S, step_idx0=t0, with_plies=True, with_trace=True)
    trace, res, plies = (out[k].cpu() for k in ("trace", "result", "plies"))
    checked = 0
    for s in range(S):
        rep = VecEnv.from_state(env.state.clone(), n, seed=env.seed)
        played = torch.zeros(n, dtype=torch.int64)
        for p in range(9):
            live, _ = _live(rep)
            live = live.cpu()
            tr = trace[:, s, p]
            assert torch.equal(tr != 0xFF, live), (s, p)          # a ply is played iff the game is still on
            played += live.to(torch.int64)
            if not live.any():
                assert (trace[:, s, p:] == 0xFF).all()
                break
            a = (tr & 63).to(torch.int64)
            bit = (tr >> 6).to(torch.int64)
            idx = torch.nonzero(live).flatten()
            h = _hashes(env.seed, idx.numpy() + env.board_offset, np.full(len(idx), t0 + 16 * s + p))
            h1, h2 = h & np.uint64(0xFFFFFFFF), h >> np.uint64(32)
            assert np.array_equal(bit[idx].numpy(), (h1 >> np.uint64(31)).astype(np.int64))
            u = torch.from_numpy((h2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24)
            _, lg, pr = forward64(sd, rep.encode(with_mask=False).cpu())
            lg, pr = lg[idx], pr[idx]
            ai = a[idx]
            assert torch.isfinite(lg.gather(1, ai[:, None])).all(), "an illegal action was drawn"
            hi = pr.cumsum(1).gather(1, ai[:, None])[:, 0]
            lo = hi - pr.gather(1, ai[:, None])[:, 0]
            slack = U_SLACK[dtype]
            bad = (u < lo - slack) | (u > hi + slack)
            assert not bad.any(), (s, p, int(bad.sum()), u[bad][:4], lo[bad][:4], hi[bad][:4])
            checked += len(idx)
            act = torch.where(live, a, torch.full_like(a, 0))
            pairs = action36_to_pairs(act.to(DEV)).clone()
            pairs[~live.to(DEV)] = 255                               # finished lanes: a noop (env.py:36-43)
            rep.step_raw(pairs.contiguous(), bit.to(torch.uint8).to(DEV).contiguous())
        _, info = _live(rep)
        w = info["winner"].cpu().to(torch.int64)
        assert torch.equal(res[:, s].to(torch.int64), torch.where(w < 0, 0, torch.where(w > 0, 1, -1)))
        assert torch.equal(plies[:, s].to(torch.int64), played)
    assert checked > n * S * 2


def _golden_env(g):
    from qtttgym_amd import VecEnv
    env = VecEnv(len(g["value"]), device=DEV)
    env.import_boards(g["moves"], g["n_moves"], g["board"], g["qmask"].astype("int16"), g["n_q"])
    return env


@pytest.mark.parametrize("dtype", DTYPES)
def test_leaf_outputs_equal_evaluate_bit_for_bit(golden, dtype):
    """On the fixture's 800 positions (all-masked terminal rows among them) and on 4 099 random ones."""
    net = _net(golden_state_dict(golden), dtype)
    for env in (_golden_env(golden), _positions(4099, seed=11, plies=6)):
        ev = env.evaluate(net, rows=("value", "probs"))
        for S in (1, 3):
            out = env.rollout_policy(net, n_sims=S, leaf=("value", "probs"))
            assert torch.equal(out["value"].view(torch.int32), ev["value"].view(torch.int32))
            assert torch.equal(out["probs"].view(torch.int32), ev["probs"].view(torch.int32))
    assert int(torch.isnan(_golden_env(golden).rollout_policy(net, leaf=("probs",))["probs"]).all(1).sum()) >= 11


def test_simulation_layout_and_board_offset(golden):
    net = _net(golden_state_dict(golden), torch.float32)
    env = _positions(300, seed=5)
    S, t0 = 5, 77
    many = env.rollout_policy(net, n_sims=S, step_idx0=t0, with_plies=True, with_trace=True)
    for s in range(S):
        one = env.rollout_policy(net, n_sims=1, step_idx0=t0 + 16 * s, with_plies=True, with_trace=True)
        for k in ("result", "plies", "trace"):
            assert torch.equal(many[k][:, s], one[k][:, 0]), (s, k)
    # board_offset shifts the draws exactly as it does for rollout_many: boards k.. at offset k = rows k.. at offset 0
    k = 37
    sub = env.take(torch.arange(k, 300), board_offset=k)
    part = sub.rollout_policy(net, n_sims=S, step_idx0=t0, with_trace=True)
    assert torch.equal(part["trace"], many["trace"][k:]) and torch.equal(part["result"], many["result"][k:])
    shifted = env.take(torch.arange(300), board_offset=1).rollout_policy(net, n_sims=S, step_idx0=t0, with_trace=True)
    assert not torch.equal(shifted["trace"], many["trace"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_sizes_tails_terminal_leaves_and_out_reuse(golden, dtype):
    """Each board's row depends on the board and its draws only: every batch size (tile tails included) gives the rows
    of the 1 M-board call.  Terminal leaves play no ply and have NaN probs; the input state is not modified."""
    net = _net(golden_state_dict(golden), dtype)
    big = _positions(1 << 20, seed=9, plies=8)
    before = big.state.clone()
    ref = big.rollout_policy(net, with_plies=True, leaf=("probs",))
    assert torch.equal(big.state, before)
    live, info = _live(big)
    assert torch.equal(ref["plies"][:, 0] > 0, live)
    assert torch.equal(torch.isnan(ref["probs"]).all(1), info["legal"] == 0)
    w = info["winner"].to(torch.int64)
    dead = ~live
    assert dead.any() and live.any()
    assert torch.equal(ref["result"][dead, 0].to(torch.int64), torch.where(w < 0, 0, torch.where(w > 0, 1, -1))[dead])
    for n in (1, 63, 64, 65, 127, 129, 65537):
        env = big.take(torch.arange(n))
        out = env.rollout_policy(net, n_sims=2, with_plies=True, with_trace=True, leaf=("value", "probs"))
        one = env.rollout_policy(net, n_sims=1, with_plies=True, leaf=("probs",))
        assert torch.equal(one["result"], ref["result"][:n]) and torch.equal(one["plies"], ref["plies"][:n]), n
        assert torch.equal(one["probs"].view(torch.int32), ref["probs"][:n].view(torch.int32)), n
        again = env.rollout_policy(net, n_sims=2, out=out)
        assert again is out and sorted(again) == ["plies", "probs", "result", "trace", "value"]
        fresh = env.rollout_policy(net, n_sims=2, with_plies=True, with_trace=True, leaf=("value", "probs"))
        for k in fresh:
            assert torch.equal(fresh[k].view(torch.uint8), out[k].view(torch.uint8)), (n, k)
        assert torch.equal(out["result"][:, 0], ref["result"][:n, 0])


def test_frequencies_match_the_reference_alphazero_simulate(golden):
    """16 384 f32 simulations per position against the reference's ~1 000 (AlphaZero._simulate on model.pt): each of
    the +1 / -1 / 0 frequencies within 5 combined standard errors (96 comparisons: Bonferroni-safe)."""
    from qtttgym_amd import VecEnv
    with np.load(STATS) as d:
        st = {k: d[k] for k in d.files}
    P, reps, S = len(st["counts"]), 128, 128
    env = VecEnv(P * reps, device=DEV)
    rep = np.repeat(np.arange(P), reps)
    env.import_boards(st["moves"][rep], st["n_moves"][rep], st["board"][rep], st["qmask"][rep].astype("int16"),
                      st["n_q"][rep])
    res = env.rollout_policy(_net(golden_state_dict(golden), torch.float32), n_sims=S)["result"].cpu().numpy()
    res = res.reshape(P, reps * S)
    m = reps * S
    ours = np.stack([(res == 1).sum(1), (res == -1).sum(1), (res == 0).sum(1)], 1) / m
    nref = int(st["n_sims"])
    theirs = st["counts"] / nref
    pool = (ours * m + theirs * nref) / (m + nref)
    se = np.sqrt(pool * (1 - pool) * (1.0 / m + 1.0 / nref))
    z = np.abs(ours - theirs) / np.maximum(se, 1e-12)
    assert (z <= 5.0).all(), (z.max(), np.argwhere(z > 5.0), ours[z.max(1) > 5], theirs[z.max(1) > 5])
    assert np.abs(ours - theirs).max() < 0.1


def test_one_kernel_per_call(golden):
    env = _positions(1000)
    net = _net(golden_state_dict(golden), torch.bfloat16)
    out = env.rollout_policy(net, n_sims=3, with_plies=True, with_trace=True, leaf=("value", "probs"))
    assert kernels_enqueued(lambda: env.rollout_policy(net, n_sims=3, out=out), DEV) == (1, 1)


def test_weight_refresh_changes_the_next_call(golden):
    env = _positions(4096, seed=21)
    net = _net(golden_state_dict(golden), torch.float32)
    blob = net.blob.data_ptr()
    a = env.rollout_policy(net, n_sims=2, with_trace=True)
    net.load_state_dict(random_state_dict(7))
    b = env.rollout_policy(net, n_sims=2, with_trace=True)
    assert net.blob.data_ptr() == blob
    assert not torch.equal(a["trace"], b["trace"])
    net.load_state_dict(golden_state_dict(golden))
    c = env.rollout_policy(net, n_sims=2, with_trace=True)
    assert torch.equal(a["trace"], c["trace"]) and torch.equal(a["result"], c["result"])


# ---------------------------------------------------------------- whole launches replayed on the host
MODEL_BOARDS, MODEL_SIMS, MODEL_T0 = 513, 3, 4321       # 1 539 lanes: tiles of 64 and of 128 lanes straddle boards


def host_playout(env, S, t0, choose):
    """policy_playout_model.host_playout on the boards of `env`, with its seed and board_offset."""
    import oracle
    ex = {k: t.cpu().numpy() for k, t in env.export_boards().items()}
    ob = oracle.boards_from_arrays(ex["board"], ex["moves"], ex["n_moves"], ex["qmask"], ex["n_q"])
    return policy_playout_model.host_playout(ob, env.seed, env.board_offset, S, t0, choose)


def _assert_launch_equals(out, model):
    trace, result, plies, _ = model
    assert np.array_equal(out["trace"].cpu().numpy(), trace)
    assert np.array_equal(out["result"].cpu().numpy(), result)
    assert np.array_equal(out["plies"].cpu().numpy(), plies)


@pytest.fixture(scope="module")
def model_env():
    return random_play_env(MODEL_BOARDS, 41)


def _launch(env, sd, dtype, leaf=()):
    return env.rollout_policy(_net(sd, dtype), n_sims=MODEL_SIMS, step_idx0=MODEL_T0, with_plies=True, with_trace=True,
                              leaf=leaf)


def test_zero_network_samples_uniformly_and_replays_exactly(model_env):
    model = host_playout(model_env, MODEL_SIMS, MODEL_T0, lambda j, p, legal, u: uniform_choice(legal, u))
    assert (model[2] == 0).any() and model[2].max() >= 7 and len(np.unique(model[0] & 63)) == 37
    outs = [_launch(model_env, zero_state_dict(), dtype) for dtype in DTYPES]
    for out in outs:
        _assert_launch_equals(out, model)
    for k in ("trace", "result", "plies"):
        assert torch.equal(outs[0][k], outs[1][k])
    # the f32 rule is not the float64 interval's: u * k is rounded before the comparison.  31 u = 2 - 2^-24 is a tie in
    # f32 and rounds to 2.0, so the third action is played where the float64 CDF interval names the second.
    u, legal = 1082401 * 2.0 ** -24, (1 << 31) - 1
    assert u * 31 < 2.0 and np.float32(u) * np.float32(31) == np.float32(2.0) and uniform_choice(legal, u) == 2
    assert uniform_choice(legal, 1082400 * 2.0 ** -24) == 1


def test_greedy_network_plays_the_largest_bias(model_env):
    sd = greedy_state_dict()
    bias = sd["pi_head.1.bias"].tolist()
    model = host_playout(model_env, MODEL_SIMS, MODEL_T0, lambda j, p, legal, u: max(_legal_list(legal), key=bias.__getitem__))
    legal0 = model[3]
    for dtype in DTYPES:
        out = _launch(model_env, sd, dtype, leaf=("probs",))
        _assert_launch_equals(out, model)
        probs = out["probs"].cpu()
        want = torch.zeros((MODEL_BOARDS, 36))
        for i, lm in enumerate(legal0):
            if lm:
                want[i, max(_legal_list(int(lm)), key=bias.__getitem__)] = 1.0
        live = torch.from_numpy(legal0 != 0)
        assert torch.equal(probs[live].view(torch.int32), want[live].view(torch.int32))
        assert torch.isnan(probs[~live]).all() and (~live).any()


def _nan_policy_head(sd):
    sd["pi_head.1.bias"][:] = float("nan")


def _nan_in_trunk(sd):
    sd["fc.2.weight"][17, 200] = float("nan")


def _inf_bias(sd):
    sd["pi_head.1.bias"][8] = float("inf")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutate", [_nan_policy_head, _nan_in_trunk, _inf_bias], ids=lambda f: f.__name__.strip("_"))
def test_non_finite_weights_keep_every_move_legal(model_env, mutate, dtype):
    """include/qttt_policy_rollout.h: when no comparison of the running sum succeeds (a NaN or an infinite exp-sum), the
    move is the largest legal action.  The host model takes each move from the trace (it asserts that the move is
    legal on the replayed position) unless the rule fixes it: an all-NaN head or trunk, or +inf at a legal action,
    makes the sum NaN."""
    sd = {k: t.clone() for k, t in random_state_dict(7).items()}
    mutate(sd)
    out = _launch(model_env, sd, dtype)
    trace = out["trace"].cpu().numpy().reshape(-1, 9)

    def choose(j, p, legal, u):
        if mutate is not _inf_bias or legal >> 8 & 1:
            return legal.bit_length() - 1
        return int(trace[j, p]) & 63 if trace[j, p] != 0xFF else -1

    model = host_playout(model_env, MODEL_SIMS, MODEL_T0, choose)
    _assert_launch_equals(out, model)
    if mutate is _inf_bias:                               # both branches of the model were taken
        first = model[3][np.repeat(np.arange(MODEL_BOARDS), MODEL_SIMS)].reshape(-1)
        assert ((first >> np.uint64(8)) & np.uint64(1)).any() and (trace[:, 1:] != 0xFF).any()


def test_alphazero_example_beats_random():
    """examples/alphazero_selfplay.py: the reference's AlphaZero._rollout batched over the games (PUCT on the network's
    priors, expand(), network playouts from both children) as P1 against a random P2: well above a random P1's
    52.8 % + its share of double-line games (DESIGN.md §11 records the measured figure)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "alphazero_selfplay.py"), "--games", "256",
                          "--iters", "24", "--sims", "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    assert line.startswith("games 256"), line
    pct = float(line.split("(")[2].split("%")[0])
    assert pct > 85.0, line

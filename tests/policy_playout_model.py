"""The network playout of include/qttt_policy_rollout.h on the host: the draw of one ply, the sampling rule where it is
deterministic in f32 (every e_a exactly 0 or 1: the zero, greedy and sharp counting networks of tests/nn_reference64.py)
and whole launches replayed on the C oracle's boards.  Test infrastructure: tests/test_policy_rollout_gpu.py replays the
kernel's launches with it, tests/tree_model.py and tests/selfplay_model.py play their network playouts with it, and the
generators of tests/golden/az_tree_traces.npz and selfplay_traces.npz take their sample_action draw from it.  A plain
helper module."""
import numpy as np

import oracle

SIM_STRIDE = 16


def draw(h64):
    """(collapse bit, u) of one ply from qttt_hash's 64 bits."""
    h1, h2 = h64 & 0xFFFFFFFF, h64 >> 32
    return h1 >> 31, (h2 >> 8) * 2.0 ** -24


def legal_list(legal):
    return [a for a in range(36) if legal >> a & 1]


def exp_terms(logits, legal):
    """e_a = expf(logit_a - max over the legal logits) as f32[36], 0 at the illegal actions."""
    idx = legal_list(legal)
    lg = np.asarray(logits, dtype=np.float32)
    e = np.zeros(36, dtype=np.float32)
    e[idx] = np.exp(lg[idx] - lg[idx].max())
    assert e.dtype == np.float32
    return e


def exact_choice(legal, e, u):
    """The rule where every e_a is exactly 0 or 1, in f32 as the kernel computes it: S = their number exactly, every
    running sum is a small integer, and the action is the smallest legal a whose running sum exceeds
    float32(u) * float32(S); the largest legal a if rounding leaves none."""
    idx = legal_list(legal)
    e = np.asarray(e, dtype=np.float32)
    assert ((e[idx] == 0) | (e[idx] == 1)).all(), "the rule is not deterministic in f32 here"
    total = e[idx].sum(dtype=np.float32)
    target = np.float32(u) * total
    assert target.dtype == np.float32 and total >= 1
    run = np.float32(0.0)
    for a in idx:
        run = np.float32(run + e[a])
        if run > target:
            return a
    return idx[-1]


def uniform_choice(legal, u):
    """The rule under equal logits: every e_a = expf(0) = 1, S = k exactly, and the action is the r-th legal one for the
    smallest r with float32(r + 1) > float32(u) * float32(k)."""
    return exact_choice(legal, np.ones(36, dtype=np.float32), u)


def logits32(sd, ob):
    """The float64 forward's masked logits of the boards, rounded to f32: f32[n,36] (exact for the exact networks)."""
    import torch
    from nn_reference64 import forward64
    return forward64(sd, torch.from_numpy(oracle.to_vector(ob)))[1].to(torch.float32).numpy()


def probs32(sd, ob):
    """The float64 forward's probabilities rounded to f32: f32[n,36], NaN rows where no action is legal."""
    import torch
    from nn_reference64 import forward64
    return forward64(sd, torch.from_numpy(oracle.to_vector(ob)))[2].to(torch.float32).numpy()


def host_playout(ob, seed, board_offset, S, t0, choose=None, net=None):
    """The documented rule on the C oracle: lane (i, s) of the boards `ob` (OracleBoards) plays until its game is over,
    ply p with (collapse bit, u) = draw(qttt_hash(seed, board_offset + i, t0 + 16 s + p)) and the action
    choose(lane, p, legal mask, u), which must be legal; or, with net = a state dict of an exact network, the action
    exact_choice gives on the network's logits of the lane's position.  Returns trace u8[n,S,9], result i8[n,S], plies
    u8[n,S] and the boards' legal masks."""
    assert (choose is None) != (net is None)
    pair = [oracle.ind2move(a) for a in range(36)]
    n, N = ob.n, ob.n * S
    lanes = oracle.OracleBoards.from_records(np.repeat(ob.b, S))
    trace, plies, legal0 = np.full((N, 9), 0xFF, np.uint8), np.zeros(N, np.uint8), None
    for p in range(9):
        _, terminal, legal, _ = oracle.node_info(lanes)
        legal0 = legal[::S].copy() if p == 0 else legal0
        live = np.flatnonzero((terminal == 0) & (legal != 0))
        if not len(live):
            break
        sub = oracle.OracleBoards.from_records(lanes.b[live])
        logits = logits32(net, sub) if net is not None else None
        acts, bits = np.zeros((len(live), 2), np.uint8), np.zeros(len(live), np.uint8)
        for r, j in enumerate(live):
            i, s = divmod(int(j), S)
            bit, u = draw(oracle.hash64(seed, board_offset + i, t0 + SIM_STRIDE * s + p))
            if net is None:
                a = choose(int(j), p, int(legal[j]), u)
            else:
                a = exact_choice(int(legal[j]), exp_terms(logits[r], int(legal[j])), u)
            assert 0 <= a < 36 and int(legal[j]) >> a & 1, (j, p, a, hex(int(legal[j])))
            acts[r], bits[r], trace[j, p] = pair[a], bit, a | bit << 6
        sub.step(acts, bits)
        lanes.b[live] = sub.b
        plies[live] += 1
    winner = oracle.node_info(lanes)[0]
    result = np.where(winner < 0, 0, np.where(winner > 0, 1, -1)).astype(np.int8)
    return trace.reshape(n, S, 9), result.reshape(n, S), plies.reshape(n, S), legal0

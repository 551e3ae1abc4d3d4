"""The network search and the self-play batch on the MI355X against the reference's own classes: TreeSearch(net=...)
reproduces what the reference's AlphaZero class recorded (tests/golden/az_tree_traces.npz) and SelfPlay(net=...) the
games of its play_game on QTTTGame and the batch of self_play.py's own statements (tests/golden/selfplay_traces.npz),
under the three exact networks of tests/nn_reference64.py, in f32 and in bf16, without a tolerance but for the sum of
pi.  tests/test_az_reference_cpu.py holds the Python models to the same two files."""
import os

import numpy as np
import pytest
import torch

import selfplay_model
import tree_layout
import tree_model
from nn_reference64 import EXACT_NETS
from tree_harness import DEV, env_from_arrays, stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AZ_TREE = os.path.join(ROOT, "tests", "golden", "az_tree_traces.npz")
SELFPLAY = os.path.join(ROOT, "tests", "golden", "selfplay_traces.npz")
DTYPES = [torch.float32, torch.bfloat16]
NETS = sorted(EXACT_NETS)


def _net(name, dtype):
    from qtttgym_amd import PolicyValueNet
    return PolicyValueNet(EXACT_NETS[name](), device=DEV, dtype=dtype)


def _children_ntot(t):
    """i32[G, 36, 2]: Ntot of the root's children per action and child index (-1: none), read from the tree buffer by
    the layout of include/qttt_tree.h."""
    G, cap = t.num_games, t.capacity
    games, nodes, _, _ = tree_layout.decode(t.tree.cpu().numpy(), G, cap)
    out = np.full((G, 36, 2), -1, dtype=np.int32)
    for g in range(G):
        root = nodes[g, games["root"][g]]
        for a in range(36):
            child = int(root["slots"]["child"][a])
            if child < 0:
                continue
            first = child & (tree_layout.CHILD_PAIR - 1)
            for c in range(2 if child & tree_layout.CHILD_PAIR else 1):
                assert first + c < games["used"][g]
                out[g, a, c] = nodes[g, first + c]["Ntot"]
    return out


def _assert_record(t, rec, ci, nodes):
    st = stats(t)
    for k in ("N", "Ntot", "choose"):
        assert np.array_equal(st[k], rec[k][:, ci]), (k, ci)
    for k in ("W", "Q", "P"):                                                    # bit for bit
        assert st[k].dtype == np.float64 and st[k].tobytes() == rec[k][:, ci].tobytes(), (k, ci)
    assert np.array_equal(_children_ntot(t), rec["child_Ntot"][:, ci]), ci
    if nodes:
        assert np.array_equal(st["nodes_used"], rec["n_nodes"][:, ci]), ci
    assert not st["overflow"].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("name", NETS)
def test_tree_search_reproduces_the_reference_alphazero_class(name, dtype):
    """Both groups (one with a board offset above 2^32), every checkpoint; then the move and sync, once without
    compact() in a pool that holds everything and once with compact() in the smallest pool that run needs (its
    rollouts launched without contemplate's host-side bound, which counts two nodes per rollout), which the run
    without compact() outgrows."""
    from qtttgym_amd import TreeSearch
    from qtttgym_amd.actions import action36_to_pairs
    net = _net(name, dtype)
    for grp in (g for g in tree_model.az_golden_groups(AZ_TREE) if g["net"] == name):
        rec, last = grp["records"], len(grp["checkpoints"])
        total = grp["checkpoints"][-1] + grp["after"]
        tight = tree_model.az_tight_capacity(grp)
        for compact in (False, True):
            env = env_from_arrays(grp["arrays"])
            t = TreeSearch(env.num_envs, capacity=tight if compact else 2 + 2 * total, num_simulations=grp["n_sims"],
                           net=net, seed=grp["seed"], board_offset=grp["offset"], device=DEV)
            t.reset(env)
            done = 0
            for ci, c in enumerate(grp["checkpoints"]):
                for _ in range(c - done):
                    t._rollout() if compact else t.contemplate(1)
                done = c
                _assert_record(t, rec, ci, True)
            a = torch.as_tensor(grp["sync_action"], device=DEV)
            env.step_raw(action36_to_pairs(a).contiguous(), torch.as_tensor(grp["sync_bit"], device=DEV).contiguous())
            t.sync(env)
            if compact:
                t.compact()
                assert np.array_equal(t.nodes_used().cpu().numpy(), grp["n_synced"])
            for _ in range(grp["after"]):
                t._rollout() if compact else t.contemplate(1)
            _assert_record(t, rec, last, compact)
            if not compact:
                assert int(t.nodes_used().max()) > tight


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("name", NETS)
def test_selfplay_reproduces_the_reference_play_game_and_batch(name, dtype):
    from qtttgym_amd import SelfPlay
    fx = [f for f in selfplay_model.golden_games(SELFPLAY) if f["net"] == name][0]
    net = _net(name, dtype)
    batches = []
    for compact in (False, True):
        sp = SelfPlay(fx["G"], n_rollouts=fx["n_rollouts"], num_simulations=fx["n_sims"], net=net, seed=fx["seed"],
                      compact=compact, device=DEV)
        batch = sp.play()
        batches.append(batch)
        selfplay_model.assert_games_equal_reference(fx, batch.action36.cpu().numpy(), batch.length.cpu().numpy(),
                                                    batch.winner.cpu().numpy())
        s, pi, mask, v, done = (x.cpu().numpy() for x in batch.flat())
        selfplay_model.assert_rows_equal_reference(fx, s, pi, mask, v, done)
    for k in ("states", "pi", "mask", "done", "v", "action36", "length", "winner"):
        assert torch.equal(getattr(batches[0], k).view(torch.uint8), getattr(batches[1], k).view(torch.uint8)), k

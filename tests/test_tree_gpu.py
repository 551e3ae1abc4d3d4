"""qtttgym_amd.TreeSearch on the MI355X: the reference MCTS's own traces (tests/golden/tree_traces.npz), lockstep with
the float64 model (tests/tree_model.py, driven by tests/tree_harness.py) in both playout modes, ragged batches,
invariants at 65 536 games, sync, the select kernel's sqrt, and playing strength against a random opponent."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
import tree_model
from tree_harness import (DEV, assert_stats_equal, boards, env_from_arrays, export, random_positions, rollout, search,
                          stats)
from tree_harness import net as _net

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tree_traces.npz")


# ---------------------------------------------------------------- (a) the reference's own traces
def test_device_reproduces_the_reference_mcts_traces():
    from qtttgym_amd import TreeSearch
    from qtttgym_amd.actions import action36_to_pairs
    for grp in tree_model.golden_groups(GOLDEN):
        env = env_from_arrays(grp["arrays"])
        G = env.num_envs
        total = grp["checkpoints"][-1] + grp["after"]
        t = TreeSearch(G, capacity=1 + 2 * total + 1, num_simulations=grp["n_sims"], seed=grp["seed"],
                       board_offset=grp["offset"], device=DEV)
        t.reset(env)
        rec = grp["records"]
        done = 0
        for ci, c in enumerate(grp["checkpoints"]):
            t.contemplate(c - done)
            done = c
            st = stats(t)
            for k, r in (("N", "N"), ("W", "W"), ("Q", "Q"), ("Ntot", "Ntot"), ("choose", "choose"),
                         ("nodes_used", "n_nodes")):
                assert np.array_equal(st[k], rec[r][:, ci]), (k, c)
            assert not st["overflow"].any()
        a = torch.as_tensor(grp["sync_action"], device=DEV)
        bits = torch.as_tensor(grp["sync_bit"], device=DEV).contiguous()
        env.step_raw(action36_to_pairs(a).contiguous(), bits)
        t.sync(env)
        t.contemplate(grp["after"])
        st = stats(t)
        for k in ("N", "W", "Q", "Ntot", "choose"):
            assert np.array_equal(st[k], rec[k][:, -1]), k


# ---------------------------------------------------------------- (b, c) lockstep with the model
def _lockstep(G, rollouts, S, net=None, seed=5, offset=17):
    t, m, _ = search(random_positions(G, seed), 3 + 2 * rollouts, S, net=net, seed=seed, offset=offset)
    for _ in range(rollouts):
        rollout(t, m)             # select -> playouts -> backup on the device, the leaves compared
    assert_stats_equal(stats(t), m.root_stats(), ("N", "W", "Q", "P", "Ntot", "choose", "nodes_used"))
    return t, m


def test_lockstep_with_the_model_uniform_playouts():
    t, m = _lockstep(4096, 64, 4)
    # the device's playouts are qttt_rollout_many's, checked here on a sample against the oracle
    leaves = m.select()
    sample = np.arange(0, 4096, 37)
    t.contemplate(1)
    dev = t._out.cpu().numpy()[sample]
    for s in range(4):
        ref = np.array([oracle.rollout(oracle.OracleBoards.from_records(leaves.b[g:g + 1]), 5, 64 * 4 * 16 + s * 16,
                                       17 + int(g))[0][0] for g in sample])
        assert np.array_equal(dev[:, s], ref), s


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lockstep_with_the_model_network_playouts(dtype):
    _lockstep(1024, 24, 4, net=_net(dtype), seed=9)


# ---------------------------------------------------------------- (d) ragged batches
@pytest.mark.parametrize("G", [1, 63, 64, 65, 1000])
def test_ragged_batches(G):
    _lockstep(G, 12, 3, seed=G)


# ---------------------------------------------------------------- (e) invariants at scale
def test_invariants_at_65536_games():
    from qtttgym_amd import TreeSearch
    G, R = 65536, 16
    arrays = random_positions(G, 21)
    env = env_from_arrays(arrays)
    t = TreeSearch(G, capacity=1 + 2 * R + 1, num_simulations=10, seed=1, device=DEV)
    t.reset(env)
    t.contemplate(R)
    st = stats(t)
    info = env.node_info(python_key=False)
    term = info["terminal"].cpu().numpy().astype(bool)
    legal = info["legal"].cpu().numpy().astype(np.uint64)
    assert np.array_equal(st["Ntot"], st["N"].sum(1))
    assert np.array_equal(st["Ntot"], np.where(term, 0, R - 1))
    assert (st["nodes_used"] <= 1 + 2 * R).all() and not st["overflow"].any()
    assert (np.abs(st["Q"]) <= 1.0).all()
    visited = (st["N"] > 0)
    assert not (visited & ((legal[:, None] >> np.arange(36, dtype=np.uint64)) & 1 == 0)).any()
    # every root child is the root's expand(): syncing onto expand()'s child 1 (= child 0 without a collapse) of the
    # most visited action finds it in the tree, so no fresh node is allocated
    a = torch.as_tensor(st["N"].argmax(1).astype(np.uint8), device=DEV)
    kids = env.expand(a, python_key=False)
    t.sync(kids["child1"])
    n2 = t.nodes_used().cpu().numpy()
    assert (n2[~term] == st["nodes_used"][~term]).all()


# ---------------------------------------------------------------- (f) sync
def test_sync_keeps_the_chosen_subtree_and_starts_fresh_otherwise():
    from qtttgym_amd import TreeSearch
    from qtttgym_amd.actions import action36_to_pairs
    G, R = 1024, 40
    arrays = random_positions(G, 33)
    env = env_from_arrays(arrays)
    t = TreeSearch(G, capacity=1 + 2 * R + 2, num_simulations=4, seed=3, device=DEV)
    t.reset(env)
    t.contemplate(R)
    m = tree_model.TreeModel(4, seed=3)
    m.reset(boards(arrays))
    for _ in range(R):
        m.rollout()
    before = stats(t)
    # half the games play the chosen (visited) action, half the least visited legal one (often never expanded)
    legal = env.node_info(python_key=False)["legal"].cpu().numpy().astype(np.uint64)
    lmask = ((legal[:, None] >> np.arange(36, dtype=np.uint64)) & 1) == 1
    least = np.where(lmask, before["N"], 1 << 30).argmin(1)
    act = np.where(np.arange(G) % 2 == 0, before["choose"], least).astype(np.uint8)
    act[~lmask.any(1)] = 255
    bits = (np.arange(G) // 2 % 2).astype(np.uint8)
    env.step_raw(action36_to_pairs(torch.as_tensor(act, device=DEV)).contiguous(), torch.as_tensor(bits, device=DEV))
    t.sync(env)
    m.sync(boards(export(env)))
    after = stats(t)
    ref = m.root_stats()
    assert_stats_equal(after, ref, ("N", "W", "Q", "P", "Ntot", "choose"))
    fresh = after["nodes_used"] > before["nodes_used"]
    assert fresh.any() and (~fresh).any()
    assert (after["Ntot"][fresh] == 0).all()


# ---------------------------------------------------------------- (g) sqrt
def test_select_sqrt_is_correctly_rounded_for_every_reachable_ntot():
    from qtttgym_amd import _native
    L = _native.lib()
    n_max = _native.TREE_MAX_ROLLOUTS
    chunk = 1 << 22
    out = torch.empty(chunk, dtype=torch.float64, device=DEV)
    for first in range(0, n_max, chunk):
        rc = L.qttt_tree_sqrt(first, chunk, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        ref = np.sqrt(np.arange(first, first + chunk, dtype=np.float64))
        dev = out.cpu().numpy()
        bad = np.nonzero(dev != ref)[0]
        assert bad.size == 0, (first + bad[:8], dev[bad[:8]], ref[bad[:8]])


# ---------------------------------------------------------------- (h) strength
def _tournament(p1, games, sims=4):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tree_tournament.py"), "--p1", p1,
                          "--p2", "random", "--games", str(games), "--sims", str(sims)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    line = out.stdout.strip().splitlines()[-1]
    first = float(line.rsplit("(", 1)[1].rstrip(")"))
    return first, line


@pytest.mark.parametrize("p1", ["mcts:200", "az:200"])
def test_tree_search_beats_a_random_opponent(p1):
    """As the first mover against the uniform-random policy, as the root-level examples are measured."""
    rate, line = _tournament(p1, 1024, sims=10)
    print(line)
    assert rate > 0.90, line

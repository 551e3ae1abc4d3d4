"""The exact endgame solver on the GPU at full depth (VecEnv.solve, include/qttt_solve.h): bit for bit against the deep
fixture (tests/golden/solve_deep.npz: sixteenths, the largest trees of its candidates, leaf roots of every winner); the
Bellman equation through the step kernel on boards no recorder drew, at every number of moves played from eight down to
four, which with the leaf rule proves every sampled solution by induction; symmetry and chunking on the large trees.
Nothing here has a tolerance."""
import os
import time

import numpy as np
import pytest
import torch

from test_solve_gpu import assert_equals_fixture, assert_same, bits, env_of, joined

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def deep():
    with np.load(os.path.join(ROOT, "tests", "golden", "solve_deep.npz")) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def four(deep):
    """The four-move boards solved once, in one call at the default boards_per_launch: (indices, SolveResult)."""
    idx = np.flatnonzero(deep["played"] == 4)
    return idx, env_of(deep, idx).solve(min_ply=4)


def odd_sixteenths(x):
    x = np.asarray(x, dtype=np.float64)
    x = x[np.isfinite(x)] * 16
    assert np.array_equal(x, np.round(x))
    return int((x.astype(np.int64) & 1).sum())


# ---------------------------------------------------------------- a. the fixture, bit for bit
def test_four_move_boards_equal_the_fixture_sixteenths_and_the_largest_tree_included(deep, four):
    idx, res = four
    assert len(idx) >= 4 and deep["nodes"][idx].max() >= 29000000
    assert odd_sixteenths(deep["q"][idx]) >= 1                        # an odd 16 q: `sum / 2` of an odd sum is compared
    assert_equals_fixture(res, deep, idx)


def test_five_move_boards_equal_the_fixture(deep):
    idx = np.flatnonzero(deep["played"] == 5)
    assert len(idx) == 64 and odd_sixteenths(deep["q"][idx]) >= 1 and (deep["best"][idx] == 255).any()
    assert_equals_fixture(env_of(deep, idx).solve(min_ply=5), deep, idx)


def test_boards_with_six_or_more_moves_equal_the_fixture_in_one_batch(deep):
    idx = np.flatnonzero(deep["played"] >= 6)
    assert len(idx) == 768
    assert_equals_fixture(env_of(deep, idx).solve(min_ply=6), deep, idx)


def test_four_move_boards_among_skipped_and_late_boards_give_what_they_give_alone(deep, four):
    """More boards than one launch at min_ply 4 holds, the four-move boards on both sides of the launch boundary."""
    from qtttgym_amd import VecEnv
    from qtttgym_amd.solve import default_boards_per_launch
    idx, alone = four
    late_idx = np.flatnonzero(deep["played"] >= 6)[::3]
    early = []
    for k in range(4):
        e = VecEnv(40, seed=31 + k)
        if k:
            e.step_random_many(k)
        early.append(e)
    h = len(idx) // 2
    parts = [early[0], early[1], env_of(deep, idx[:h]), env_of(deep, late_idx), early[2], env_of(deep, idx[h:]), early[3]]
    at = np.cumsum([0] + [p.num_envs for p in parts])
    per = default_boards_per_launch(4)
    assert at[2] < per < at[5] < at[-1]                               # a launch boundary between the two halves
    res = joined(parts).solve(min_ply=4)
    solved = res.solved.cpu().numpy()
    where4 = np.concatenate([np.arange(at[2], at[3]), np.arange(at[5], at[6])])
    where_late = np.arange(at[3], at[4])
    want = np.zeros(at[-1], dtype=bool)                               # no game is over within three moves: all skipped
    want[where4] = want[where_late] = True
    assert np.array_equal(solved, want)
    skipped = torch.from_numpy(~want)
    assert torch.isnan(res.value.cpu()[skipped]).all() and torch.isnan(res.q.cpu()[skipped]).all()
    assert (res.nodes.cpu()[skipped] == 0).all() and (res.best.cpu()[skipped] == 255).all()
    for name in ("value", "q"):
        assert np.array_equal(bits(getattr(res, name))[where4], bits(getattr(alone, name))), name
        assert np.array_equal(bits(getattr(res, name))[where_late], deep[name][late_idx].view(np.uint32)), name
    for name in ("best", "nodes"):
        assert np.array_equal(getattr(res, name).cpu().numpy()[where4], getattr(alone, name).cpu().numpy()), name
        assert np.array_equal(getattr(res, name).cpu().numpy()[where_late], deep[name][late_idx]), name


# ---------------------------------------------------------------- b. Bellman consistency through the step kernel
def leaf_rule(winner, n_played):
    """qttt_solve.h's leaf rule in float64: +1 if `winner` (1 / 0 / -1 = first / second / none) is the player to move, -1
    if it is the other; the first player moves after an even number of moves."""
    w = winner.double()
    r = torch.where(w < 0, torch.zeros_like(w), torch.where(w > 0, torch.ones_like(w), -torch.ones_like(w)))
    return r if n_played % 2 == 0 else 0.0 - r


@pytest.mark.parametrize("k,n", [(4, 8), (5, 256), (6, 2048), (7, 2048), (8, 2048)])
def test_the_solution_of_random_boards_satisfies_the_bellman_equation_over_the_step_kernel(k, n):
    """V and q of a parent with k moves played from the solutions of its children with k + 1, the children made by
    step_raw with explicit collapse bits 0 and 1 (the step kernel, pinned against the reference on its own).  The
    children with nine moves are leaves, so k = 8 rests on the leaf rule alone and every k on the one above it."""
    from qtttgym_amd import VecEnv
    from qtttgym_amd.actions import action36_to_pairs
    t0 = time.perf_counter()
    env = VecEnv(n, seed=7000 + k, auto_reset=False)
    env.step_random_many(k)
    dev = env.device
    info = env.node_info(python_key=False)
    inner = (~info["terminal"].bool() & (info["legal"] != 0)).nonzero(as_tuple=True)[0]
    if inner.numel() == 0:
        pytest.skip("no unfinished board among %d with %d moves played" % (n, k))
    assert k > 6 or 2 * inner.numel() >= n
    parents = env.take(inner)
    m = parents.num_envs
    res = parents.solve(min_ply=k)
    assert res.solved.all()
    legal = ((parents.node_info(python_key=False)["legal"][:, None] >> torch.arange(36, device=dev)) & 1).bool()
    b, a = legal.nonzero(as_tuple=True)
    pairs = action36_to_pairs(a.to(torch.uint8)).contiguous()
    kids, sol, planes = [], [], []
    for bit in (0, 1):
        c = parents.take(b)
        c.step_raw(pairs, bits=torch.full((b.numel(),), bit, dtype=torch.uint8, device=dev))
        r = c.solve(min_ply=k + 1)
        assert r.solved.all()
        kids.append(c)
        sol.append(r)
        planes.append(c.state.view(torch.int64).view(2, -1)[:, :b.numel()])
    differ = (planes[0] != planes[1]).any(dim=0)
    n_children = parents.take(b).expand(a.to(torch.uint8), python_key=False)["n_children"]
    assert torch.equal(differ, n_children == 2)
    # the leaf rule on every leaf child, at the parity of the child's own move count
    leaves = 0
    for c, r in zip(kids, sol):
        ci = c.node_info(python_key=False)
        leaf = ci["terminal"].bool() | (ci["legal"] == 0)
        assert k < 8 or leaf.all()
        want = leaf_rule(ci["winner"], k + 1).float()
        assert np.array_equal(bits(r.value[leaf]), bits(want[leaf]))
        assert (r.nodes[leaf] == 1).all() and (r.best[leaf] == 255).all() and torch.isneginf(r.q[leaf]).all()
        assert (r.best[~leaf] < 36).all() and (r.nodes[~leaf] > 1).all()
        leaves += int(leaf.sum())
    # the Bellman equation, in float64, cast to f32
    v0, v1 = sol[0].value.double(), sol[1].value.double()
    want_q = torch.full((m, 36), NEG_INF, dtype=torch.float64, device=dev)
    want_q[b, a] = 0.0 - (v0 + v1) / 2.0
    assert np.array_equal(bits(res.q), bits(want_q.float()))
    assert torch.equal(torch.isneginf(res.q), ~legal)
    assert np.array_equal(bits(res.value), bits(res.q.max(dim=1).values))
    actions = torch.arange(36, device=dev).expand(m, 36)
    lowest = torch.where(res.q == res.value[:, None], actions, torch.full_like(actions, 36)).min(dim=1).values
    assert torch.equal(res.best.long(), lowest)
    want_nodes = torch.ones(m, dtype=torch.int64, device=dev)
    want_nodes.index_add_(0, b, sol[0].nodes + differ.long() * sol[1].nodes)
    assert torch.equal(res.nodes, want_nodes)
    q = res.q[legal].double().cpu().numpy()
    print("bellman k=%d: parents %d of %d, pairs %d, collapses %d, leaf children %d, distinct q %d, odd sixteenths %d, "
          "nodes max %d, %.2f s" % (k, m, n, b.numel(), int(differ.sum()), leaves, len(np.unique(q)), odd_sixteenths(q),
                                    int(res.nodes.max()), time.perf_counter() - t0))


# ---------------------------------------------------------------- c. chunking and symmetry on a large tree
def test_the_largest_tree_and_a_sixteenth_board_are_the_same_under_a_rotation_and_a_reflection(deep, four):
    from qtttgym_amd import symmetry
    idx, base = four
    nodes = deep["nodes"][idx]
    has16 = np.array([odd_sixteenths(deep["q"][i]) > 0 for i in idx])
    pick = np.unique([int(np.argmax(nodes)), int(np.flatnonzero(has16)[np.argmin(nodes[has16])])])
    env = env_of(deep, idx[pick])
    sel = torch.as_tensor(pick, device=env.device)
    for k in (1, 6):                                                  # a quarter turn; the mirror image turned twice
        img = env.transformed(k).solve(min_ply=4)
        tau = torch.tensor(symmetry.ACTIONS[k], dtype=torch.int64, device=env.device)
        assert img.solved.all()
        assert np.array_equal(bits(img.value), bits(base.value[sel])) and torch.equal(img.nodes, base.nodes[sel]), k
        assert np.array_equal(bits(img.q[:, tau]), bits(base.q[sel])), k  # the image's q at tau(a) is the board's at a


def test_one_board_per_launch_on_the_four_move_boards_equals_the_default(deep, four):
    idx, base = four
    assert_same(env_of(deep, idx).solve(min_ply=4, boards_per_launch=1), base)

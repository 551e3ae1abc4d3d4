"""The exact endgame solver on the GPU (VecEnv.solve, include/qttt_solve.h): bit for bit against the recorded fixture
(tests/golden/solve_positions.npz, from the C oracle), against a route composed of expand, node_info and a torch
back-up, under the board's symmetries, in chunks, and with the call's housekeeping.  Nothing here has a tolerance."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("moves", "n_moves", "board", "qmask", "n_q")
GUARD = 0xA5


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "solve_positions.npz")) as d:
        return {k: d[k] for k in d.files}


def env_of(g, idx):
    from qtttgym_amd import VecEnv
    idx = np.asarray(idx)
    env = VecEnv(len(idx))
    a = {k: g[k][idx] for k in ARRAYS}
    env.import_boards(torch.from_numpy(a["moves"].copy()), torch.from_numpy(a["n_moves"].copy()),
                      torch.from_numpy(a["board"].copy()), torch.from_numpy(a["qmask"].view(np.int16).copy()),
                      torch.from_numpy(a["n_q"].copy()))
    return env


def joined(envs):
    """One VecEnv over the boards of several, in order (plane indexing only)."""
    from qtttgym_amd import VecEnv, _native
    P = torch.cat([e.state.view(torch.int64).view(2, -1)[:, :e.num_envs] for e in envs], dim=1)
    m = P.shape[1]
    st = torch.zeros(int(_native.lib().qttt_state_bytes(m)), dtype=torch.uint8, device=P.device)
    st.view(torch.int64).view(2, -1)[:, :m] = P
    return VecEnv.from_state(st, m)


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def assert_equals_fixture(res, g, idx):
    idx = np.asarray(idx)
    assert res.solved.all()
    assert np.array_equal(bits(res.value), g["value"][idx].view(np.uint32))
    assert np.array_equal(bits(res.q), g["q"][idx].view(np.uint32))
    assert np.array_equal(res.best.cpu().numpy(), g["best"][idx])
    assert np.array_equal(res.nodes.cpu().numpy(), g["nodes"][idx])


def assert_same(a, b):
    for k in ("value", "q"):
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k          # NaN payloads included
    for k in ("best", "nodes", "solved"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ---------------------------------------------------------------- against the fixture
@pytest.mark.parametrize("batch", [1, 63, 64, 65])
def test_late_boards_equal_the_fixture(golden, batch):
    late = np.flatnonzero(golden["played"] >= 6)
    idx = late[(np.arange(batch) * 37 + batch) % len(late)]           # a mix of six, seven and eight moves, leaves among them
    res = env_of(golden, idx).solve(min_ply=6)
    assert_equals_fixture(res, golden, idx)
    assert res.value.dtype == torch.float32 and res.q.shape == (batch, 36) and res.best.dtype == torch.uint8
    assert res.nodes.dtype == torch.int64 and res.solved.dtype == torch.bool


def test_every_late_board_equals_the_fixture(golden):
    idx = np.flatnonzero(golden["played"] >= 6)
    assert_equals_fixture(env_of(golden, idx).solve(min_ply=6), golden, idx)
    assert (golden["best"][idx] == 255).any()                         # leaf roots among them


def test_five_move_boards_equal_the_fixture(golden):
    idx = np.flatnonzero(golden["played"] == 5)
    assert len(idx) == 8
    assert_equals_fixture(env_of(golden, idx).solve(min_ply=5), golden, idx)


def test_two_four_move_boards_equal_the_fixture(golden):
    idx = np.flatnonzero(golden["played"] == 4)
    assert len(idx) == 2
    assert_equals_fixture(env_of(golden, idx).solve(min_ply=4), golden, idx)


# ---------------------------------------------------------------- against a composed device route
def composed(env, played):
    """value, q[36], nodes of the one board of `env` from existing kernels: breadth-first expand over the frontier,
    node_info for winner / terminal / legal, then a torch back-up with max and mean."""
    dev = env.device
    shifts = torch.arange(36, device=dev)
    levels, cur, d = [], env, 0
    while True:
        info = cur.node_info(python_key=False)
        leaf = info["terminal"].bool() | (info["legal"] == 0)
        r = info["winner"].double()
        r = torch.where(r < 0, torch.zeros_like(r), torch.where(r > 0, torch.ones_like(r), -torch.ones_like(r)))
        leaf_value = r if (played + d) % 2 == 0 else 0.0 - r          # the first player moves after an even count
        legal = ((info["legal"][:, None] >> shifts) & 1).bool() & ~leaf[:, None]
        node, action = legal.nonzero(as_tuple=True)
        level = {"leaf": leaf, "leaf_value": leaf_value, "node": node, "action": action, "n": cur.num_envs}
        levels.append(level)
        if node.numel() == 0:
            break
        ex = cur.take(node).expand(action.to(torch.uint8), python_key=False)
        kids = ex["n_children"].long()
        assert bool((kids >= 1).all())
        two = (kids == 2).nonzero(as_tuple=True)[0]
        level["kids"], level["two"] = kids, two
        cur = joined([ex["child0"]] + ([ex["child1"].take(two)] if two.numel() else []))
        d += 1
        assert d <= 9 - played
    value = nodes = None
    for lv in reversed(levels):
        v = lv["leaf_value"].clone()
        cnt = torch.ones(lv["n"], dtype=torch.int64, device=dev)
        q = torch.full((lv["n"], 36), float("-inf"), dtype=torch.float64, device=dev)
        if lv["node"].numel():
            m = lv["node"].numel()
            s, c = value[:m].clone(), nodes[:m].clone()
            s[lv["two"]] += value[m:]
            c[lv["two"]] += nodes[m:]
            pair_q = torch.where(lv["kids"] == 2, 0.0 - s / 2.0, 0.0 - s)
            q[lv["node"], lv["action"]] = pair_q
            best = q.max(dim=1).values
            v = torch.where(lv["leaf"], v, best)
            cnt.index_add_(0, lv["node"], c)
        value, nodes, root_q = v, cnt, q
    return value, root_q, nodes


def test_one_five_move_board_equals_a_route_composed_of_expand_node_info_and_a_torch_backup(golden):
    five = np.flatnonzero(golden["played"] == 5)
    i = five[np.argmin(golden["nodes"][five])]
    env = env_of(golden, [i])
    res = env.solve(min_ply=5)
    value, q, nodes = composed(env, 5)
    assert int(nodes[0]) == int(res.nodes[0]) > 1000
    assert np.array_equal(bits(value.float()), bits(res.value)) and np.array_equal(bits(q.float()), bits(res.q))
    assert int(res.best[0]) == int((q[0] == value[0]).nonzero()[0, 0])


# ---------------------------------------------------------------- the skip rule
def test_early_boards_are_skipped_and_late_ones_give_what_they_give_alone(golden):
    from qtttgym_amd import VecEnv
    late_idx = np.flatnonzero(golden["played"] >= 6)[::3]
    late = env_of(golden, late_idx)
    early = []
    for k in range(4):
        e = VecEnv(5, seed=11 + k)
        if k:
            e.step_random_many(k)
        early.append(e)
    mixed = joined([early[0], early[1], late, early[2], early[3]])
    res = mixed.solve(min_ply=6)
    n_late = len(late_idx)
    is_late = torch.zeros(mixed.num_envs, dtype=torch.bool)
    is_late[10:10 + n_late] = True
    assert torch.equal(res.solved.cpu(), is_late)
    skipped = ~is_late
    assert torch.isnan(res.value.cpu()[skipped]).all() and torch.isnan(res.q.cpu()[skipped]).all()
    assert (res.nodes.cpu()[skipped] == 0).all() and (res.best.cpu()[skipped] == 255).all()
    alone = late.solve(min_ply=6)
    assert_equals_fixture(alone, golden, late_idx)
    for k in ("value", "q"):
        assert np.array_equal(bits(getattr(res, k))[10:10 + n_late], bits(getattr(alone, k))), k
    assert torch.equal(res.best[10:10 + n_late], alone.best) and torch.equal(res.nodes[10:10 + n_late], alone.nodes)
    # a regret is NaN on a skipped board, 0 for the best move of a solved one that is no leaf, +inf for an illegal move
    reg = res.regret(torch.where(res.best < 36, res.best, torch.zeros_like(res.best))).cpu()
    inner = is_late & (res.best.cpu() < 36)
    assert torch.isnan(reg[skipped]).all() and (reg[inner] == 0).all() and inner.any()
    illegal = torch.isneginf(alone.q).float().argmax(dim=1)
    has_illegal = torch.isneginf(alone.q).any(dim=1) & (alone.best < 36)
    assert torch.isposinf(alone.regret(illegal)[has_illegal]).all() and has_illegal.any()


# ---------------------------------------------------------------- symmetry
def test_the_solution_is_the_same_under_every_symmetry(golden):
    from qtttgym_amd import symmetry
    idx = np.concatenate([np.flatnonzero(golden["played"] == 5)[:2], np.flatnonzero(golden["played"] >= 6)[::4]])
    env = env_of(golden, idx)
    base = env.solve(min_ply=5)
    assert_equals_fixture(base, golden, idx)
    for k in range(8):
        img = env.transformed(k).solve(min_ply=5)
        tau = torch.tensor(symmetry.ACTIONS[k], dtype=torch.int64, device=env.device)
        assert np.array_equal(bits(img.value), bits(base.value)) and torch.equal(img.nodes, base.nodes), k
        assert np.array_equal(bits(img.q[:, tau]), bits(base.q)), k       # the image's q at tau(a) is the board's at a
        assert torch.equal(img.solved, base.solved)


# ---------------------------------------------------------------- chunking
def test_three_boards_per_launch_on_ten_boards_equal_one_launch(golden):
    idx = np.concatenate([np.flatnonzero(golden["played"] == 5)[:3], np.flatnonzero(golden["played"] >= 6)[5:12]])
    assert len(idx) == 10
    env = env_of(golden, idx)
    one = env.solve(min_ply=5, boards_per_launch=10)
    assert_equals_fixture(one, golden, idx)
    assert_same(env.solve(min_ply=5, boards_per_launch=3), one)
    assert_same(env.solve(min_ply=5, boards_per_launch=1), one)
    assert_same(env.solve(min_ply=6, boards_per_launch=3), env.solve(min_ply=6, boards_per_launch=None))   # skipped boards too
    with pytest.raises(ValueError):
        env.solve(boards_per_launch=0)
    with pytest.raises(ValueError):
        env.solve(min_ply=3)


# ---------------------------------------------------------------- housekeeping
def test_state_guards_single_outputs_repeat_and_out(golden):
    from qtttgym_amd import SolveResult
    idx = np.concatenate([np.flatnonzero(golden["played"] == 5)[:1], np.flatnonzero(golden["played"] >= 6)[::5]])
    n = len(idx)
    env = env_of(golden, idx)
    dev = env.device
    before = env.state.clone()
    ref = env.solve(min_ply=5)
    assert_equals_fixture(ref, golden, idx)
    assert torch.equal(env.state, before)                             # the boards are read only
    assert_same(env.solve(min_ply=5), ref)                            # two calls agree
    # guard bytes behind every output, and out= written in place
    sizes = {"value": 4 * n, "q": 4 * 36 * n, "best": n, "nodes": 8 * n, "solved": n}
    raw = {k: torch.full((b + 64,), GUARD, dtype=torch.uint8, device=dev) for k, b in sizes.items()}
    out = SolveResult(raw["value"][:4 * n].view(torch.float32), raw["q"][:4 * 36 * n].view(torch.float32).view(n, 36),
                      raw["best"][:n], raw["nodes"][:8 * n].view(torch.int64), raw["solved"][:n].view(torch.bool))
    got = env.solve(min_ply=5, out=out)
    assert got is out and out.value.data_ptr() == raw["value"].data_ptr()
    assert_same(out, ref)
    for k, b in sizes.items():
        assert (raw[k][b:] == GUARD).all(), k
    with pytest.raises(ValueError):
        env.solve(out=(ref.value, ref.q))
    with pytest.raises(ValueError):
        env.solve(out=SolveResult(ref.value[:-1], ref.q, ref.best, ref.nodes, ref.solved))
    # each output alone, the others null: the same bits
    status = (~ref.solved).to(torch.uint8)
    want = {"value": ref.value, "q": ref.q, "best": ref.best, "nodes": ref.nodes, "status": status}
    order = ("value", "q", "best", "nodes", "status")
    for k in order:
        buf = torch.full_like(want[k], 0x5A if want[k].dtype in (torch.uint8, torch.int64) else 7.0)
        ptrs = [buf.data_ptr() if name == k else None for name in order]
        env._call("qttt_solve", env.state.data_ptr(), n, 5, *ptrs)
        assert torch.equal(buf.view(torch.uint8), want[k].view(torch.uint8)), k
    assert torch.equal(env.state, before)

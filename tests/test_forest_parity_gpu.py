"""Every consumer of the re-root walk (csrc/qttt_step_core.h step_reroot) on the MI355X against
tests/golden/step_forest_traces.npz, the reference's recording of forced forest shapes with walks of every length 0..8
(tests/golden/make_golden_forest.py; tests/test_forest_golden_cpu.py holds the coverage): the step kernels in every launch
shape, step_many in its three forms, import, expand / expand_rollout, transform and the Board façade.  Bit for bit."""
import os

import numpy as np
import pytest
import torch

import forest_model as F
import symmetry_model as M
import test_step_parity_gpu as sp
from test_holes_gpu import LAUNCH_SHAPES, tuning  # noqa: F401  (tuning: the fixture that puts the default shape back)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXPORT_KEYS = ("board", "moves", "n_moves", "qmask", "n_q")


def _np(t):
    return t.cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def words(env, n):
    """The n boards' plane words, int64[2, n]."""
    return env.state.view(torch.int64).view(2, -1)[:, :n]


def env_of_words(w):
    """A VecEnv over the boards whose plane words are w int64[2, m]."""
    from qtttgym_amd import VecEnv, _native
    m = w.shape[1]
    st = torch.zeros(int(_native.lib().qttt_state_bytes(m)), dtype=torch.uint8, device="cuda")
    st.view(torch.int64).view(2, -1)[:, :m] = w
    return VecEnv.from_state(st, m)


def assert_rows(env, fx, e, t, tag):
    """env's boards are the fixture's rows (e[i], t[i]): everything qttt_export gives."""
    ex = {k: _np(v) for k, v in env.export_boards().items()}
    for k in EXPORT_KEYS:
        got = ex[k].view(np.uint16) if k == "qmask" else ex[k]
        sp._same(got, fx[k][e, t], k, tag)


def assert_outputs(reward, term, fx, e, t, tag):
    sp._same(_np(reward).view(np.uint32), fx["reward"][e, t].astype(np.float32).view(np.uint32), "reward bits", tag)
    sp._same(_np(term).astype(np.uint8), fx["terminated"][e, t], "terminated", tag)


@pytest.fixture(scope="module")
def forest():
    with np.load(os.path.join(GOLDEN, "step_forest_traces.npz")) as d:
        fx = {k: d[k] for k in d.files}
    E, T = fx["bits"].shape
    fx["E"], fx["T"], fx["all"] = E, T, np.arange(E)
    fx["close"] = F.closing_steps(fx)
    fx["paired"] = np.nonzero(fx["close"] >= 0)[0]
    assert len(fx["paired"]) == E and (fx["close"] >= 1).all()          # every row has a twin; a cycle needs an earlier move
    return fx


@pytest.fixture(scope="module")
def stepped(forest):
    """The fixture stepped once through step_raw, the exported boards held against the fixture at every step: the state
    words after each step, int64[T, 2, E] — what the other tests compare with.  Never written to again."""
    from qtttgym_amd import VecEnv
    E, T = forest["E"], forest["T"]
    env = VecEnv(E)
    W = torch.empty((T, 2, E), dtype=torch.int64, device="cuda")
    for t in range(T):
        r, tm = env.step_raw(_dev(forest["actions"][:, t]), _dev(forest["bits"][:, t]))
        assert_rows(env, forest, forest["all"], np.full(E, t), ("stepped", t))
        assert_outputs(r, tm, forest, forest["all"], np.full(E, t), ("stepped", t))
        W[t] = words(env, E)
    return W


@pytest.fixture(scope="module")
def closing(forest, stepped):
    """The paired rows at their closing move: rows e, step c, the state words before it, the move and its bit."""
    e = forest["paired"]
    c = forest["close"][e]
    pre = stepped[torch.as_tensor(c - 1, device="cuda"), :, torch.as_tensor(e, device="cuda")].t().contiguous()
    return {"e": e, "c": c, "pre": pre, "act": forest["actions"][e, c], "bit": forest["bits"][e, c]}


def test_forest_traces_through_hip(forest):
    sp.check_traces_through_hip(forest)


@pytest.mark.parametrize("bpl,blk", LAUNCH_SHAPES)
def test_forest_traces_in_every_launch_shape(tuning, forest, stepped, bpl, blk):  # noqa: F811
    from qtttgym_amd import VecEnv
    assert tuning(bpl, blk) == 0
    E, T = forest["E"], forest["T"]
    env = VecEnv(E)
    for t in range(T):
        r, tm = env.step_raw(_dev(forest["actions"][:, t]), _dev(forest["bits"][:, t]))
        assert_outputs(r, tm, forest, forest["all"], np.full(E, t), (bpl, blk, t))
        assert torch.equal(words(env, E), stepped[t]), (bpl, blk, t)
    assert_rows(env, forest, forest["all"], np.full(E, T - 1), (bpl, blk))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("outputs", [True, False])
def test_forest_traces_through_step_many(forest, stepped, fused, outputs):
    """Un-fused and fused with every step's outputs kept, and the output-free forms (the un-fused one runs every step but the
    last through the quiet kernel)."""
    from qtttgym_amd import VecEnv
    E, T = forest["E"], forest["T"]
    acts = _dev(forest["actions"].transpose(1, 0, 2))
    bits = _dev(forest["bits"].T)
    env = VecEnv(E)
    if outputs:
        rew = torch.full((T, E), 7.0, dtype=torch.float32, device="cuda")
        term = torch.ones((T, E), dtype=torch.bool, device="cuda")
        env.step_many(acts, bits, reward=rew, terminated=term, fused=fused)
        for t in range(T):
            assert_outputs(rew[t], term[t], forest, forest["all"], np.full(E, t), (fused, t))
    else:
        env._reward.fill_(7.0)
        env._terminated.fill_(False)
        r, tm = env.step_many(acts, bits, fused=fused)
        assert_outputs(r, tm, forest, forest["all"], np.full(E, T - 1), (fused, "last"))
    assert torch.equal(words(env, E), stepped[T - 1]), (fused, outputs)
    assert_rows(env, forest, forest["all"], np.full(E, T - 1), (fused, outputs))


def _import(fx, e, t):
    from qtttgym_amd import VecEnv
    env = VecEnv(len(e))
    env.import_boards(fx["moves"][e, t], fx["n_moves"][e, t], fx["board"][e, t], fx["qmask"][e, t].view(np.int16),
                      fx["n_q"][e, t])
    return env


def test_import_of_every_row_gives_the_stepped_state_words(forest, stepped):
    """import_board's contract: the state that stepping reaches, rooted forest included."""
    E = forest["E"]
    for t in range(forest["T"]):
        env = _import(forest, forest["all"], np.full(E, t))
        bad = torch.nonzero((words(env, E) != stepped[t]).any(0)).flatten()[:8].tolist()
        assert not bad, (t, bad)


def test_stepping_on_from_the_imported_pre_closing_state(forest, closing):
    e, c = closing["e"], closing["c"]
    env = _import(forest, e, c - 1)
    assert torch.equal(words(env, len(e)), closing["pre"])
    r, tm = env.step_raw(_dev(closing["act"]), _dev(closing["bit"]))
    assert_outputs(r, tm, forest, e, c, "closing")
    assert_rows(env, forest, e, c, "closing")


def _node_rows(fx, e, t):
    """winner (mcts.py:52-65), terminal and the legal mask (mcts.py:20-27) from the fixture's rows."""
    p1, p2 = fx["p1_round"][e, t].astype(np.int64), fx["p2_round"][e, t].astype(np.int64)
    winner = np.full(len(e), -1, dtype=np.int8)
    winner[(p1 > 0) & (p2 > 0)] = (p1 < p2)[(p1 > 0) & (p2 > 0)]
    winner[(p1 > 0) & (p2 < 0)] = 1
    winner[(p1 < 0) & (p2 > 0)] = 0
    empty = fx["board"][e, t] == -1
    legal = np.zeros(len(e), dtype=np.int64)
    for a, (lo, hi) in enumerate(M.PAIRS):
        legal |= (empty[:, lo] & empty[:, hi]).astype(np.int64) << a
    return winner, fx["terminated"][e, t].astype(bool), legal


@pytest.mark.parametrize("rollout", [False, True])
def test_expand_at_every_closing_move_gives_both_twins(forest, stepped, closing, rollout):
    from qtttgym_amd.actions import move2ind
    sel = np.nonzero(closing["bit"] == 0)[0]                  # one parent per pair: its bit-0 row, the twin is the bit-1 row
    e0, c = closing["e"][sel], closing["c"][sel]
    e1 = forest["twin"][e0].astype(np.int64)
    assert len(sel) * 2 == len(closing["e"]) and (forest["bits"][e1, c] == 1).all()
    n = len(sel)
    parent = env_of_words(closing["pre"][:, torch.as_tensor(sel, device="cuda")])
    a36 = np.array([move2ind(int(a), int(b)) for a, b in closing["act"][sel]], dtype=np.uint8)
    out = parent.expand_rollout(_dev(a36), n_sims=1) if rollout else parent.expand(_dev(a36))
    assert bool((out["n_children"] == 2).all())
    ct = torch.as_tensor(c, device="cuda")
    for child, rows in ((0, e0), (1, e1)):
        want = stepped[ct, :, torch.as_tensor(rows, device="cuda")].t()
        got = words(out["child%d" % child], n)
        bad = torch.nonzero((got != want).any(0)).flatten()[:8].tolist()
        assert not bad, (child, bad)
        assert_rows(out["child%d" % child], forest, rows, c, ("child", child))
        winner, terminal, legal = _node_rows(forest, rows, c)
        sp._same(_np(out["winner"][:, child]), winner, "winner", child)
        sp._same(_np(out["terminal"][:, child]), terminal, "terminal", child)
        sp._same(_np(out["legal"][:, child]), legal, "legal", child)
        info = out["child%d" % child].node_info(python_key=False)
        sp._same(_np(info["winner"]), winner, "node_info winner", child)
        sp._same(_np(info["terminal"]), terminal, "node_info terminal", child)
        sp._same(_np(info["legal"]), legal, "node_info legal", child)


@pytest.mark.parametrize("k", range(8))
def test_the_mirrored_closing_move_on_the_transformed_state(forest, closing, k):
    from qtttgym_amd import symmetry
    assert tuple(symmetry.CELLS) == M.CELLS                   # symmetry_model's image() permutes by the library's tables
    e, c = closing["e"], closing["c"]
    n = len(e)
    pre = env_of_words(closing["pre"])
    T = pre.transformed(k)
    assert torch.equal(words(T.transformed(symmetry.inverse(k)), n), closing["pre"])
    sigma = np.array(symmetry.CELLS[k], dtype=np.uint8)
    act = closing["act"]
    mbit = np.array([M.mirrored_bit(int(min(a, b)), int(max(a, b)), int(bit), k) for (a, b), bit in zip(act, closing["bit"])],
                    dtype=np.uint8)
    r, tm = T.step_raw(_dev(sigma[act]), _dev(mbit))
    assert_outputs(r, tm, forest, e, c, ("mirrored", k))
    ex = {key: _np(v) for key, v in T.export_boards().items()}
    sp._same(ex["n_moves"], forest["n_moves"][e, c], "n_moves", k)
    for i in range(n):
        board, moves, qmask, n_q = M.image(forest["board"][e[i], c[i]], forest["moves"][e[i], c[i]],
                                           forest["n_moves"][e[i], c[i]], k)
        got = (ex["board"][i].tolist(), ex["moves"][i].tolist(), ex["qmask"][i].view(np.uint16).tolist(), int(ex["n_q"][i]))
        assert got == (board, moves, qmask, n_q), (k, i, int(e[i]))
    # and it is the image of the stepped state
    stepped_env = env_of_words(closing["pre"])
    stepped_env.step_raw(_dev(act), _dev(closing["bit"]))
    assert torch.equal(words(stepped_env.transformed(k), n), words(T, n))


def test_every_eighth_episode_through_the_board_facade(forest):
    from qtttgym_amd import Board, QEvalClassic
    rows = list(range(0, forest["E"], 8))
    boards = [Board(QEvalClassic()) for _ in rows]
    n_before = np.zeros(len(rows), dtype=np.int64)
    for t in range(forest["T"]):
        res = Board.make_moves(boards, [tuple(int(x) for x in forest["actions"][e, t]) for e in rows],
                               [int(forest["bits"][e, t]) for e in rows])
        n_after = forest["n_moves"][rows, t].astype(np.int64)
        assert [x is None for x in res] == (n_after > n_before).tolist(), t
        n_before = n_after
        for b, e in zip(boards, rows):
            nm = int(forest["n_moves"][e, t])
            assert b.board == forest["board"][e, t].tolist(), (e, t)
            assert b.moves == [(int(forest["moves"][e, t, i, 0]), int(forest["moves"][e, t, i, 1]), i) for i in range(nm)], (e, t)
            assert b.qstructs == [set(s for s in range(9) if int(forest["qmask"][e, t, i]) >> s & 1)
                                  for i in range(int(forest["n_q"][e, t]))], (e, t)
    for b, e in zip(boards, rows):
        assert b.check_win() == (int(forest["p1_round"][e, -1]), int(forest["p2_round"][e, -1])), e

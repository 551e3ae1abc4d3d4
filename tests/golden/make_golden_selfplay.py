#!/usr/bin/env python3
"""Generates tests/golden/selfplay_traces.npz from the UNMODIFIED reference's self-play (`self_play.py`: play_game
:43-76 on `qttt.py`'s QTTTGame with its 10 hard-coded simulations, and the batch statements of its `__main__` block,
:186-222) with the reference's own nn.Model, loaded through ref_shim.py, for each of the three exact networks of
tests/nn_reference64.py.  Build container only; the .npz is data (inputs + expected outputs).

Whole games: game g of a network is `play_game(net, N_ROLLOUTS)` itself, with board id g.  Only draws are replaced, as
in make_golden_az_tree.py (whose Source this script uses), with the seeds of qtttgym_amd.SelfPlay.play(SEED): the trees
draw with seed 2 * SEED + 1 and board_offset 0, the rollout index k running on through the game (k = ply * N_ROLLOUTS + i),
and `np.random.choice(self.root.children[action])` in QTTTGame.make_move (qttt.py:169) -> children[the collapse bit of
(SEED, g, ply)], the bit the environment of SelfPlay draws for that game and ply.  `self_play.QTTTGame` is swapped for
a subclass whose do_rollout, _select, _simulate and make_move call the reference's with the bookkeeping that tells the
draws apart; `self_play.Categorical` as in make_golden_az_tree.py.

The batch: the statements of self_play.py's `__main__` block are taken from the parsed file (`ast`) when this script
runs: the assignments before the `for run` loop but `net = Model()`, and the loop's body up to `EPOCHS = ...`, where
the training starts.  They are executed as they stand, in a namespace where `M` and `n_rollouts` are this script's
values (the two constant assignments are replaced in the tree), `trange` is `range`, and `play_game` replays the games
recorded above.  No statement had to be restated.  Recorded per network: s_batch (rounded to f32), pi_batch, mask_batch,
v_batch, done, and per game its actions, collapse bits, winner and number of rows.
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_az_tree import NETS, Patched, SIM_STRIDE, Source, reference_modules  # noqa: E402
import oracle  # noqa: E402  (test infrastructure: the counter hash only)
from nn_reference64 import EXACT_NETS  # noqa: E402

SEED, GAMES, N_ROLLOUTS = 5, 6, 12
N_SIMS = 10                                                 # qttt.py:252, hard-coded


def selfplay_modules():
    reference_modules()
    import qttt as ref_qttt                                 # the reference's qttt.py / self_play.py, unmodified
    import self_play as ref_sp
    return ref_qttt, ref_sp


def tracked_game(ref_qttt, src, log):
    """QTTTGame with the bookkeeping of the draws around the reference's own methods."""
    class Game(ref_qttt.QTTTGame):
        def __init__(self):
            super().__init__()
            src.k, self.ply, self.sim = 0, 0, 0
            log.append({"actions": [], "bits": []})

        def do_rollout(self):
            self.sim = 0
            super().do_rollout()
            src.k += 1

        def _select(self, node):
            src.in_select, src.select_depth, src.draws_this_ply = True, 0, 0
            try:
                return super()._select(node)
            finally:
                src.in_select = False

        def _simulate(self, node):
            src.step = src.k * N_SIMS * SIM_STRIDE + self.sim * SIM_STRIDE
            self.sim += 1
            return super()._simulate(node)

        def make_move(self, action):
            src.move_bit = oracle.collapse_bit(SEED, src.board_id, self.ply)
            src.in_move, src.expanding, src.draws_this_ply = True, True, 0
            try:
                super().make_move(action)
            finally:
                src.in_move = src.expanding = False
            log[-1]["actions"].append(int(action))
            log[-1]["bits"].append(int(src.move_bit))
            self.ply += 1
    return Game


def batch_statements(ref_sp, M, n_rollouts):
    """self_play.py's own statements that build one batch, as an ast.Module: the `__main__` block's assignments before
    the `for run` loop (without `net = Model()`) and that loop's body up to the training epochs."""
    tree = ast.parse(open(ref_sp.__file__).read())
    main = [n for n in tree.body if isinstance(n, ast.If) and isinstance(n.test, ast.Compare)
            and getattr(n.test.left, "id", None) == "__name__"]
    assert len(main) == 1
    body = main[0].body
    loop = [n for n in body if isinstance(n, ast.For) and getattr(n.target, "id", None) == "run"]
    assert len(loop) == 1
    head = [n for n in body[:body.index(loop[0])]
            if not (isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "net")]
    stmts = []
    for n in loop[0].body:
        if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "EPOCHS":
            break
        stmts.append(n)
    else:
        raise AssertionError("the training epochs were not found")
    replaced = 0
    for n in stmts:
        if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) in ("M", "n_rollouts"):
            assert isinstance(n.value, ast.Constant)
            n.value = ast.Constant({"M": M, "n_rollouts": n_rollouts}[n.targets[0].id])
            replaced += 1
    assert replaced == 2
    return ast.fix_missing_locations(ast.Module(body=head + stmts, type_ignores=[]))


def generate(net_name, games=GAMES):
    """Games 0..games-1 of network `net_name` and their batch: a dict of arrays."""
    ref_qttt, ref_sp = selfplay_modules()
    src, log, played = Source(), [], []
    code = compile(batch_statements(ref_sp, games, N_ROLLOUTS), ref_sp.__file__, "exec")
    with Patched(src, [ref_qttt, ref_sp]):
        saved = ref_sp.QTTTGame
        ref_sp.QTTTGame = tracked_game(ref_qttt, src, log)
        try:
            net = ref_sp.Model()                            # the reference's own nn.Model with the exact network
            net.load_state_dict(EXACT_NETS[net_name]())
            for g in range(games):
                src.seed, src.board_id = 2 * SEED + 1, g
                played.append(ref_sp.play_game(net, N_ROLLOUTS))
            replay = iter(played)
            ns = dict(vars(ref_sp))
            ns.update(net=net, trange=lambda n, **kw: range(n), play_game=lambda net_, n_: next(replay))
            exec(code, ns)
            assert next(replay, None) is None
        finally:
            ref_sp.QTTTGame = saved
    length = [len(states) for states, _ in played]
    acts = np.full((games, 9), 255, dtype=np.uint8)
    bits = np.zeros((games, 9), dtype=np.uint8)
    for g, rec in enumerate(log):
        assert len(rec["actions"]) == length[g] - 1
        acts[g, :len(rec["actions"])] = rec["actions"]
        bits[g, :len(rec["bits"])] = rec["bits"]
    s = ns["s_batch"].numpy()
    assert s.dtype == np.float64 and len(s) == sum(length)
    return {"s": s.astype(np.float32), "pi": ns["pi_batch"].numpy(), "mask": ns["mask_batch"].numpy(),
            "v": ns["v_batch"].numpy().astype(np.int8), "done": np.array(ns["done"], dtype=bool),
            "not_done": ns["not_done"].numpy(), "length": np.array(length, dtype=np.uint8),
            "winner": np.array([{True: 1, False: 0, None: -1}[w] for _, w in played], dtype=np.int8),
            "actions": acts, "bits": bits}


def main():
    out = {"nets": np.array(NETS), "seed": np.int64(SEED), "n_rollouts": np.int32(N_ROLLOUTS), "n_sims": np.int32(N_SIMS)}
    for name in NETS:
        d = generate(name)
        assert np.array_equal(d.pop("not_done"), ~d["done"])
        for k, v in d.items():
            out["%s_%s" % (name, k)] = v
        print("%s: %d games, rows %s, winners %s" % (name, len(d["length"]), d["length"].tolist(), d["winner"].tolist()),
              flush=True)
    path = os.path.join(HERE, "selfplay_traces.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d networks x %d games, %d rows, %d B"
          % (path, len(NETS), GAMES, sum(len(out[n + "_s"]) for n in NETS), os.path.getsize(path)))


CHECK = ("sharp", 1)                                        # what --check regenerates: a network, its first games


def check():
    """Regenerates the first game of one network and its batch and compares them with the committed file: the rows of
    the first games are the first rows of the fixture's batch."""
    z = np.load(os.path.join(HERE, "selfplay_traces.npz"))
    name, games = CHECK
    d = generate(name, games)
    assert np.array_equal(d.pop("not_done"), ~d["done"])
    rows = int(d["length"].sum())
    for k, v in d.items():
        n = games if k in ("length", "winner", "actions", "bits") else rows
        want = z["%s_%s" % (name, k)][:n]
        assert v.dtype == want.dtype and v.tobytes() == want.tobytes(), k
    print("selfplay_traces.npz: %s, %d game(s), %d rows regenerated and equal" % (name, games, rows))


if __name__ == "__main__":
    check() if sys.argv[1:] == ["--check"] else main()

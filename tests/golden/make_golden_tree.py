#!/usr/bin/env python3
"""Generates tests/golden/tree_traces.npz from the UNMODIFIED reference MCTS class (`mcts.py`: reset's root, _rollout
:166-176, _backpropogate :175-183, _simulate :185-198, _expand_child :210-221, _step :233-267, _select :269-278,
_uct_select :280-285, get_action_probs :287-289, choose :308-315, sync :317-337), loaded through ref_shim.py.  Build
container only; the .npz is data (inputs + expected outputs).

Every random draw is replaced by the counter hash of include/qttt_tree.h (`oracle.hash64` = qttt_hash), k = the
rollout index since the root was set:
  * in _select: `np.random.choice(children)` at path depth d -> children[bit d of hash(seed, offset + g,
    2^31 + k)], and the qeval draws of _expand_child's _step return the lower square first, so that children are in
    qttt_expand's order (child 0 = the closing move lands on the lower square);
  * in _simulate: the draws of make_golden_playout.py (qttt_rollout_many's), simulation s of rollout k starting at
    step index k * n_sims * 16 + s * 16.
`_select`, `_rollout` and `_simulate` are wrapped on the instance to tell the draws apart; nothing is edited.

Roots are built with their qstructs and assigned to `strat.root` (MCTS.reset would drop the open entanglements of a
non-empty position, include/qttt_tree.h): the empty board, positions 1-6 plies deep and a few finished games.  After
each checkpoint of rollouts: root N, W, Q, Ntot, choose() and len(strat.nodes).  Then choose() is played with a fixed
collapse bit, sync() follows, and more rollouts are recorded the same way.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from ref_shim import load_reference, REFERENCE_ROOT  # noqa: E402
from make_golden_playout import NpStandIn, board_arrays  # noqa: E402
import oracle  # noqa: E402  (test infrastructure: the counter hash only)

SIM_STRIDE = 16
SELECT_BASE = 1 << 31
# (seed, board_offset, n_sims, roots, checkpoints, rollouts after the sync)
GROUPS = ((11, 0, 4, 48, (1, 2, 3, 10, 50, 200), 100),
          (0xBEEF, 5000, 10, 4, (1, 10, 100, 300), 100))


class Source:
    def __init__(self):
        self.seed = self.board_id = self.step = 0
        self.k = 0
        self.in_select = False
        self.select_depth = 0
        self.bit = 0
        self.draws_this_ply = 0

    def choice(self, a, p=None):
        if self.in_select:                                  # _select's pick of a child (mcts.py:276)
            assert p is None
            d = self.select_depth
            self.select_depth += 1
            if len(a) == 1:
                return a[0]
            bits = oracle.hash64(self.seed, self.board_id, SELECT_BASE + self.k) & 0xFFFFFFFF
            return a[(bits >> d) & 1]
        if p is not None:                                   # sample_action (mcts.py:292)
            h = oracle.hash64(self.seed, self.board_id, self.step)
            h1, h2 = h & 0xFFFFFFFF, h >> 32
            self.bit = h1 >> 31
            self.draws_this_ply = 0
            return a[(h2 * len(a)) >> 32]
        self.step += 1                                      # _simulate's pick of a branch ends the ply
        return a[0]

    class _Qeval:
        def __init__(self, outer):
            self.o = outer

        def choice(self, seq):
            assert len(seq) == 2
            o = self.o
            b = 0 if o.in_select else o.bit                 # expansion: lower square first
            out = seq[b ^ (o.draws_this_ply & 1)]
            o.draws_this_ply += 1
            return out


def main():
    qtttgym, _ = load_reference()
    sys.path.insert(0, REFERENCE_ROOT)
    import mcts as ref_mcts                                 # the reference's mcts.py, unmodified
    src = Source()
    qtttgym.qeval.random = Source._Qeval(src)
    ref_mcts.np = NpStandIn(np, src)
    GS = ref_mcts.MCTS.GameState
    rng = random.Random(4242)

    R = {k: [] for k in ("group", "board", "moves", "n_moves", "qmask", "n_q", "sync_action", "sync_bit")}
    C = {k: [] for k in ("N", "W", "Q", "Ntot", "choose", "n_nodes")}
    for gi, (seed, offset, n_sims, count, checkpoints, after) in enumerate(GROUPS):
        for pi in range(count):
            # ---- the root: random play with this script's own collapse bits
            if pi == 0:
                depth = 0
            elif pi < count - 4 or gi > 0:
                depth = 1 + (pi % 6)
            else:
                depth = 9                                   # play to the end: a finished game
            gs = GS([-1] * 9, [], True, None, False)
            game = qtttgym.Board(qtttgym.QEvalClassic())
            for _ in range(depth):
                legal = [a for a in range(36) if gs.board[ref_mcts.ind2move(a)[0]] == -1
                         and gs.board[ref_mcts.ind2move(a)[1]] == -1]
                p1, p2 = gs.check_win()
                if not legal or p1 > 0 or p2 > 0:
                    break
                a = rng.choice(legal)
                b = rng.getrandbits(1)
                for board in (gs, game):
                    src.in_select, src.bit, src.draws_this_ply = False, b, 0
                    board.make_move(ref_mcts.ind2move(a))
            gs.turn = len(gs.moves) % 2 == 0                # MCTS.reset (mcts.py:141)
            gs.update_actions()
            gs.winner, gs.terminal = None, False
            gs.update_winner()
            b_, mv, nm, qm, nq = board_arrays(gs)
            R["group"].append(gi); R["board"].append(b_); R["moves"].append(mv); R["n_moves"].append(nm)
            R["qmask"].append(qm); R["n_q"].append(nq)

            strat = ref_mcts.MCTS(rollouts=1, num_simulations=n_sims)
            strat.game = game
            strat.root = gs
            strat.nodes = {hash(gs): gs}
            inner_select, inner_rollout, inner_simulate = strat._select, strat._rollout, strat._simulate
            sim_count = [0]

            def select(node, _inner=inner_select):
                src.in_select, src.select_depth, src.draws_this_ply = True, 0, 0
                try:
                    return _inner(node)
                finally:
                    src.in_select = False

            def rollout(_inner=inner_rollout):
                sim_count[0] = 0
                _inner()
                src.k += 1

            def simulate(node, _inner=inner_simulate, _S=n_sims):
                src.step = src.k * _S * SIM_STRIDE + sim_count[0] * SIM_STRIDE
                sim_count[0] += 1
                return _inner(node)
            strat._select, strat._rollout, strat._simulate = select, rollout, simulate
            src.seed, src.board_id, src.k = seed, offset + pi, 0

            def record():
                n = strat.root
                N = [0] * 36; W = [0.0] * 36; Q = [0.0] * 36
                for a in n.actions:
                    N[a], W[a], Q[a] = n.N[a], float(n.W[a]), float(n.Q[a])
                C["N"].append(N); C["W"].append(W); C["Q"].append(Q); C["Ntot"].append(n.Ntot)
                C["choose"].append(strat.choose() if n.actions else 255)
                C["n_nodes"].append(len(strat.nodes))

            done = 0
            for c in checkpoints:
                for _ in range(c - done):
                    strat._rollout()
                done = c
                record()
            # ---- play choose() with a fixed collapse bit, sync, more rollouts
            if gs.terminal or not gs.actions:
                R["sync_action"].append(255); R["sync_bit"].append(0)
                C_pad = len(C["N"]) - 1                     # no move: the after-sync record repeats the last one
                for k in C:
                    C[k].append(C[k][C_pad])
                continue
            a = strat.choose()
            b = rng.getrandbits(1)
            src.in_select, src.bit, src.draws_this_ply = False, b, 0
            game.make_move(ref_mcts.ind2move(a))
            strat.sync(a)
            R["sync_action"].append(a); R["sync_bit"].append(b)
            for _ in range(after):
                strat._rollout()
            record()

    n_ck = [len(g[4]) + 1 for g in GROUPS]
    out = {
        "g_seed": np.array([g[0] for g in GROUPS], dtype=np.uint64),
        "g_offset": np.array([g[1] for g in GROUPS], dtype=np.int64),
        "g_n_sims": np.array([g[2] for g in GROUPS], dtype=np.int32),
        "g_count": np.array([g[3] for g in GROUPS], dtype=np.int64),
        "g_after": np.array([g[5] for g in GROUPS], dtype=np.int32),
        "r_group": np.array(R["group"], dtype=np.uint8),
        "r_board": np.array(R["board"], dtype=np.int8), "r_moves": np.array(R["moves"], dtype=np.uint8),
        "r_n_moves": np.array(R["n_moves"], dtype=np.uint8), "r_qmask": np.array(R["qmask"], dtype=np.uint16),
        "r_n_q": np.array(R["n_q"], dtype=np.uint8),
        "r_sync_action": np.array(R["sync_action"], dtype=np.uint8), "r_sync_bit": np.array(R["sync_bit"], dtype=np.uint8),
        "c_N": np.array(C["N"], dtype=np.int32), "c_W": np.array(C["W"], dtype=np.float64),
        "c_Q": np.array(C["Q"], dtype=np.float64), "c_Ntot": np.array(C["Ntot"], dtype=np.int32),
        "c_choose": np.array(C["choose"], dtype=np.uint8), "c_n_nodes": np.array(C["n_nodes"], dtype=np.int32),
    }
    for gi, g in enumerate(GROUPS):
        out["g%d_checkpoints" % gi] = np.array(g[4], dtype=np.int32)
    out["g_records"] = np.array(n_ck, dtype=np.int32)
    path = os.path.join(HERE, "tree_traces.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d roots, %d records, %d terminal, %d B" % (path, len(R["group"]), len(C["N"]),
          int((out["r_sync_action"] == 255).sum()), os.path.getsize(path)))


if __name__ == "__main__":
    main()

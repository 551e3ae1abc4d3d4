"""The value rollout of include/qttt_tree_value.h (qtttgym_amd.TreeSearch(leaf_eval="value")) on the float64 tree
model: ValueTreeModel is tests/tree_model.py's TreeModel with the leaf evaluation and the backed-up value replaced, and
nothing else.  Test infrastructure: tests/test_tree_value_cpu.py checks it by hand on small trees and asserts that the
root pool below drives it through every branch; tests/test_tree_value_gpu.py compares the device's whole trees with it.

The rules, as the header states them.  The leaf's value v is seen by the player to move at the leaf.  A leaf that is
not terminal: v = the network's f32 value, widened to a Python float.  A terminal leaf: the network is not consulted,
v = +1 if the winner is the player to move at the leaf, -1 if it is the other one, 0 if there is none.  The path's edges,
deepest first, get -v, +v, ...  A leaf that is neither terminal nor has priors gets the network's f32 probs, in the
rollout that reaches it; a leaf that has priors (an overflowed select ends on one) keeps them.

Under an exact network of tests/nn_reference64.py the model evaluates its leaves itself (the float64 forward rounded to
f32 is then the kernel's output in either precision); under general weights the test hands backup() the device's
qttt_evaluate rows.  The counting network is in between: its value and logits are exact integers, but its softmax is
whatever expf gives, so a test sets `probs_of` to the device's qttt_evaluate probs and the model keeps its own values.
A plain helper module."""
import numpy as np

import oracle
from tree_model import TreeModel


def terminal_value(winner, turn):
    """The reward of a finished game for the player to move (turn True = the first player): winner 1 / 0 / -1 =
    True / False / None."""
    if winner < 0:
        return 0.0
    return 1.0 if (winner == 1) == bool(turn) else -1.0


class ValueTreeModel(TreeModel):
    """TreeModel(n_sims, ...)'s constructor, n_sims ignored.  select(), sync(), compact(), dump() and the rest are
    inherited; `ends` counts what the rollouts ended on, for the coverage floor of tests/test_tree_value_cpu.py."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.ends = {"terminal": set(), "overflowed": 0, "fresh": 0}
        self.probs_of = None          # leaves (OracleBoards) -> f32[G, 36]; None: the float64 forward's, rounded

    def priors(self, leaves):
        return super().priors(leaves) if self.probs_of is None else self.probs_of(leaves)

    # ---- the leaf evaluation: f32[G] values where TreeModel has i8[G, n_sims] playout results
    def playouts(self, leaves):
        import torch
        from nn_reference64 import forward64
        return forward64(self.net, torch.from_numpy(oracle.to_vector(leaves)))[0].to(torch.float32).numpy()

    # ---- _backpropogate with the leaf's value, and the leaf's priors
    def backup(self, values, probs):
        for g, st in enumerate(self.games):
            nodes = st["nodes"]
            leaf = nodes[st["leaf"]]
            if leaf.terminal:
                r = terminal_value(leaf.winner, leaf.turn)
                self.ends["terminal"].add((leaf.winner, leaf.turn))
            else:
                r = float(np.float32(values[g]))
                if leaf.P is not None:
                    self.ends["overflowed"] += 1
            self._back_up(st, st["path"], r)
            if not leaf.terminal and leaf.P is None:
                self.ends["fresh"] += 1
                leaf.P = {a: float(np.float32(probs[g][a])) for a in leaf.legal}
                leaf.probs = np.array(probs[g], dtype=np.float32)
        self.k += 1


# ---------------------------------------------------------------- the root pool of the value-rollout tests
# plies of random play behind root g (cycled): every depth 0..8, most of them 5 or more; a game that ends on the way
# stays where it ended, so terminal roots are among them
POOL_PLIES = (7, 0, 8, 5, 6, 8, 3, 7, 8, 6, 1, 8, 7, 5, 8, 2, 6, 7, 8, 4, 8, 7)
POOL_SEED = 2027
OVERFLOW_CAPACITY = 12          # nodes per game in the tests' small pool: most games of 40 rollouts overflow it


def root_pool(G, seed=POOL_SEED):
    """G roots as import arrays (tree_harness.search's `arrays`): root g is game g of uniform random play (the oracle's
    draws under `seed`) after POOL_PLIES[g % len] plies, or at its end if that came earlier.  root_pool(G) is the first
    G roots of every larger pool."""
    ob = oracle.OracleBoards(G)
    plies = np.array([POOL_PLIES[g % len(POOL_PLIES)] for g in range(G)])
    for t in range(9):
        frozen = (plies <= t) | (oracle.node_info(ob)[1] != 0)
        before = ob.b.copy()
        acts = ob.sample_actions(seed, t)
        acts[frozen] = (0, 1)
        ob.step(acts, None, seed, t)
        ob.b[frozen] = before[frozen]
    return {"board": ob.board.copy(), "moves": ob.moves, "n_moves": ob.n_moves, "qmask": ob.qmask, "n_q": ob.n_q}

"""Exact leaves of include/qttt_tree_exact.h (qtttgym_amd.TreeSearch(leaf_eval="value", exact_from=M)) on the float64 tree
model: tests/leaf_parallel_model.py's round with the header's two rules, the exact values taken from
tests/solve_model.py.  Test infrastructure: tests/test_tree_exact_cpu.py checks the model's own invariants and the
coverage floor; tests/test_tree_exact_gpu.py compares the device's whole trees, solved flags and leaf rows with it.

ExactRules is a mixin over LeafParallelModel (ExactLeavesModel) and over tests/gumbel_model.py's GumbelModel
(ExactGumbelModel).  Per game st["solved"] = {node index: the exact value, a Python float} is the device's solved bit and
value bits.  backup_batch(values, probs) first applies qttt_tree_solve_leaves to the round in flight (last_rows keeps what
the device's leaf_value / leaf_exact rows must hold), then backs up by qttt_tree_backup_batch_exact's rule.  With
exact_from every rollout is a round, the first after a reset() or sync() included, as TreeSearch.contemplate makes them.
A plain helper module."""
import numpy as np

import solve_model
import tree_model
from gumbel_model import GumbelModel
from leaf_parallel_model import REC_OVERFLOW, LeafParallelModel, terminal_value

EXACT_MIN_PLY, EXACT_MAX_PLY = 6, 9
NODE_SOLVED, NODE_VALUE_SHIFT, NODE_VALUE_MASK = 1 << 4, 16, 63 << 16
SOLVER = solve_model.Solver()           # one memo for every model of a test session


def flag_bits(value):
    """The bits that a solved node with this exact value adds to its flags word."""
    v16 = value * 16
    assert v16 == int(v16) and -16 <= v16 <= 16
    return NODE_SOLVED | ((int(v16) + 16) << NODE_VALUE_SHIFT)


class ExactRules:
    def __init__(self, *args, exact_from=None, **kwargs):
        super().__init__(*args, **kwargs)
        assert exact_from is None or EXACT_MIN_PLY <= int(exact_from) <= EXACT_MAX_PLY
        self.exact_from = None if exact_from is None else int(exact_from)
        self.last_rows = None         # (values f32[G K] after solve_leaves, exact u8[G K]) of the last round
        self.met.update({"eligible": 0, "enumerated": 0, "reused": 0, "same_eligible_leaf": 0, "solved_root_expanded": 0,
                         "eligible_but_overflowed": 0})

    def reset(self, ob):
        super().reset(ob)
        for st in self._games:
            st["solved"] = {}

    # ---- the schedule: with exact_from every rollout is a round
    def rollout(self):
        if self.exact_from is None:
            super().rollout()
        else:
            self._queued += 1

    def contemplate(self, r):
        if self.exact_from is None:
            return super().contemplate(r)
        if r and self.fresh:
            self.round_of(1)
            r -= 1
            self.fresh = False
        K = self.leaves
        for k in [K] * (r // K) + [r % K] * (r % K > 0):
            self.round_of(k)

    # ---- qttt_tree_solve_leaves on the round in flight
    def eligible(self, st, rec):
        leaf = st["nodes"][rec["leaf"]]
        plain = (len(rec["path"]) >= 1 and not leaf.terminal and leaf.P is None
                 and solve_model.played(leaf.rec.tobytes()) >= self.exact_from)
        if plain and rec["flags"] & REC_OVERFLOW:
            self.met["eligible_but_overflowed"] += 1
        return plain and not rec["flags"] & REC_OVERFLOW

    def solve_leaves(self, values):
        values = np.array(values, dtype=np.float32).copy()
        exact = np.zeros(len(values), dtype=np.uint8)
        K = self._round_k
        for g, st in enumerate(self._games):
            seen = set()
            for j, rec in enumerate(self.round[g]):
                if not self.eligible(st, rec):
                    continue
                i = rec["leaf"]
                self.met["eligible"] += 1
                self.met["same_eligible_leaf"] += i in seen
                seen.add(i)
                if i in st["solved"]:
                    self.met["reused"] += 1
                else:
                    self.met["enumerated"] += 1
                    st["solved"][i] = float(SOLVER.value(st["nodes"][i].rec.tobytes())[0])
                values[g * K + j] = np.float32(st["solved"][i])
                exact[g * K + j] = 1
        return values, exact

    # ---- qttt_tree_backup_batch_exact (and, without exact_from, qttt_tree_backup_batch as it is)
    def backup_batch(self, values, probs):
        if self.exact_from is None:
            return super().backup_batch(values, probs)
        assert self.round is not None
        values, exact = self.last_rows = self.solve_leaves(values)
        for g, st in enumerate(self._games):
            nodes = st["nodes"]
            K = self._round_k
            for j, rec in enumerate(self.round[g]):
                i = rec["leaf"]
                leaf = nodes[i]
                row = g * K + j
                solved = len(rec["path"]) >= 1 and i in st["solved"] and not leaf.terminal and leaf.P is None
                if leaf.terminal:
                    r = terminal_value(leaf.winner, leaf.turn)
                elif solved:
                    r = st["solved"][i]
                else:
                    r = float(np.float32(values[row]))
                self._back_up(st, rec["path"], r)
                for n, a in rec["path"]:
                    st["fN"][n, a] -= 1
                    st["fNtot"][n] -= 1
                if not leaf.terminal and leaf.P is None and not solved:
                    self.met["solved_root_expanded"] += i in st["solved"]
                    leaf.P = {a: float(np.float32(probs[row][a])) for a in leaf.legal}
                    leaf.probs = np.array(probs[row], dtype=np.float32)
        self.k += self._round_k
        self.round = None

    # ---- qttt_tree_compact moves the flags with the nodes
    def compact(self):
        for st in self.games:
            keep = tree_model.reachable(st)
            if st["root"] == 0 and len(keep) == len(st["nodes"]):
                continue
            fwd = {old: new for new, old in enumerate(keep)}
            st["solved"] = {fwd[i]: v for i, v in st["solved"].items() if i in fwd}
        super().compact()

    # ---- what the device holds
    def solved_flags(self):
        """Per game {node index: the solved bit and value bits of its flags word}."""
        return [{i: flag_bits(v) for i, v in st["solved"].items()} for st in self.games]

    def solved_counts(self):
        return np.array([len(st["solved"]) for st in self.games], dtype=np.int64)

    def check_invariants(self):
        """A solved node that is not the root has no priors and no expanded child; its value times 16 is an integer in
        [-16, 16] and equals solve_model's."""
        fresh = solve_model.Solver()
        n = 0
        for st in self.games:
            for i, v in st["solved"].items():
                node = st["nodes"][i]
                assert v * 16 == int(v * 16) and -16 <= v * 16 <= 16
                assert v == fresh.solve(node.rec)["value"]
                assert not node.terminal and solve_model.played(node.rec.tobytes()) >= self.exact_from
                if i != st["root"]:
                    assert node.P is None and all(c is None for c in node.children), (i, st["root"])
                n += 1
        return n


class ExactLeavesModel(ExactRules, LeafParallelModel):
    """LeafParallelModel(n_sims, seed=, board_offset=, c_puct=, capacity=, net=, leaves=, virtual_loss=, exact_from=)."""


class ExactGumbelModel(ExactRules, GumbelModel):
    """GumbelModel with exact leaves: contemplate_gumbel's first rollout is a round of one leaf too."""

    def contemplate_gumbel(self, r, **begin):
        if self.exact_from is None:
            return super().contemplate_gumbel(r, **begin)
        if r and self.fresh:
            self.round_of(1)
            r -= 1
            self.fresh = False
        if r == 0:
            return
        self.begin(r, **begin)
        K = self.leaves
        for k in [K] * (r // K) + [r % K] * (r % K > 0):
            self.round_gumbel(k)


# ---------------------------------------------------------------- the roots and the searches that the tests run
ROLLOUTS, CAPACITY, OVERFLOW_CAPACITY, G_MAX = 24, 256, 8, 65
SEED, OFFSET = 5, 17
ARRAYS = ("board", "moves", "n_moves", "qmask", "n_q")
# (network, leaves, exact_from, capacity) of the whole-tree comparisons: leaves x exact_from under one exact network, the
# other exact networks at one shape, and the pool that overflows.  exact_from = 9 solves nothing by the game's own rules
# (the ninth move fills the board: a position with nine moves played is terminal), so it is the search without exact leaves.
WHOLE_CASES = ([("sharp", K, M, CAPACITY) for K in (1, 4, 8) for M in (6, 7, 9)]
               + [(net, 4, 7, CAPACITY) for net in ("zero", "greedy", "counting")]
               + [("sharp", 4, 6, OVERFLOW_CAPACITY), ("zero", 8, 6, OVERFLOW_CAPACITY)])


def fixture():
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_positions.npz")) as d:
        return {k: d[k] for k in d.files}


def roots(G, played=None):
    """Import arrays of G roots: tests/golden/solve_positions.npz's boards with four and five moves played and its first
    six with six, cycled (game g and game g + 16 share a position and differ in their collapse draws); played = n: the
    boards with n moves played alone, cycled."""
    z = fixture()
    if played is None:
        idx = np.concatenate([np.flatnonzero(z["played"] == 4), np.flatnonzero(z["played"] == 5),
                              np.flatnonzero(z["played"] == 6)[:6]])
    else:
        idx = np.flatnonzero(z["played"] == played)
    idx = idx[np.arange(G) % len(idx)]
    return {k: z[k][idx] for k in ARRAYS}, idx


def boards_of(arrays):
    import oracle
    return oracle.boards_from_arrays(arrays["board"], arrays["moves"], arrays["n_moves"], arrays["qmask"], arrays["n_q"])


def searched(net, K, M, capacity, G=G_MAX, probs_of=None, rollouts=ROLLOUTS, stages=False):
    """The model of the G roots under the state dict `net` after `rollouts` rollouts with exact_from = M; stages=True:
    (that model, the moves, the models after the sync and after 2 K + 1 more rollouts without and with a compaction)."""
    import copy
    from leaf_parallel_model import move_of
    m = ExactLeavesModel(1, seed=SEED, board_offset=OFFSET, capacity=capacity, net=net, leaves=K, exact_from=M)
    m.probs_of = probs_of
    m.reset(boards_of(roots(G)[0]))
    m.contemplate(rollouts)
    if not stages:
        return m
    first = copy.deepcopy(m)
    act, bits = move_of(m)
    # every game follows its most visited legal action where a solved child hangs under it, so that solved leaves become roots
    for g, st in enumerate(m.games):
        n = st["nodes"][st["root"]]
        hit = [a for a in n.legal if any(c in st["solved"] for c in (n.children[a] or ()))]
        if hit and not n.terminal:
            act[g] = max(hit, key=lambda a: n.N[a])
    after, _ = tree_model.after_move(m.root_positions(), act, bits)
    m.sync(after)
    out = {"first": first, "synced": copy.deepcopy(m)}
    for compact in (False, True):
        c = copy.deepcopy(m)
        if compact:
            c.compact()
        c.contemplate(2 * K + 1)
        out["second", compact] = c
    return out, act, bits

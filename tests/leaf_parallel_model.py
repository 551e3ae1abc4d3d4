"""Leaf-parallel rounds of include/qttt_tree_leaves.h (qtttgym_amd.TreeSearch(leaf_eval="value", leaves=K)) on the float64
tree model: LeafParallelModel is tests/value_tree_model.py's ValueTreeModel with select_batch(K, virtual_loss) /
backup_batch(values, probs) beside its one-leaf rollout, in Python floats, with the header's formulas in the header's
order.  Test infrastructure: tests/test_tree_leaves_cpu.py checks it by hand on small trees and asserts the coverage
floor; tests/test_tree_leaves_gpu.py compares the device's whole trees, path records and leaf rows with it.

In-flight visits are kept beside the counts (per game st["fN"][node, action] and st["fNtot"][node], empty outside a
round), not inside them: raw_words() gives the device's N and Ntot words (count | in flight << 24) for the comparison in
the middle of a round.

contemplate(R) is TreeSearch.contemplate's schedule: one single rollout first when nothing was contemplated since the last
reset() or sync(), then rounds of K, then one shorter round.  rollout() with leaves > 1 only queues: the queue is run as one
contemplate() when the trees are next looked at (`games`), which is what lets tests/selfplay_model.py's play(), which
calls rollout() R times per move, drive this model.  A plain helper module."""
import math
from collections import Counter

import numpy as np

import oracle
import value_tree_model
from tree_model import SELECT_BASE
from value_tree_model import OVERFLOW_CAPACITY, POOL_SEED, ValueTreeModel, terminal_value  # noqa: F401

MAX_LEAVES = 64
FLIGHT_SHIFT = 24
REC_OVERFLOW, REC_LEAF_TURN, REC_LEAF_TERMINAL = 1, 2, 4

# a path record of include/qttt_tree_leaves.h, by the layout written in that header
PATH_BYTES = 64
PATH_DTYPE = np.dtype({"names": ["leaf", "depth", "flags", "action", "node"],
                       "formats": ["<i4", "u1", "u1", ("u1", (10,)), ("<i4", (10,))],
                       "offsets": [0, 4, 5, 8, 24], "itemsize": PATH_BYTES})


class LeafParallelModel(ValueTreeModel):
    def __init__(self, *args, leaves=1, virtual_loss=1.0, **kwargs):
        self._games, self._queued = [], 0
        super().__init__(*args, **kwargs)
        self.leaves, self.virtual_loss = int(leaves), float(virtual_loss)
        self.fresh = True
        self.round = None             # the records of the round in flight: per game a list of K dicts
        # what the rounds met, for the coverage floor of tests/test_tree_leaves_cpu.py
        self.met = {"shared_edge_below_root": 0, "same_open_leaf": 0, "terminal_in_round": 0, "sibling_entered": 0,
                    "descents_after_overflow": 0, "diverted": 0}

    # ---- rollout() queues while leaves > 1; looking at the trees runs the queue
    @property
    def games(self):
        if self._queued:
            r, self._queued = self._queued, 0
            self.contemplate(r)
        return self._games

    @games.setter
    def games(self, value):
        self._games, self._queued = value, 0

    def reset(self, ob):
        super().reset(ob)
        self.fresh = True

    def sync(self, ob):
        super().sync(ob)
        self.fresh = True

    def rollout(self):
        if self.leaves == 1:
            super().rollout()
        else:
            self._queued += 1

    def contemplate(self, r):
        if self.leaves == 1:
            for _ in range(r):
                super().rollout()
            return
        if r and self.fresh:
            super().rollout()
            r -= 1
            self.fresh = False
        K = self.leaves
        for k in [K] * (r // K) + [r % K] * (r % K > 0):
            self.round_of(k)

    def round_of(self, k):
        leaves = self.select_batch(k, self.virtual_loss)
        self.backup_batch(self.playouts(leaves), self.priors(leaves))

    # ---- the select rule
    def _score_in_flight(self, node, a, f, f_tot, vloss):
        """The score of action a of `node` with f descents in flight through the edge and f_tot through the node."""
        Ne = node.N[a] + f
        We = node.W[a] - vloss * float(f)
        q = We / Ne if Ne else 0.0
        u = node.P[a] * math.sqrt(float(node.Ntot + f_tot)) / (1 + Ne)
        return q + self.c_puct * u

    def select_batch(self, K, virtual_loss):
        """K descents per game, j = 0 .. K-1 in order; returns the G * K leaves as OracleBoards, row g * K + j."""
        assert 1 <= K <= MAX_LEAVES and self.round is None
        games = self.games
        vloss = float(virtual_loss)
        leaves, self.round, self._round_k = [], [], K
        for g, st in enumerate(games):
            nodes = st["nodes"]
            fN, fNtot = st["fN"], st["fNtot"] = Counter(), Counter()

            def score(node, i):
                key = lambda x: self._score_in_flight(node, x, fN[i, x], fNtot[i], vloss)
                if fNtot[i]:
                    plain = max(node.legal, key=lambda x: self._score(node, x))
                    self.met["diverted"] += plain != max(node.legal, key=key)
                return key

            recs = []
            overflowed_before = False
            for j in range(K):
                bits = oracle.hash64(self.seed, self.board_offset + g, SELECT_BASE + self.k + j) & 0xFFFFFFFF
                path, i, over, expanded = self._descend(st, bits, score)
                for n, a in path:
                    fN[n, a] += 1
                    fNtot[n] += 1
                leaf = nodes[i]
                self._note(recs, path, i, leaf, expanded, overflowed_before)
                overflowed_before = overflowed_before or over
                recs.append({"leaf": i, "path": path, "expanded": expanded,
                             "flags": (REC_OVERFLOW if over else 0) | (REC_LEAF_TURN if leaf.turn else 0)
                             | (REC_LEAF_TERMINAL if leaf.terminal else 0)})
                leaves.append(leaf.rec)
            st["path"], st["leaf"] = [], st["root"]          # as a compaction leaves them
            self.round.append(recs)
        return oracle.OracleBoards.from_records(leaves)

    def _note(self, recs, path, i, leaf, expanded, overflowed_before):
        met = self.met
        earlier_edges = {e for r in recs for e in r["path"][1:]}
        met["shared_edge_below_root"] += any(e in earlier_edges for e in path[1:])
        met["same_open_leaf"] += (not leaf.terminal) and any(r["leaf"] == i for r in recs)
        met["terminal_in_round"] += leaf.terminal
        met["descents_after_overflow"] += overflowed_before
        for r in recs:                # a pair expanded by an earlier descent of this round, whose other child this one enters
            kids = r["expanded"]
            if kids and len(kids) == 2 and r["leaf"] in kids:
                met["sibling_entered"] += i == (kids[0] if r["leaf"] == kids[1] else kids[1])

    # ---- the backup rule
    def backup_batch(self, values, probs):
        assert self.round is not None
        for g, st in enumerate(self._games):
            nodes = st["nodes"]
            K = self._round_k
            for j, rec in enumerate(self.round[g]):
                leaf = nodes[rec["leaf"]]
                row = g * K + j
                if leaf.terminal:
                    r = terminal_value(leaf.winner, leaf.turn)
                    self.ends["terminal"].add((leaf.winner, leaf.turn))
                else:
                    r = float(np.float32(values[row]))
                    if rec["flags"] & REC_OVERFLOW:
                        self.ends["overflowed"] += 1
                self._back_up(st, rec["path"], r)
                for i, a in rec["path"]:
                    st["fN"][i, a] -= 1
                    st["fNtot"][i] -= 1
                if not leaf.terminal and leaf.P is None:
                    self.ends["fresh"] += 1
                    leaf.P = {a: float(np.float32(probs[row][a])) for a in leaf.legal}
                    leaf.probs = np.array(probs[row], dtype=np.float32)
        self.k += self._round_k
        self.round = None

    # ---- what the device holds
    def in_flight(self):
        """The sum of every in-flight count of every game."""
        return sum(sum(st.get("fN", {}).values()) + sum(st.get("fNtot", {}).values()) for st in self._games)

    def raw_words(self):
        """Per game, per node: (the N words [36], the Ntot word) as the device stores them."""
        out = []
        for st in self._games:
            fN, fNtot = st.get("fN", {}), st.get("fNtot", {})
            out.append([([n.N[a] | (fN.get((i, a), 0) << FLIGHT_SHIFT) for a in range(36)],
                         n.Ntot | (fNtot.get(i, 0) << FLIGHT_SHIFT)) for i, n in enumerate(st["nodes"])])
        return out

    def records(self):
        """The round in flight as the device's path records: PATH_DTYPE[G, K], zero where the device writes nothing."""
        G, K = len(self.round), len(self.round[0]) if self.round else 0
        out = np.zeros((G, K), dtype=PATH_DTYPE)
        for g, recs in enumerate(self.round):
            for j, r in enumerate(recs):
                out[g, j]["leaf"], out[g, j]["depth"], out[g, j]["flags"] = r["leaf"], len(r["path"]), r["flags"]
                for d, (n, a) in enumerate(r["path"]):
                    out[g, j]["node"][d], out[g, j]["action"][d] = n, a
        return out


# ---------------------------------------------------------------- the root pool of the leaf-parallel tests
def root_pool(G, seed=POOL_SEED):
    """tests/value_tree_model.py's pool: the coverage floor of tests/test_tree_leaves_cpu.py holds on it as it is."""
    return value_tree_model.root_pool(G, seed)


# ---------------------------------------------------------------- the search that the tests run, on the model
LEAVES = (1, 2, 5, 8)
SEED, OFFSET = 5, 17


def first_rollouts(K):
    """Before the move: the single rollout, three rounds of K and a short round of 2 (a round of 1 twice at K = 1, 2)."""
    return 1 + 3 * K + 2


def second_rollouts(K):
    return 2 * K


def move_of(m):
    """The move of every game after the first rollouts: even games play the model's choice, odd games their least
    visited legal action (often a child that was never expanded: a fresh root); finished games do not move."""
    import tree_model
    act = np.full(len(m.games), 255, dtype=np.uint8)
    for g, st in enumerate(m.games):
        n = st["nodes"][st["root"]]
        if not n.terminal and n.legal:
            act[g] = tree_model.choose(n) if g % 2 == 0 else min(n.legal, key=lambda a: n.N[a])
    return act, (np.arange(len(m.games)) // 2 % 2).astype(np.uint8)


class RoundsModel(LeafParallelModel):
    """LeafParallelModel whose contemplate() goes through rounds at K = 1 as well, as a test that drives
    TreeSearch._round(1) by that schedule does."""

    def contemplate(self, r):
        if r and self.fresh:
            ValueTreeModel.rollout(self)
            r -= 1
            self.fresh = False
        K = self.leaves
        for k in [K] * (r // K) + [r % K] * (r % K > 0):
            self.round_of(k)


def model_stages(net, K, capacity, G, virtual_loss=1.0, probs_of=None):
    """The model of the G-game pool under the state dict `net`, searched as the tests search: first_rollouts(K), the
    move and the sync, second_rollouts(K) without and with a compaction in between.  Returns (stages, act, bits)."""
    import copy

    import tree_model
    arrays = root_pool(G)
    ob = oracle.boards_from_arrays(arrays["board"], arrays["moves"], arrays["n_moves"], arrays["qmask"], arrays["n_q"])
    m = RoundsModel(1, seed=SEED, board_offset=OFFSET, capacity=capacity, net=net, leaves=K, virtual_loss=virtual_loss)
    m.probs_of = probs_of
    m.reset(ob)
    m.contemplate(first_rollouts(K))
    stages = {"first": copy.deepcopy(m)}
    act, bits = move_of(m)
    after, _ = tree_model.after_move(m.root_positions(), act, bits)
    m.sync(after)
    stages["synced"] = copy.deepcopy(m)
    for compact in (False, True):
        c = copy.deepcopy(m)
        if compact:
            c.compact()
        c.contemplate(second_rollouts(K))
        stages["second", compact] = c
    return stages, act, bits

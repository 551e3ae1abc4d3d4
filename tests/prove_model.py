"""Proven interior nodes of include/qttt_tree_prove.h (qtttgym_amd.TreeSearch(leaf_eval="value", exact_from=M, prove=True))
on the float64 tree model: tests/exact_leaves_model.py's round with qttt_tree_prove after each round's backup, and what
qttt_tree_root_exact and TreeSearch.choose(exact=True) give.  Test infrastructure: tests/test_tree_prove_cpu.py checks the
model's own invariants and the coverage floor; tests/test_tree_prove_gpu.py compares the device's whole trees with it.

ProveRules is a mixin over ExactLeavesModel (ProveLeavesModel) and ExactGumbelModel (ProveGumbelModel); everything of
the round but the prove step is theirs.  A proven node joins st["solved"] (the device's solved bit and value bits) like an
enumerated leaf; st["proven"] is the set of nodes that the prove step solved, and st["kept"] = {node index: f32[36]} the
priors rows that the device leaves in the buffer when it clears a proven node's has-priors flag.  The values are kept in
integer sixteenths while they are derived, as on the device.  A plain helper module."""
import numpy as np

import exact_leaves_model as E
import solve_model
import tree_model
from exact_leaves_model import SOLVER, ExactGumbelModel, ExactLeavesModel, ExactRules  # noqa: F401
from leaf_parallel_model import terminal_value


class ProveRules:
    def __init__(self, *args, prove=True, **kwargs):
        super().__init__(*args, **kwargs)
        self.prove = bool(prove)
        assert not self.prove or self.exact_from is not None
        self.last_proved = None       # i32[G] of the last round: the nodes whose solved bit its prove step set
        self.met.update({"proved_below_root": 0, "proved_root": 0, "two_levels_in_one_walk": 0, "two_levels_stored": 0,
                         "proved_through_collapse": 0, "rederived": 0, "ended_on_proven": 0, "ended_on_proven_early": 0,
                         "records": 0, "rounds_before_first_end_on_proven": None, "rounds": 0})

    def reset(self, ob):
        super().reset(ob)
        for st in self._games:
            st["proven"], st["kept"] = set(), {}

    # ---- the rule of one node
    def sixteenths(self, st, x):
        """16 V(x) by the header's rule, or None where x is not provable."""
        nodes = st["nodes"]
        node = nodes[x]
        if node.terminal or not node.legal:
            return None
        best, collapse = None, False
        for a in node.legal:
            kids = node.children[a]
            if kids is None:
                return None
            vals = []
            for c in kids:
                if nodes[c].terminal:
                    vals.append(int(16 * terminal_value(nodes[c].winner, nodes[c].turn)))
                elif c in st["solved"]:
                    v16 = st["solved"][c] * 16
                    assert v16 == int(v16)
                    vals.append(int(v16))
                else:
                    return None
            if len(vals) == 2:
                assert (vals[0] + vals[1]) % 2 == 0, "the sum of a collapse's children is even"
                q16 = -((vals[0] + vals[1]) // 2)
                collapse = True
            else:
                q16 = -vals[0]
            best = q16 if best is None else max(best, q16)
        return best, collapse

    # ---- qttt_tree_prove on the records of the round that was just backed up
    def prove_round(self, recs):
        proved = np.zeros(len(self._games), dtype=np.int32)
        for g, st in enumerate(self._games):
            nodes = st["nodes"]
            for rec in recs[g]:
                path = rec["path"]
                new = stored = 0
                for d in range(len(path) - 1, -1, -1):
                    x = path[d][0]
                    r = self.sixteenths(st, x)
                    if r is None:
                        break
                    v16, collapse = r
                    first = x not in st["solved"]
                    assert first or st["solved"][x] * 16 == v16, "a node is re-derived with the same value"
                    st["solved"][x] = v16 / 16.0
                    st["proven"].add(x)
                    if d >= 1 and nodes[x].P is not None:
                        if nodes[x].probs is not None:
                            st["kept"][x] = nodes[x].probs
                        nodes[x].P = nodes[x].probs = None
                    stored += 1
                    new += first
                    proved[g] += first
                    self.met["rederived"] += not first
                    self.met["proved_through_collapse"] += first and collapse
                    self.met["proved_below_root" if d >= 1 else "proved_root"] += first
                self.met["two_levels_in_one_walk"] += new >= 2
                self.met["two_levels_stored"] += stored >= 2
        return proved

    def backup_batch(self, values, probs):
        recs = self.round
        if self.exact_from is not None:
            ended = 0
            for st, rs in zip(self._games, recs):
                for rec in rs:
                    i = rec["leaf"]
                    self.met["records"] += 1
                    if len(rec["path"]) >= 1 and i in st.get("proven", ()) and st["nodes"][i].P is None:
                        ended += 1
                        early = solve_model.played(st["nodes"][i].rec.tobytes()) < self.exact_from
                        self.met["ended_on_proven_early"] += early
            if ended and self.met["rounds_before_first_end_on_proven"] is None:
                self.met["rounds_before_first_end_on_proven"] = self.met["rounds"]
            self.met["ended_on_proven"] += ended
            self.met["rounds"] += 1
        super().backup_batch(values, probs)
        if self.exact_from is None or not self.prove:
            return
        for st in self._games:                # a row that the backup has just written again is no longer a kept one
            for x in [x for x in st["kept"] if st["nodes"][x].P is not None]:
                del st["kept"][x]
        self.last_proved = self.prove_round(recs)

    def compact(self):
        for st in self.games:
            keep = tree_model.reachable(st)
            if st["root"] == 0 and len(keep) == len(st["nodes"]):
                continue
            fwd = {old: new for new, old in enumerate(keep)}
            st["proven"] = {fwd[i] for i in st["proven"] if i in fwd}
            st["kept"] = {}               # a compaction leaves the rows of nodes without network priors unspecified
        super().compact()

    # ---- qttt_tree_root_exact, and TreeSearch.choose(exact=True)
    def root_exact(self):
        G = len(self.games)
        out = {"proven": np.zeros((G, 36), dtype=bool), "q_exact": np.full((G, 36), np.nan, dtype=np.float32),
               "root_solved": np.zeros(G, dtype=bool), "root_value_exact": np.full(G, np.nan, dtype=np.float32)}
        for g, st in enumerate(self.games):
            nodes, root = st["nodes"], st["root"]
            for a in nodes[root].legal:
                kids = nodes[root].children[a]
                if kids is None:
                    continue
                vals = [terminal_value(nodes[c].winner, nodes[c].turn) if nodes[c].terminal else st["solved"].get(c)
                        for c in kids]
                if any(v is None for v in vals):
                    continue
                out["proven"][g, a] = True
                out["q_exact"][g, a] = 0.0 - sum(vals) / len(vals)
            if root in st["solved"]:
                out["root_solved"][g] = True
                out["root_value_exact"][g] = st["solved"][root]
        return out

    def choose_exact(self, ordinary):
        """Where the root is solved: the lowest proven action whose q_exact is the root's value (at a root that a round
        proved, the lowest action attaining the maximal q_exact); `ordinary` where there is none."""
        ex = self.root_exact()
        out = np.array(ordinary, dtype=np.uint8).copy()
        for g in np.flatnonzero(ex["root_solved"]):
            best = np.flatnonzero(ex["proven"][g] & (ex["q_exact"][g] == ex["root_value_exact"][g]))
            if len(best):
                out[g] = int(best[0])
        return out

    def check_invariants(self):
        """Every solved node's value is a multiple of 1/16 in [-1, 1] and equals solve_model's of its position; a solved
        node below its root (reachable from it) has no priors; an enumerated one has no children and at least exact_from moves played; a
        proven one is not terminal and each of its legal actions leads to terminal or solved children.  Returns the number
        of solved nodes."""
        fresh = solve_model.Solver()
        n = 0
        for st in self.games:
            assert st["proven"] <= set(st["solved"])
            below = set(tree_model.reachable(st)) - {st["root"]}           # a root that was left keeps its priors
            for i, v in st["solved"].items():
                node = st["nodes"][i]
                assert v * 16 == int(v * 16) and -16 <= v * 16 <= 16
                assert v == fresh.solve(node.rec)["value"], (i, v)
                assert not node.terminal
                if i in below:
                    assert node.P is None and node.probs is None, (i, st["root"])
                if i in st["proven"]:
                    got = self.sixteenths(st, i)
                    assert got is not None and got[0] == v * 16
                else:
                    assert solve_model.played(node.rec.tobytes()) >= self.exact_from
                    if i in below:
                        assert all(c is None for c in node.children)
                n += 1
            for x in st["kept"]:
                assert x in st["proven"] and st["nodes"][x].P is None
        return n


class ProveLeavesModel(ProveRules, ExactLeavesModel):
    """ExactLeavesModel(..., exact_from=M, prove=True)."""


class ProveGumbelModel(ProveRules, ExactGumbelModel):
    """ExactGumbelModel(..., exact_from=M, prove=True)."""


# ---------------------------------------------------------------- the roots and the searches that the tests run
# 24 rollouts prove no root under exact_from = 8 at leaves = 1 (the model says so): 48 do, in every FLOOR_CASES search
ROLLOUTS, CAPACITY, OVERFLOW_CAPACITY, G_MAX = 48, E.CAPACITY, E.OVERFLOW_CAPACITY, E.G_MAX
SEED, OFFSET = E.SEED, E.OFFSET
# (network, leaves, exact_from, capacity) of the whole-tree comparisons.
# FLOOR_CASES meet the whole floor of tests/test_tree_prove_cpu.py.  They search with exact_from = 8: from a six-move root
# the seven-move children are interior nodes with a handful of actions, so children and then the root are proven within
# the budget, two levels in one walk.  With exact_from = 6 no node below a five- or six-move root can be proven at all
# (every node below the root has six moves played, is eligible and is solved as a leaf), and with exact_from = 7 a
# five-move root needs every six-move child proven, which no budget that fits the pool reaches: those cases prove roots
# (the six-move ones) and, at 7, single children, and are held to that.
FLOOR_CASES = [("zero", K, 8, CAPACITY) for K in (1, 4, 8)] + [("sharp", 4, 8, CAPACITY)]
WHOLE_CASES = (FLOOR_CASES
               + [("zero", 1, 7, CAPACITY), ("sharp", 4, 7, CAPACITY), ("sharp", 8, 7, CAPACITY), ("sharp", 4, 6, CAPACITY)]
               + [(net, 4, 7, CAPACITY) for net in ("zero", "greedy", "counting")]
               + [("zero", 4, 9, CAPACITY)]
               + [("zero", 4, 8, OVERFLOW_CAPACITY), ("sharp", 4, 7, OVERFLOW_CAPACITY), ("zero", 8, 6, OVERFLOW_CAPACITY)])


def roots(G):
    """Import arrays of G roots: tests/golden/solve_positions.npz's boards with five moves played, then its first six
    with six, cycled."""
    z = E.fixture()
    idx = np.concatenate([np.flatnonzero(z["played"] == 5), np.flatnonzero(z["played"] == 6)[:6]])
    idx = idx[np.arange(G) % len(idx)]
    return {k: z[k][idx] for k in E.ARRAYS}, idx


def schedule(r, K, fresh=True):
    """The rounds of TreeSearch.contemplate(r) under exact_from: one leaf first where nothing was contemplated since the
    last reset() or sync(), then rounds of K, then what is left."""
    first = [1] if r and fresh else []
    r -= len(first)
    return first + [K] * (r // K) + [r % K] * (r % K > 0)


def searched(net, K, M, capacity, G=G_MAX, probs_of=None, rollouts=ROLLOUTS, stages=False, prove=True):
    """The model of the G roots under the state dict `net` after `rollouts` rollouts with exact_from = M and the prove
    step; stages=True: ({first, synced, (second, compact)}, the moves, the bits) where every game with a proven node under
    its root moves onto one, and the second search is 2 K + 1 rollouts without and with a compaction."""
    import copy
    from leaf_parallel_model import move_of
    m = ProveLeavesModel(1, seed=SEED, board_offset=OFFSET, capacity=capacity, net=net, leaves=K, exact_from=M, prove=prove)
    m.probs_of = probs_of
    m.reset(E.boards_of(roots(G)[0]))
    m.contemplate(rollouts)
    if not stages:
        return m
    first = copy.deepcopy(m)
    act, bits = move_of(m)
    for g, st in enumerate(m.games):
        n = st["nodes"][st["root"]]
        hit = [a for a in n.legal if (n.children[a] or ()) and n.children[a][bits[g] if len(n.children[a]) == 2 else 0] in st["proven"]]
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

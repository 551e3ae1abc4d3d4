"""Forced playouts and policy target pruning of include/qttt_tree_forced.h (qtttgym_amd.TreeSearch(forced_playouts=k),
SelfPlay(prune_targets=True)) in Python floats, written from that header: the predicate, F(c), the root rule of a descent,
the pruned visit counts and the pruned pi row.  ForcedModel puts them on tests/leaf_parallel_model.py's LeafParallelModel,
which keeps the trees themselves.  Every rule is +, *, / and comparisons on IEEE doubles in the header's order, so the
device must reproduce it bit for bit.  d(c) is found here by looking at every d, where the device bisects.  Test
infrastructure: tests/test_forced_cpu.py checks it by hand and on whole searches of the model alone; tests/test_forced_gpu.py
runs the device against it.  The cases and the model's side of a whole search are here too.  A plain helper module."""
import math
from collections import Counter

import numpy as np

import explore_model
import gumbel_cases
import leaf_parallel_model as LP
import oracle
import selfplay_model
import tree_model
from leaf_parallel_model import REC_LEAF_TERMINAL, REC_LEAF_TURN, REC_OVERFLOW, LeafParallelModel, MAX_LEAVES
from tree_model import SELECT_BASE

SEED, OFFSET = gumbel_cases.SEED, gumbel_cases.OFFSET
K_FORCED, ROLLOUTS, NOISE = 2.0, 24, (0.25, 0.3)
OVERFLOW_CAPACITY = 12
GS, LEAVES = (1, 3, 130), (1, 3, 8)
# (G, leaves, noise, capacity or None = a pool that always fits)
CASES = tuple((G, K, noise, None) for G in GS for K in LEAVES for noise in (False, True)) + ((130, 3, True, OVERFLOW_CAPACITY),)


# ---------------------------------------------------------------- the rules of one root
def threshold(k, P, S):
    """(k * P) * S: two rounded products."""
    return (float(k) * float(P)) * float(int(S))


def is_forced(n, k, P, S):
    n = int(n)
    return n > 0 and float(n) * float(n) < threshold(k, P, S)


def F_of(k, P, S):
    """The smallest integer F >= 0 with F * F >= (k P) S; 0 for a product that is not a number, None for an infinite one."""
    t = threshold(k, P, S)
    if t != t or t <= 0.0:
        return 0
    if t == math.inf:
        return None
    F = max(0, int(math.sqrt(t)) - 2)
    while float(F) * float(F) < t:
        F += 1
    return F


def prior_of(node, a):
    return node.P[a] if node.P is not None else 0.0


def forced_actions(node, k, flight=None):
    """The forced legal actions of `node`; flight[a] = the visits in flight through action a."""
    if node.P is None or node.terminal:
        return []
    n = {a: node.N[a] + (flight[a] if flight else 0) for a in node.legal}
    S = sum(n.values())
    return [a for a in node.legal if is_forced(n[a], k, prior_of(node, a), S)]


def pruned_visits(node, k, c_puct):
    """N' as a list of 36 ints: the header's prune on the node's statistics as they stand."""
    out = [0] * 36
    if not node.legal:
        return out
    N, W = node.N, node.W
    star = max(node.legal, key=lambda a: N[a])                   # first maximum: ties to the lowest action
    S = sum(N[a] for a in node.legal)
    sq = math.sqrt(float(node.Ntot))

    def score(a, visits):
        q = W[a] / N[a] if N[a] else 0.0
        return q + c_puct * (prior_of(node, a) * sq / (1 + visits))

    best = score(star, N[star])
    for a in node.legal:
        out[a] = N[a]
        if a == star or N[a] == 0:
            continue
        F = F_of(k, prior_of(node, a), S)
        m = N[a] if F is None else min(N[a], F)
        d = next((x for x in range(m, 0, -1) if score(a, N[a] - x) < best), 0)
        left = N[a] - d
        out[a] = 0 if d > 0 and left <= 1 else left
    return out


def pruned_pi_row(node, k, c_puct, n_rollouts, alpha=1.0):
    return selfplay_model.pi_row(pruned_visits(node, k, c_puct), node.legal, n_rollouts, alpha)


# ---------------------------------------------------------------- the search
class ForcedModel(LeafParallelModel):
    """LeafParallelModel(n_sims, seed=, board_offset=, capacity=, net=, leaves=, virtual_loss=) with forced playouts at the
    root: select_batch_forced(K) / round_forced(k) beside the plain round, contemplate_forced(r) = TreeSearch's schedule.
    forced_taken counts the descents whose root action the rule chose."""

    def __init__(self, *args, forced_k=K_FORCED, **kwargs):
        super().__init__(*args, **kwargs)
        self.forced_k = float(forced_k)
        self.noise_idx = 0
        self.forced_taken = 0

    def reset(self, ob):
        super().reset(ob)
        self.noise_idx = 0

    path_records = LeafParallelModel.records

    def select_batch_forced(self, K):
        """qttt_tree_select_batch_forced: K descents per game; the G * K leaves as OracleBoards."""
        assert 1 <= K <= MAX_LEAVES and self.round is None
        vloss, k = self.virtual_loss, self.forced_k
        leaves, self.round, self._round_k = [], [], K
        for g, st in enumerate(self.games):
            nodes = st["nodes"]
            fN, fNtot = st["fN"], st["fNtot"] = Counter(), Counter()
            recs = []

            def score(node, i):
                key = lambda x: self._score_in_flight(node, x, fN[i, x], fNtot[i], vloss)      # noqa: E731
                if i == st["root"]:
                    forced = set(forced_actions(node, k, {a: fN[i, a] for a in node.legal}))
                    if forced:
                        self.forced_taken += 1
                        return lambda x: (x in forced, key(x) if x in forced else 0.0)
                return key

            for j in range(K):
                bits = oracle.hash64(self.seed, self.board_offset + g, SELECT_BASE + self.k + j) & 0xFFFFFFFF
                path, i, over, expanded = self._descend(st, bits, score)
                for n, a in path:
                    fN[n, a] += 1
                    fNtot[n] += 1
                leaf = nodes[i]
                recs.append({"leaf": i, "path": path, "expanded": expanded,
                             "flags": (REC_OVERFLOW if over else 0) | (REC_LEAF_TURN if leaf.turn else 0)
                             | (REC_LEAF_TERMINAL if leaf.terminal else 0)})
                leaves.append(leaf.rec)
            st["path"], st["leaf"] = [], st["root"]
            self.round.append(recs)
        return oracle.OracleBoards.from_records(leaves)

    def round_forced(self, k):
        leaves = self.select_batch_forced(k)
        self.backup_batch(self.playouts(leaves), self.priors(leaves))

    def contemplate_forced(self, r):
        """TreeSearch(forced_playouts=k).contemplate(r): the plain rollout where the roots may lack priors, then rounds of
        K through the forced select, also at K = 1."""
        if r and self.fresh:
            super(LeafParallelModel, self).rollout()
            r -= 1
            self.fresh = False
        K = self.leaves
        for k in [K] * (r // K) + [r % K] * (r % K > 0):
            self.round_forced(k)

    def contemplate(self, r):
        self.contemplate_forced(r)

    def rollout(self):
        self._queued += 1                                        # run as one contemplate() when the trees are looked at

    # ---- root noise: the model's own (numpy's log and cos), or the device's priors
    def add_root_noise(self, epsilon, alpha):
        games = self.games
        roots = [st["nodes"][st["root"]] for st in games]
        legal = [list(r.legal) if r.P is not None and not r.terminal else [] for r in roots]
        noise, applied, _ = explore_model.noise_rows(self.seed, self.board_offset, self.noise_idx, legal, alpha)
        for g, r in enumerate(roots):
            if applied[g]:
                p = np.zeros(36)
                for a in r.legal:
                    p[a] = r.P[a]
                row = explore_model.mix(p, noise[g], r.legal, epsilon)
                r.P = {a: float(row[a]) for a in r.legal}
                r.probs = row
        self.noise_idx += 1

    def adopt_priors(self, P, applied):
        """The device's noised priors P f64[G, 36] of the roots that were noised."""
        for g, st in enumerate(self.games):
            if applied[g]:
                n = st["nodes"][st["root"]]
                n.P = {a: float(P[g, a]) for a in n.legal}
                n.probs = P[g].astype(np.float32)
        self.noise_idx += 1

    # ---- what the roots say
    def roots(self):
        return [st["nodes"][st["root"]] for st in self.games]

    def forced_now(self):
        out = np.zeros((len(self.games), 36), dtype=bool)
        for g, r in enumerate(self.roots()):
            out[g, forced_actions(r, self.forced_k)] = True
        return out

    def pruned_now(self):
        return np.array([pruned_visits(r, self.forced_k, self.c_puct) for r in self.roots()], dtype=np.int32).reshape(-1, 36)


class PlainRoundsModel(LP.RoundsModel):
    """The plain in-flight search by the same schedule (rounds also at K = 1), with the model's noise."""
    noise_idx = 0
    add_root_noise = ForcedModel.add_root_noise


# ---------------------------------------------------------------- the whole search of a case
def capacity_of(case):
    G, K, noise, cap = case
    return cap if cap is not None else 2 + 4 * ROLLOUTS          # two searches, the first root, a fresh root


def new_model(case, net=None, forced_k=K_FORCED, cls=ForcedModel):
    G, K, noise, cap = case
    kw = {} if cls is not ForcedModel else {"forced_k": forced_k}
    model = cls(1, seed=SEED, board_offset=OFFSET, capacity=cap, net=net, leaves=K, **kw)
    model.reset(gumbel_cases.boards(gumbel_cases.positions(G)))
    return model


def search_once(model, noise, steps=None):
    """SelfPlay._search's schedule: one rollout, the noise, the other ROLLOUTS - 1."""
    model.contemplate(1)
    if noise:
        model.add_root_noise(*NOISE)
    model.contemplate(ROLLOUTS - 1)
    if steps is not None:
        steps.append([(list(r.N), list(r.W)) for r in (st["nodes"][st["root"]] for st in model.games)])


def move_of(model):
    return LP.move_of(model)


def model_search(case, net, forced_k=K_FORCED, cls=ForcedModel):
    """The whole search of a case on the model alone under the model's own network: a search from fresh roots, a move, a
    sync and a compaction, a second search on the reused subtrees.  model.first = the roots after the first search."""
    import copy
    G, K, noise, cap = case
    model = new_model(case, net, forced_k, cls)
    search_once(model, noise)
    model.first = copy.deepcopy(model.games)
    act, bits = move_of(model)
    after, _ = tree_model.after_move(model.root_positions(), act, bits)
    model.sync(after)
    model.compact()
    search_once(model, noise)
    return model

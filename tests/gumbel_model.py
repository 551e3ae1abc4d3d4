"""The Gumbel root of include/qttt_tree_gumbel.h (qtttgym_amd.TreeSearch(root_policy="gumbel")) in numpy float64, written
from that header: the visit sequence of sequential halving, the Gumbel draw and the considered actions of begin, completed
Q and sigma, the root rule of a descent, the final choice and the improved policy.  GumbelModel puts them on
tests/leaf_parallel_model.py's LeafParallelModel, which keeps the trees themselves.  Test infrastructure:
tests/test_gumbel_cpu.py checks it by hand and on synthetic statistics; tests/test_gumbel_gpu.py runs the device against it.

The device's log and exp sit an ulp or so from numpy's, so a GumbelModel can be handed the device's own record
(begin(records=...)): gumbel, prior, logits and root_value are then the device's bits and every later quantity is +, *, /
in the header's order, which the device must reproduce bit for bit.  Every root decision reports its MARGIN, the gap
between the two best scores of the set it was taken over, so that a test can tell a decision that rounding could flip.
A plain helper module."""
import numpy as np

import oracle
import selfplay_model
from leaf_parallel_model import (FLIGHT_SHIFT, REC_LEAF_TERMINAL, REC_LEAF_TURN, REC_OVERFLOW, LeafParallelModel,  # noqa: F401
                                 MAX_LEAVES)
from tree_model import SELECT_BASE

GUMBEL_BASE = 0xF0000000
GUMBEL_BYTES = 880
MAX_GUMBEL = 0x10000000 // 36
REC_DTYPE = np.dtype({"names": ["gumbel", "prior", "logits", "n0", "considered", "root_value", "m_eff"],
                      "formats": [("<f8", (36,)), ("<f8", (36,)), ("<f4", (36,)), ("<u4", (36,)), "<u8", "<f4", "<u4"],
                      "offsets": [0, 288, 576, 720, 864, 872, 876], "itemsize": GUMBEL_BYTES})
wave_sum = selfplay_model.wave_sum


# ---------------------------------------------------------------- the visit sequence
def visit_sequence(m, n):
    """The header's sequence for m considered actions and n simulations, as a list of n ints."""
    if m <= 1:
        return list(range(n))
    L = int(np.ceil(np.log2(m)))
    visits, out, c = [0] * m, [], m
    while len(out) < n:
        e = max(1, n // (L * c))
        for _ in range(e):
            out.extend(visits[:c])
            for i in range(c):
                visits[i] += 1
        c = max(2, c // 2)
    return out[:n]


def visit_table(n):
    return np.array([visit_sequence(m, n) for m in range(37)], dtype=np.int32)


def phases(seq):
    """The sequence cut where it decreases: within a phase the values never fall."""
    cuts = [0] + [i for i in range(1, len(seq)) if seq[i] < seq[i - 1]] + [len(seq)]
    return [seq[a:b] for a, b in zip(cuts, cuts[1:])]


# ---------------------------------------------------------------- begin
def uniforms(seed, board_id, move_idx, actions):
    """U53 of the Gumbel draws of the actions `actions` of board `board_id`."""
    h = np.array([oracle.hash64(int(seed), int(board_id), (GUMBEL_BASE + int(move_idx) * 36 + int(a)) & 0xFFFFFFFF)
                  for a in actions], dtype=np.uint64)
    return ((h >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def gumbel_of(u):
    return -np.log(-np.log(np.asarray(u, dtype=np.float64)))


def softmax_legal(x, legal):
    """exp(x - max) / the wave sum over the legal actions, 0 elsewhere; x f64[36]."""
    out = np.zeros(36, dtype=np.float64)
    if legal:
        e = np.zeros(36, dtype=np.float64)
        e[legal] = np.exp(x[legal] - x[legal].max())
        out[legal] = e[legal] / wave_sum(e)
    return out


def top_considered(gumbel, logits, legal, max_considered):
    """(the mask of the considered actions, m_eff): the m_eff legal actions of largest s0, ties to the lowest action."""
    m_eff = min(int(max_considered), len(legal))
    s0 = np.asarray(gumbel, dtype=np.float64) + np.asarray(logits, dtype=np.float32).astype(np.float64)
    order = sorted(legal, key=lambda a: (-s0[a], a))
    return sum(1 << a for a in order[:m_eff]), m_eff


# ---------------------------------------------------------------- completed Q, sigma, the decisions
def completed_q(N, W, legal, prior, root_value, c_visit, c_scale):
    """(q_hat f64[36], sigma f64[36], v_mix) by the header's formulas in the header's order; 0 at illegal actions."""
    n = np.zeros(36, dtype=np.int64)
    n[legal] = np.asarray(N, dtype=np.int64)[legal]
    W = np.asarray(W, dtype=np.float64)
    S, n_max = int(n.sum()), int(n.max()) if len(legal) else 0
    q = np.zeros(36, dtype=np.float64)
    seen = n > 0
    q[seen] = W[seen] / n[seen].astype(np.float64)
    root_value = np.float64(np.float32(root_value))
    if S:
        A = wave_sum(np.where(seen, np.asarray(prior, dtype=np.float64) * q, 0.0))
        B = wave_sum(np.where(seen, np.asarray(prior, dtype=np.float64), 0.0))
        with np.errstate(invalid="ignore", divide="ignore"):
            v_mix = (root_value + (np.float64(S) * A) / B) / (np.float64(1.0) + np.float64(S))
    else:
        v_mix = root_value
    q_hat = np.zeros(36, dtype=np.float64)
    q_hat[legal] = np.where(seen, q, v_mix)[legal]
    sigma = ((np.float64(c_visit) + np.float64(n_max)) * np.float64(c_scale)) * q_hat
    return q_hat, sigma, v_mix


def _argmax(actions, score):
    """(the first action of largest score, the gap to the runner-up; inf when there is none)."""
    best = max(actions, key=lambda a: score[a])                  # first maximum, as the wave's ties to the lowest lane
    rest = [score[a] for a in actions if a != best]
    return best, (float(score[best] - max(rest)) if rest else float("inf"))


def root_action(rec, N, F, W, legal, c, c_visit, c_scale):
    """The root rule of one descent: (action, margin), or (None, inf) where the ordinary rule holds.  N, F = the counts
    and the in-flight visits of the root's actions; c = the visit table's entry."""
    if rec["m_eff"] == 0:
        return None, float("inf")
    _, sigma, _ = completed_q(N, W, legal, rec["prior"], rec["root_value"], c_visit, c_scale)
    score = rec["s0"] + sigma
    cons = [a for a in legal if (rec["considered"] >> a) & 1]
    match = [a for a in cons if (int(N[a]) - int(rec["n0"][a])) + int(F[a]) == int(c)]
    return _argmax(match or cons, score)


def final(rec, N, W, legal, c_visit, c_scale):
    """(choose, pi f64[36], q_hat f64[36], margin) after the search: qttt_tree_gumbel_root's outputs."""
    q_hat, sigma, _ = completed_q(N, W, legal, rec["prior"], rec["root_value"], c_visit, c_scale)
    cons = [a for a in legal if (rec["considered"] >> a) & 1]
    choose, margin = 255, float("inf")
    if cons:
        visits = {a: int(N[a]) - int(rec["n0"][a]) for a in cons}
        most = max(visits.values())
        choose, margin = _argmax([a for a in cons if visits[a] == most], rec["s0"] + sigma)
    with np.errstate(invalid="ignore"):
        x = rec["logits"].astype(np.float64) + sigma
    return choose, softmax_legal(x, legal), q_hat, margin


def make_rec(gumbel, prior, logits, n0, considered, root_value, m_eff):
    logits = np.asarray(logits, dtype=np.float32)
    gumbel = np.asarray(gumbel, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        s0 = gumbel + logits.astype(np.float64)
    return {"gumbel": gumbel, "prior": np.asarray(prior, dtype=np.float64), "logits": logits, "s0": s0,
            "n0": np.asarray(n0, dtype=np.int64), "considered": int(considered), "root_value": np.float32(root_value),
            "m_eff": int(m_eff)}


# ---------------------------------------------------------------- the search
class GumbelModel(LeafParallelModel):
    """LeafParallelModel(n_sims, seed=, board_offset=, capacity=, net=, leaves=, virtual_loss=) with the Gumbel root:
    begin(n, records=None, evaluation=None), round_gumbel(k) / select_batch_gumbel(k) + backup_batch, contemplate_gumbel(n),
    finals().  margins: (game, margin) of every root decision taken so far."""

    def __init__(self, *args, max_considered=16, c_visit=50.0, c_scale=1.0, **kwargs):
        super().__init__(*args, **kwargs)
        self.max_considered, self.c_visit, self.c_scale = int(max_considered), float(c_visit), float(c_scale)
        self.move_idx, self.recs, self.table, self.sim_idx, self.margins = 0, None, None, 0, []

    def reset(self, ob):
        super().reset(ob)
        self.move_idx = 0

    def root_evaluation(self):
        """(value f32[G], masked logits f32[G, 36]) of the roots under the model's own (exact) network."""
        import torch
        from nn_reference64 import forward64
        v, logits, _ = forward64(self.net, torch.from_numpy(oracle.to_vector(self.root_positions())))
        return v.to(torch.float32).numpy(), logits.to(torch.float32).numpy()

    def begin(self, n, records=None, evaluation=None):
        """qttt_tree_gumbel_begin for a budget of n simulations.  records = the device's REC_DTYPE[G]: gumbel, prior,
        logits and root_value are taken from it (the considered set, m_eff and n0 are the model's own, to be compared).
        Otherwise evaluation = (value[G], logits[G, 36]) or the model's network, and numpy's log and exp."""
        if records is None:
            value, logits = evaluation if evaluation is not None else self.root_evaluation()
        self.recs = []
        for g, st in enumerate(self.games):
            root = st["nodes"][st["root"]]
            legal = [] if root.terminal else list(root.legal)
            if records is not None:
                gumbel, prior = records["gumbel"][g].copy(), records["prior"][g].copy()
                lg, rv = records["logits"][g].copy(), records["root_value"][g]
            else:
                lg, rv = np.asarray(logits[g], dtype=np.float32), np.float32(value[g])
                gumbel = np.zeros(36, dtype=np.float64)
                gumbel[legal] = gumbel_of(uniforms(self.seed, self.board_offset + g, self.move_idx, legal))
                prior = softmax_legal(lg.astype(np.float64), legal)
            considered, m_eff = top_considered(gumbel, lg, legal, self.max_considered)
            n0 = [root.N[a] if a in legal else 0 for a in range(36)]
            self.recs.append(make_rec(gumbel, prior, lg, n0, considered, rv, m_eff))
        self.table, self.sim_idx, self.n_sims_gumbel = visit_table(n), 0, int(n)
        self.move_idx += 1

    def records(self):
        raise NotImplementedError("use path_records() for the round's paths")

    path_records = LeafParallelModel.records

    def select_batch_gumbel(self, K):
        """qttt_tree_select_batch_gumbel: K descents per game; the G * K leaves as OracleBoards."""
        from collections import Counter
        assert 1 <= K <= MAX_LEAVES and self.round is None and self.sim_idx + K <= self.n_sims_gumbel
        vloss = self.virtual_loss
        leaves, self.round, self._round_k = [], [], K
        for g, st in enumerate(self.games):
            nodes, rec = st["nodes"], self.recs[g]
            fN, fNtot = st["fN"], st["fNtot"] = Counter(), Counter()
            recs = []
            for j in range(K):
                c = self.table[rec["m_eff"], self.sim_idx + j]

                def score(node, i, c=c):
                    if i == st["root"]:
                        a, margin = root_action(rec, node.N, [fN[i, x] for x in range(36)], node.W, node.legal, c,
                                                self.c_visit, self.c_scale)
                        if a is not None:
                            self.margins.append((g, margin))
                            return lambda x: 1 if x == a else 0
                    return lambda x: self._score_in_flight(node, x, fN[i, x], fNtot[i], vloss)

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
        self.sim_idx += K
        return oracle.OracleBoards.from_records(leaves)

    def round_gumbel(self, k):
        leaves = self.select_batch_gumbel(k)
        self.backup_batch(self.playouts(leaves), self.priors(leaves))

    def contemplate_gumbel(self, r, **begin):
        """TreeSearch(root_policy="gumbel").contemplate(r): the plain rollout where the roots have no priors, begin with
        the simulations that remain, rounds of K."""
        if r and self.fresh:
            super(LeafParallelModel, self).rollout()
            r -= 1
            self.fresh = False
        if r == 0:
            return
        self.begin(r, **begin)
        K = self.leaves
        for k in [K] * (r // K) + [r % K] * (r % K > 0):
            self.round_gumbel(k)

    def finals(self):
        """Per game (choose, pi, q_hat, margin) of the roots as they stand."""
        out = []
        for st, rec in zip(self.games, self.recs):
            root = st["nodes"][st["root"]]
            out.append(final(rec, root.N, root.W, list(root.legal), self.c_visit, self.c_scale))
        return out

    def device_records(self):
        """The records as the device stores them: REC_DTYPE[G]."""
        out = np.zeros(len(self.recs), dtype=REC_DTYPE)
        for g, r in enumerate(self.recs):
            for k in ("gumbel", "prior", "logits", "n0", "considered", "root_value", "m_eff"):
                out[k][g] = r[k]
        return out

    def min_margin(self):
        """Per game the smallest margin of a root decision so far (inf: none was taken)."""
        m = np.full(len(self.games), np.inf)
        for g, x in self.margins:
            m[g] = min(m[g], x)
        return m

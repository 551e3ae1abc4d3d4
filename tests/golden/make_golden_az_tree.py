#!/usr/bin/env python3
"""Generates tests/golden/az_tree_traces.npz from the UNMODIFIED reference AlphaZero class (`alphazero.py`: _rollout
:173-180, _backpropogate :182-190, _simulate :192-205, _expand_child :217-227, _prune :229-238, _step :240-274, _select
:276-284, _uct_select :287-292, get_action_probs :294-300, sample_action :302-303, choose :319-326, sync :328-348) with
the reference's own nn.Model, loaded through ref_shim.py, for each of the three exact networks of
tests/nn_reference64.py (EXACT_NETS: zero, greedy, sharp).  Build container only; the .npz is data (inputs + expected
outputs).

Only draws are replaced, each by the device's documented rule (k = the rollout index since the root was set):
  * `np.random.choice(children)` in _select (:283) at path depth d -> children[bit d of hash(seed, offset + g,
    2^31 + k)]; the qeval draws of an expansion (_select's and sync's _expand_child) return the lower square first, so
    that children are in qttt_expand's order;
  * `int(node.dist.sample())` in sample_action (:303) -> the rule of include/qttt_policy_rollout.h applied in f32 to the
    logits the reference's own Model.forward returned: ply p of simulation s of rollout k hashes step index
    k * n_sims * 16 + s * 16 + p, u = (h2 >> 8) * 2^-24, e_a = expf(logit_a - max) over the legal actions, each
    asserted to be exactly 0 or 1, and the action is the smallest legal a whose running sum exceeds f32(u) * f32(S).
    `alphazero.Categorical` is swapped for a subclass whose sample() is that rule; its probs are torch's own;
  * the qeval draws of _simulate's _step (:201) -> seq[bit], bit = h1 >> 31 of the same hash, and seq[1 - bit] for the
    resample loop's second draw; `np.random.choice(nodes)` in _simulate (:202) -> nodes[0], the same bit's branch.
`_select`, `_rollout`, `_simulate` and `sync` are wrapped on the instance to tell the draws apart; nothing is edited.

Roots as in make_golden_tree.py (built with their qstructs and assigned to `strat.root`): the empty board, positions
1-6 plies deep and a few finished games, each from a generator of its own so that any of them can be regenerated alone
(tests/test_az_reference_cpu.py does).  After each checkpoint of rollouts: root N, W, Q, P (float(p[a]); 0 while P is
None), Ntot, choose(), len(strat.nodes) and every root child's Ntot.  Then choose() is played with a fixed collapse
bit, sync() follows (len(strat.nodes) right after it is recorded), and more rollouts are recorded the same way.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ref_shim import load_reference, REFERENCE_ROOT  # noqa: E402
from make_golden_playout import NpStandIn, board_arrays  # noqa: E402
import oracle  # noqa: E402  (test infrastructure: the counter hash only)
from policy_playout_model import draw, exact_choice, exp_terms  # noqa: E402  (the sampling rule)
from nn_reference64 import EXACT_NETS  # noqa: E402

SIM_STRIDE = 16
SELECT_BASE = 1 << 31
NETS = ("zero", "greedy", "sharp")
# (seed, board_offset, n_sims, roots, finished games among them, checkpoints, rollouts after the sync)
GROUPS = ((11, 0, 4, 20, 3, (1, 2, 3, 10, 60), 40),
          (0xBEEF, (1 << 32) + 5000, 10, 4, 0, (1, 2, 3, 10, 60), 40))
RECORD_KEYS = ("N", "W", "Q", "P", "Ntot", "choose", "n_nodes", "child_Ntot")


class Source:
    """The draws of one search, keyed like the device's kernels."""

    def __init__(self):
        self.seed = self.board_id = self.step = self.k = 0
        self.in_select = self.expanding = self.in_move = False
        self.select_depth = self.bit = self.move_bit = self.draws_this_ply = 0

    # ---- numpy.random stand-in
    def choice(self, a, p=None):
        assert p is None
        if self.in_move:                                    # QTTTGame.make_move's pick of the new root (qttt.py:169)
            return a[self.move_bit] if len(a) == 2 else a[0]
        if self.in_select:                                  # _select's pick of a child (alphazero.py:283)
            d = self.select_depth
            self.select_depth += 1
            if len(a) == 1:
                return a[0]
            bits = oracle.hash64(self.seed, self.board_id, SELECT_BASE + self.k) & 0xFFFFFFFF
            return a[(bits >> d) & 1]
        self.step += 1                                      # _simulate's pick of a branch ends the ply
        return a[0]

    # ---- Categorical.sample stand-in (sample_action): include/qttt_policy_rollout.h in f32
    def sample(self, logits):
        lg = np.asarray(logits, dtype=np.float32)
        legal = sum(1 << a for a in range(36) if np.isfinite(lg[a]))
        self.bit, u = draw(oracle.hash64(self.seed, self.board_id, self.step))
        self.draws_this_ply = 0
        return exact_choice(legal, exp_terms(lg, legal), u)   # asserts that every e_a is exactly 0 or 1

    # ---- `random` stand-in inside qeval.py (qeval.py:35)
    class _Qeval:
        def __init__(self, outer):
            self.o = outer

        def choice(self, seq):
            assert len(seq) == 2
            o = self.o
            b = 0 if (o.in_select or o.expanding) else o.bit            # expansion: lower square first
            out = seq[b ^ (o.draws_this_ply & 1)]
            o.draws_this_ply += 1
            return out


def rule_categorical(base, src):
    """`base` (torch.distributions.Categorical) with sample() replaced by src.sample on the logits it was given."""
    import torch

    class RuleCategorical(base):
        def __init__(self, probs=None, logits=None, validate_args=None):
            self.given = logits.detach().clone()
            super().__init__(probs=probs, logits=logits, validate_args=validate_args)

        def sample(self, sample_shape=torch.Size()):
            return torch.tensor(src.sample(self.given.numpy()))
    return RuleCategorical


class Patched:
    """The reference's modules with their random sources swapped for `src`; everything is put back on exit."""

    def __init__(self, src, modules):
        self.src, self.modules, self.saved = src, modules, []

    def __enter__(self):
        import torch
        qtttgym, _ = load_reference()
        self.saved.append((qtttgym.qeval, "random", qtttgym.qeval.random))
        qtttgym.qeval.random = Source._Qeval(self.src)
        for mod in self.modules:
            if hasattr(mod, "np"):
                self.saved.append((mod, "np", mod.np))
                mod.np = NpStandIn(np, self.src)
            if hasattr(mod, "Categorical"):
                self.saved.append((mod, "Categorical", mod.Categorical))
                mod.Categorical = rule_categorical(mod.Categorical, self.src)
        self.threads = torch.get_num_threads()
        torch.set_num_threads(1)
        self.grad = torch.no_grad()
        self.grad.__enter__()
        return qtttgym

    def __exit__(self, *exc):
        import torch
        self.grad.__exit__(*exc)
        torch.set_num_threads(self.threads)
        for obj, name, val in reversed(self.saved):
            setattr(obj, name, val)


def reference_modules():
    load_reference()
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    import alphazero as ref_az                              # the reference's alphazero.py / nn.py, unmodified
    return ref_az


def root_depth(gi, pi):
    _, _, _, count, finished, _, _ = GROUPS[gi]
    if pi == 0:
        return 0
    return 9 if pi >= count - finished else 1 + (pi % 6)    # 9: play to the end, a finished game


def generate(net_name, gi, roots=None):
    """The records of network `net_name` on group gi's roots `roots` (default: all of them): (R, C), lists per root and
    per record."""
    ref_az = reference_modules()
    seed, offset, n_sims, count, _, checkpoints, after = GROUPS[gi]
    src = Source()
    R = {k: [] for k in ("group", "board", "moves", "n_moves", "qmask", "n_q", "sync_action", "sync_bit", "n_synced")}
    C = {k: [] for k in RECORD_KEYS}
    with Patched(src, [ref_az]) as qtttgym:
        GS = ref_az.AlphaZero.GameState
        sd = EXACT_NETS[net_name]()
        for pi in (range(count) if roots is None else roots):
            rng = random.Random(4242 + 1000 * gi + pi)
            # ---- the root: random play with this script's own collapse bits
            gs = GS([-1] * 9, [], True, None, False)
            game = qtttgym.Board(qtttgym.QEvalClassic())
            for _ in range(root_depth(gi, pi)):
                legal = [a for a in range(36) if gs.board[ref_az.ind2move(a)[0]] == -1
                         and gs.board[ref_az.ind2move(a)[1]] == -1]
                p1, p2 = gs.check_win()
                if not legal or p1 > 0 or p2 > 0:
                    break
                a = rng.choice(legal)
                b = rng.getrandbits(1)
                for board in (gs, game):
                    src.in_select, src.bit, src.draws_this_ply = False, b, 0
                    board.make_move(ref_az.ind2move(a))
            gs.turn = len(gs.moves) % 2 == 0                # AlphaZero.reset (alphazero.py:148)
            gs.update_actions()
            gs.winner, gs.terminal = None, False
            gs.update_winner()
            b_, mv, nm, qm, nq = board_arrays(gs)
            R["group"].append(gi); R["board"].append(b_); R["moves"].append(mv); R["n_moves"].append(nm)
            R["qmask"].append(qm); R["n_q"].append(nq)

            strat = ref_az.AlphaZero(rollouts=1, num_simulations=n_sims, filepath=os.path.join(REFERENCE_ROOT, "model.pt"))
            strat.model.load_state_dict(sd)                 # the reference's own nn.Model with the exact network
            strat.game = game
            strat.root = gs
            strat.nodes = {hash(gs): gs}
            inner_select, inner_rollout, inner_simulate, inner_sync = strat._select, strat._rollout, strat._simulate, strat.sync
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

            def sync(action, _inner=inner_sync):
                src.expanding, src.draws_this_ply = True, 0
                try:
                    return _inner(action)
                finally:
                    src.expanding = False
            strat._select, strat._rollout, strat._simulate, strat.sync = select, rollout, simulate, sync
            src.seed, src.board_id, src.k = seed, offset + pi, 0

            def record():
                n = strat.root
                N = [0] * 36; W = [0.0] * 36; Q = [0.0] * 36; P = [0.0] * 36
                kids = [[-1, -1] for _ in range(36)]
                for a in n.actions:
                    N[a], W[a], Q[a] = n.N[a], float(n.W[a]), float(n.Q[a])
                    if n.P is not None:
                        P[a] = n.P[a]
                    for c, child in enumerate(n.children[a] or ()):
                        kids[a][c] = child.Ntot
                C["N"].append(N); C["W"].append(W); C["Q"].append(Q); C["P"].append(P); C["Ntot"].append(n.Ntot)
                C["choose"].append(strat.choose() if n.actions else 255)
                C["n_nodes"].append(len(strat.nodes)); C["child_Ntot"].append(kids)

            done = 0
            for c in checkpoints:
                for _ in range(c - done):
                    strat._rollout()
                done = c
                record()
            # ---- play choose() with a fixed collapse bit, sync, more rollouts
            if gs.terminal or not gs.actions:
                R["sync_action"].append(255); R["sync_bit"].append(0); R["n_synced"].append(len(strat.nodes))
                for k in C:
                    C[k].append(C[k][-1])                   # no move: the after-sync record repeats the last one
                continue
            a = strat.choose()
            b = rng.getrandbits(1)
            src.in_select, src.bit, src.draws_this_ply = False, b, 0
            game.make_move(ref_az.ind2move(a))
            strat.sync(a)
            R["sync_action"].append(a); R["sync_bit"].append(b); R["n_synced"].append(len(strat.nodes))
            for _ in range(after):
                strat._rollout()
            record()
    return R, C


RECORD_DTYPES = {"N": np.int32, "W": np.float64, "Q": np.float64, "P": np.float64, "Ntot": np.int32, "choose": np.uint8,
                 "n_nodes": np.int32, "child_Ntot": np.int32}


def main():
    roots, per_net = None, []
    for name in NETS:
        R = {}
        C = {k: [] for k in RECORD_KEYS}
        for gi in range(len(GROUPS)):
            r, c = generate(name, gi)
            for k in r:
                R.setdefault(k, []).extend(r[k])
            for k in c:
                C[k].extend(c[k])
        shared = {k: R[k] for k in ("group", "board", "moves", "n_moves", "qmask", "n_q", "sync_bit")}
        assert roots is None or roots == shared             # the roots do not depend on the network
        roots = shared
        per_net.append((R, C))
        print("%s: %d roots, %d records" % (name, len(R["group"]), len(C["N"])), flush=True)
    out = {
        "nets": np.array(NETS),
        "g_seed": np.array([g[0] for g in GROUPS], dtype=np.uint64),
        "g_offset": np.array([g[1] for g in GROUPS], dtype=np.int64),
        "g_n_sims": np.array([g[2] for g in GROUPS], dtype=np.int32),
        "g_count": np.array([g[3] for g in GROUPS], dtype=np.int64),
        "g_after": np.array([g[6] for g in GROUPS], dtype=np.int32),
        "g_records": np.array([len(g[5]) + 1 for g in GROUPS], dtype=np.int32),
        "r_group": np.array(roots["group"], dtype=np.uint8),
        "r_board": np.array(roots["board"], dtype=np.int8), "r_moves": np.array(roots["moves"], dtype=np.uint8),
        "r_n_moves": np.array(roots["n_moves"], dtype=np.uint8), "r_qmask": np.array(roots["qmask"], dtype=np.uint16),
        "r_n_q": np.array(roots["n_q"], dtype=np.uint8), "r_sync_bit": np.array(roots["sync_bit"], dtype=np.uint8),
        "n_sync_action": np.array([r["sync_action"] for r, _ in per_net], dtype=np.uint8),
        "n_synced": np.array([r["n_synced"] for r, _ in per_net], dtype=np.int32),
    }
    for k in RECORD_KEYS:
        out["c_" + k] = np.array([c[k] for _, c in per_net], dtype=RECORD_DTYPES[k])
    for gi, g in enumerate(GROUPS):
        out["g%d_checkpoints" % gi] = np.array(g[5], dtype=np.int32)
    path = os.path.join(HERE, "az_tree_traces.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d networks x %d roots, %d records each, %d without a move, %d B"
          % (path, len(NETS), len(roots["group"]), out["c_N"].shape[1], int((out["n_sync_action"][0] == 255).sum()),
             os.path.getsize(path)))


CHECK = ("sharp", ((0, (0, 5, 18)), (1, (1,))))             # what --check regenerates: a network, (group, roots)


def check():
    """Regenerates a few roots of one network and compares them with the committed file (the fixture has not rotted:
    the reference, the exact network, the rule and the recording are still what wrote it)."""
    z = np.load(os.path.join(HERE, "az_tree_traces.npz"))
    name, parts = CHECK
    ni = [str(x) for x in z["nets"]].index(name)
    nr = [int(x) for x in z["g_records"]]
    for gi, roots in parts:
        R, C = generate(name, gi, roots)
        sel = np.nonzero(z["r_group"] == gi)[0]
        first = sum(int((z["r_group"] == h).sum()) * nr[h] for h in range(gi))
        for j, pi in enumerate(roots):
            r = sel[pi]
            for k in ("board", "moves", "n_moves", "qmask", "n_q", "sync_bit"):
                assert np.array_equal(np.array(R[k][j], dtype=z["r_" + k].dtype), z["r_" + k][r]), (k, gi, pi)
            assert R["sync_action"][j] == z["n_sync_action"][ni, r] and R["n_synced"][j] == z["n_synced"][ni, r], (gi, pi)
            for k in RECORD_KEYS:
                got = np.array(C[k][j * nr[gi]:(j + 1) * nr[gi]], dtype=RECORD_DTYPES[k])
                want = z["c_" + k][ni, first + pi * nr[gi]:first + (pi + 1) * nr[gi]]
                assert got.tobytes() == want.tobytes(), (k, gi, pi)
    print("az_tree_traces.npz: %s, %s regenerated and equal" % (name, parts))


if __name__ == "__main__":
    check() if sys.argv[1:] == ["--check"] else main()

"""A float64 Python restatement of the batched search tree of include/qttt_tree.h (qtttgym_amd.TreeSearch), built on the
C oracle's expand / rollout / counter hash.  Test infrastructure: tests/test_tree_cpu.py and
tests/test_tree_compact_cpu.py tie it to the reference's own MCTS class (tests/golden/tree_traces.npz); the GPU tests
run the device in lockstep with it (tests/tree_harness.py) and compare whole trees with it (tests/tree_layout.py).

Per game a plain list of nodes (the reference's node dict never merges two paths: its keys hold the full move
history).  The arithmetic is the reference's, in Python floats: score = Q + c_puct * (P * sqrt(Ntot) / (1 + N)),
W += r, Q = W / N.

TreeModel(capacity=c) also restates the header's overflow rule: an expansion (in select) or a fresh root (in sync) that
does not fit c nodes sets the game's sticky overflow flag and allocates nothing.  Node indices equal the device's: child
0 at `used`, child 1 at `used + 1`, a fresh root appended.

TreeModel(net=sd) searches as AlphaZero does (alphazero.py:192-205, 294-303) under an exact network of
tests/nn_reference64.py: the playouts are the host network playout of tests/policy_playout_model.py and the leaf's priors
the float64 forward's probabilities rounded to f32; tests/test_az_reference_cpu.py ties that to the reference's own
AlphaZero class (tests/golden/az_tree_traces.npz) and QTTTGame (tests/golden/selfplay_traces.npz).

compact() is qttt_tree_compact (the reference's _prune as MCTS.sync does it), a stable renumbering: per game the nodes
reachable from the root keep their relative order, the root becomes node 0, every child list is rewritten, and the
recorded path is cleared as by reset.  A game that is compact already (root 0, every node reachable) is left as it is,
its recorded path included.
"""
import math

import numpy as np

import oracle

SIM_STRIDE = 16
SELECT_BASE = 1 << 31


def _one(rec):
    return oracle.OracleBoards.from_records([rec])


def position_key(rec):
    """What identifies a position: Board.board, .moves, .qstructs (the fields the reference's hash and state hold)."""
    n, nq = int(rec["n_moves"]), int(rec["n_q"])
    return (bytes(np.asarray(rec["board"]).tobytes()), bytes(np.asarray(rec["moves"])[:n].tobytes()), n,
            bytes(np.asarray(rec["q"])[:nq].tobytes()), nq)


class Node:
    __slots__ = ("rec", "turn", "terminal", "winner", "legal", "Ntot", "N", "W", "P", "probs", "children")

    def __init__(self, rec, turn):
        self.rec = rec
        ob = _one(rec)
        w, t, legal, _ = oracle.node_info(ob)
        self.turn, self.terminal, self.winner = bool(turn), bool(t[0]), int(w[0])
        self.legal = [a for a in range(36) if (int(legal[0]) >> a) & 1]
        self.Ntot = 0
        self.N = [0] * 36
        self.W = [0.0] * 36
        self.P = None
        self.probs = None             # the network's f32[36] row behind P (None: no priors yet, or uniform ones)
        self.children = [None] * 36


class TreeModel:
    def __init__(self, n_sims, seed=0, board_offset=0, c_puct=1.0, capacity=None, net=None):
        self.n_sims, self.seed, self.board_offset, self.c_puct = int(n_sims), int(seed), int(board_offset), float(c_puct)
        self.net = net                                                    # None: MCTS; a state dict: AlphaZero
        self.capacity = None if capacity is None else int(capacity)       # None: the pool always fits
        self.games = []
        self.k = 0

    # ---- MCTS.reset
    def reset(self, ob):
        self.games = []
        for g in range(ob.n):
            rec = ob.b[g].copy()
            root = Node(rec, int(rec["n_moves"]) % 2 == 0)
            self.games.append({"nodes": [root], "root": 0, "path": [], "leaf": 0, "overflow": False})
        self.k = 0

    def _score(self, node, a):
        U = node.P[a] * math.sqrt(node.Ntot) / (1 + node.N[a])
        Q = node.W[a] / node.N[a] if node.N[a] else 0.0
        return Q + self.c_puct * U

    # ---- _select with _expand_child: the one descent, of select() and of leaf_parallel_model's select_batch()
    def _descend(self, st, bits, score):
        """One path of game `st` from its root under the collapse choices `bits`; score(node, i) = the key that ranks the
        legal actions of node i.  Returns (path, leaf, overflowed, expanded): the edges [(node, action)], the leaf's
        index, whether an expansion did not fit, and the children this descent expanded (None: none)."""
        nodes = st["nodes"]
        i = st["root"]
        path, overflowed, expanded = [], False, None
        while nodes[i].P is not None and not nodes[i].terminal and nodes[i].legal and len(path) < 10:
            node = nodes[i]
            a = max(node.legal, key=score(node, i))                          # first maximum, as Python's max
            if node.children[a] is None:
                nch, kids, _, _, _, _ = oracle.expand(_one(node.rec), np.array([a], dtype=np.uint8))
                if self.capacity is not None and len(nodes) + int(nch[0]) > self.capacity:
                    st["overflow"] = overflowed = True     # does not fit: the descent ends here, this edge is not on the path
                    break
                node.children[a] = []
                for c in range(int(nch[0])):
                    nodes.append(Node(kids[c].b[0].copy(), not node.turn))
                    node.children[a].append(len(nodes) - 1)
                expanded = node.children[a]
            kids = node.children[a]
            path.append((i, a))
            i = kids[(bits >> (len(path) - 1)) & 1] if len(kids) == 2 else kids[0]
        return path, i, overflowed, expanded

    def select(self):
        """Returns the leaves as OracleBoards."""
        leaves = []
        for g, st in enumerate(self.games):
            bits = oracle.hash64(self.seed, self.board_offset + g, SELECT_BASE + self.k) & 0xFFFFFFFF
            st["path"], st["leaf"], _, _ = self._descend(st, bits, lambda node, i: lambda x: self._score(node, x))
            leaves.append(st["nodes"][st["leaf"]].rec)
        return oracle.OracleBoards.from_records(leaves)

    def playouts(self, leaves):
        """result i8[G, n_sims] of the playouts of rollout k: uniform (oracle.rollout, the draws of qttt_rollout_many),
        or under the network (policy_playout_model.host_playout, the draws of qttt_rollout_policy)."""
        S = self.n_sims
        if self.net is not None:
            import policy_playout_model
            return policy_playout_model.host_playout(leaves, self.seed, self.board_offset, S, self.k * S * SIM_STRIDE,
                                                     net=self.net)[1]
        out = np.empty((leaves.n, S), dtype=np.int8)
        for s in range(S):
            out[:, s] = oracle.rollout(leaves, self.seed, self.k * S * SIM_STRIDE + s * SIM_STRIDE, self.board_offset)[0]
        return out

    # ---- _backpropogate: r = the leaf's value as the player to move there sees it
    @staticmethod
    def _back_up(st, path, r):
        for i, a in reversed(path):
            r = -r
            node = st["nodes"][i]
            node.W[a] += r
            node.N[a] += 1
            node.Ntot += 1

    # ---- _backpropogate and the leaf's priors
    def backup(self, result, probs=None):
        S = self.n_sims
        for g, st in enumerate(self.games):
            nodes = st["nodes"]
            leaf = nodes[st["leaf"]]
            r_tot = 0
            for s in range(S):
                r = int(result[g][s])
                r_tot += r if leaf.turn else -r
            self._back_up(st, st["path"], r_tot / S)
            if not leaf.terminal and leaf.P is None:
                if probs is None:
                    leaf.P = {a: 1 / len(leaf.legal) for a in leaf.legal}
                else:
                    leaf.P = {a: float(np.float32(probs[g][a])) for a in leaf.legal}
                    leaf.probs = np.array(probs[g], dtype=np.float32)
        self.k += 1

    def priors(self, leaves):
        """What backup takes as probs: None (uniform), or the network's f32[G, 36] rows of the leaves."""
        if self.net is None:
            return None
        import policy_playout_model
        return policy_playout_model.probs32(self.net, leaves)

    def rollout(self):
        leaves = self.select()
        self.backup(self.playouts(leaves), self.priors(leaves))

    # ---- MCTS.sync: ob = the games' positions after the move
    def sync(self, ob):
        for g, st in enumerate(self.games):
            nodes = st["nodes"]
            root = nodes[st["root"]]
            key = position_key(ob.b[g])
            if position_key(root.rec) == key:
                continue
            found = None
            for a in range(36):
                for c in (root.children[a] or ()):
                    if found is None and position_key(nodes[c].rec) == key:
                        found = c
            if found is None:
                if self.capacity is not None and len(nodes) + 1 > self.capacity:
                    st["overflow"] = True          # a fresh root does not fit: the root stays where it was
                    continue
                nodes.append(Node(ob.b[g].copy(), not root.turn))
                found = len(nodes) - 1
            st["root"] = found

    # ---- qttt_tree_compact
    def reachable_counts(self):
        return np.array([len(reachable(st)) for st in self.games], dtype=np.int32)

    def compact(self):
        for st in self.games:
            keep = reachable(st)
            if st["root"] == 0 and len(keep) == len(st["nodes"]):
                continue
            fwd = {old: new for new, old in enumerate(keep)}
            nodes = [st["nodes"][i] for i in keep]
            for n in nodes:
                n.children = [None if kids is None else [fwd[c] for c in kids] for kids in n.children]
            st["nodes"], st["root"], st["path"], st["leaf"] = nodes, 0, [], 0

    def root_positions(self):
        """The roots' records, as OracleBoards."""
        return oracle.OracleBoards.from_records([st["nodes"][st["root"]].rec for st in self.games])

    # ---- the roots' statistics, as qttt_tree_root
    def root_stats(self):
        G = len(self.games)
        o = {"N": np.zeros((G, 36), np.int32), "W": np.zeros((G, 36)), "Q": np.zeros((G, 36)), "P": np.zeros((G, 36)),
             "Ntot": np.zeros(G, np.int32), "choose": np.zeros(G, np.uint8), "nodes_used": np.zeros(G, np.int32),
             "overflow": np.zeros(G, bool)}
        for g, st in enumerate(self.games):
            n = st["nodes"][st["root"]]
            for a in n.legal:
                o["N"][g, a] = n.N[a]
                o["W"][g, a] = n.W[a]
                o["Q"][g, a] = n.W[a] / n.N[a] if n.N[a] else 0.0
                o["P"][g, a] = n.P[a] if n.P is not None else 0.0
            o["Ntot"][g] = n.Ntot
            o["choose"][g] = choose(n)
            o["nodes_used"][g] = len(st["nodes"])
            o["overflow"][g] = st["overflow"]
        return o

    def root_children_ntot(self):
        """i32[G, 36, 2]: Ntot of the root's children per action and child index, -1 where there is none."""
        out = np.full((len(self.games), 36, 2), -1, dtype=np.int32)
        for g, st in enumerate(self.games):
            for a, kids in enumerate(st["nodes"][st["root"]].children):
                for c, i in enumerate(kids or ()):
                    out[g, a, c] = st["nodes"][i].Ntot
        return out

    # ---- the whole trees, node by node in allocation order (= the device's node indices)
    def dump(self):
        """Per game: used, root, overflow, the last select's path [(node, action)] and leaf, and nodes = per node rec,
        turn, terminal, winner (-1 None, 0 False, 1 True), legal (the mask), Ntot, N[36], W[36], children (per action a
        list of 0, 1 or 2 node indices) and P: None (no priors), "uniform", or the network's f32[36] row."""
        out = []
        for st in self.games:
            nodes = []
            for n in st["nodes"]:
                P = None if n.P is None else ("uniform" if n.probs is None else n.probs)
                nodes.append({"rec": n.rec, "turn": n.turn, "terminal": n.terminal, "winner": n.winner,
                              "legal": sum(1 << a for a in n.legal), "Ntot": n.Ntot, "N": list(n.N), "W": list(n.W),
                              "children": [list(c or ()) for c in n.children], "P": P})
            out.append({"used": len(nodes), "root": st["root"], "overflow": st["overflow"], "path": list(st["path"]),
                        "leaf": st["leaf"], "nodes": nodes})
        return out


def reachable(st):
    """The indices of the nodes of one game that can be reached from its root, ascending."""
    nodes = st["nodes"]
    seen = {st["root"]}
    stack = [st["root"]]
    while stack:
        for kids in nodes[stack.pop()].children:
            for c in (kids or ()):
                assert c not in seen, "a node with two parents"
                seen.add(c)
                stack.append(c)
    return sorted(seen)


def game_view(d):
    """One game of TreeModel.dump() as plain values that compare with == (records and network priors as bytes): (used,
    root, path, leaf, nodes)."""
    return (d["used"], d["root"], d["path"], d["leaf"],
            [(n["rec"].tobytes(), n["turn"], n["terminal"], n["winner"], n["legal"], n["Ntot"], n["N"], n["W"],
              n["children"], n["P"].tobytes() if isinstance(n["P"], np.ndarray) else n["P"]) for n in d["nodes"]])


def choose(n):
    """MCTS.choose (mcts.py:308-315); 255 when there is no legal action."""
    if not n.legal:
        return 255
    return max(n.legal, key=lambda a: n.W[a] / n.N[a] if n.N[a] else -math.inf)


# ---------------------------------------------------------------- tests/golden/tree_traces.npz
def golden_groups(path):
    """Per group of the fixture: dict(seed, offset, n_sims, after, checkpoints, roots (OracleBoards), sync_action,
    sync_bit, records: dict of arrays [roots, len(checkpoints) + 1, ...] (the last record: after the sync))."""
    z = np.load(path)
    out = []
    rec0 = 0
    for gi in range(len(z["g_seed"])):
        sel = np.nonzero(z["r_group"] == gi)[0]
        nr = int(z["g_records"][gi])
        rows = {k[2:]: z[k][rec0:rec0 + len(sel) * nr].reshape((len(sel), nr) + z[k].shape[1:])
                for k in z.files if k.startswith("c_")}
        rec0 += len(sel) * nr
        out.append({"seed": int(z["g_seed"][gi]), "offset": int(z["g_offset"][gi]), "n_sims": int(z["g_n_sims"][gi]),
                    "after": int(z["g_after"][gi]), "checkpoints": [int(c) for c in z["g%d_checkpoints" % gi]],
                    "roots": oracle.boards_from_arrays(z["r_board"][sel], z["r_moves"][sel], z["r_n_moves"][sel],
                                                       z["r_qmask"][sel], z["r_n_q"][sel]),
                    "arrays": {k: z["r_" + k][sel] for k in ("board", "moves", "n_moves", "qmask", "n_q")},
                    "sync_action": z["r_sync_action"][sel], "sync_bit": z["r_sync_bit"][sel], "records": rows})
    return out


def az_golden_groups(path):
    """tests/golden/az_tree_traces.npz: a list of golden_groups-shaped dicts, one per (network, group), with "net" (the
    name in nn_reference64.EXACT_NETS) and "n_synced" (the reference's len(nodes) right after its sync) besides; the
    records hold P and child_Ntot too."""
    z = np.load(path)
    out = []
    for ni, name in enumerate(str(x) for x in z["nets"]):
        rec0 = 0
        for gi in range(len(z["g_seed"])):
            sel = np.nonzero(z["r_group"] == gi)[0]
            nr = int(z["g_records"][gi])
            rows = {k[2:]: z[k][ni, rec0:rec0 + len(sel) * nr].reshape((len(sel), nr) + z[k].shape[2:])
                    for k in z.files if k.startswith("c_")}
            rec0 += len(sel) * nr
            out.append({"net": name, "group": gi, "seed": int(z["g_seed"][gi]), "offset": int(z["g_offset"][gi]),
                        "n_sims": int(z["g_n_sims"][gi]), "after": int(z["g_after"][gi]),
                        "checkpoints": [int(c) for c in z["g%d_checkpoints" % gi]],
                        "roots": oracle.boards_from_arrays(z["r_board"][sel], z["r_moves"][sel], z["r_n_moves"][sel],
                                                           z["r_qmask"][sel], z["r_n_q"][sel]),
                        "arrays": {k: z["r_" + k][sel] for k in ("board", "moves", "n_moves", "qmask", "n_q")},
                        "sync_action": z["n_sync_action"][ni][sel], "sync_bit": z["r_sync_bit"][sel],
                        "n_synced": z["n_synced"][ni][sel], "records": rows})
    return out


def az_tight_capacity(grp):
    """The smallest pool in which a search of the group that compacts after its sync never overflows: the largest
    node count the reference has before the move (and one node for a fresh root) or at its last record."""
    n = grp["records"]["n_nodes"]
    return max(int(n[:, -2].max()) + 1, int(n[:, -1].max()))


def after_move(ob, action36, bits):
    """The positions after the sync move: board g plays ind2move(action36[g]) with collapse bit bits[g]; 255 = the game
    does not move."""
    new = ob.copy()
    acts = np.zeros((ob.n, 2), dtype=np.uint8)
    for g, a in enumerate(action36):
        acts[g] = oracle.ind2move(int(a)) if a != 255 else (0, 1)
    new.step(acts, np.asarray(bits, dtype=np.uint8))
    frozen = np.asarray(action36) == 255
    new.b[frozen] = ob.b[frozen]
    return new, acts

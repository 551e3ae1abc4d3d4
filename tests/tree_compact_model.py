"""TreeModel (tests/tree_model.py) with the compaction of include/qttt_tree.h (qttt_tree_compact, the reference's
_prune as MCTS.sync does it), and the comparison of a compacted device buffer with it.  Test infrastructure for
tests/test_tree_compact_cpu.py and tests/test_tree_compact_gpu.py; a plain helper module.

compact() is the stable renumbering in Python: per game the nodes reachable from the root keep their relative order,
the root becomes node 0, every child list is rewritten, and the recorded path is cleared as by reset.  A game that is
compact already (root 0, every node reachable) is left as it is, its recorded path included.
"""
import numpy as np

import tree_layout
import tree_model
from tree_layout import CHILD_PAIR, GAME_LEAF_TERMINAL, GAME_LEAF_TURN, GAME_OVERFLOW


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


class TreeCompactModel(tree_model.TreeModel):
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


def assert_live_tree_equals_model(buf, G, capacity, model, device="cuda:0"):
    """Every game header, every node < used, every slot and every network priors row of the tree buffer `buf` (host
    bytes) against the model.  Node records and priors at or beyond `used` are not looked at: after a compaction they
    are unspecified."""
    games, nodes, priors, _ = tree_layout.decode(buf, G, capacity)
    dump = model.dump()
    assert len(dump) == G
    used = np.array([d["used"] for d in dump], dtype=np.int32)
    assert (used <= capacity).all()
    for key, ref in (("used", used), ("root", [d["root"] for d in dump]), ("depth", [len(d["path"]) for d in dump]),
                     ("leaf", [d["leaf"] for d in dump])):
        assert np.array_equal(games[key], np.array(ref, dtype=np.int32)), (key, games[key], ref)
    gflags = np.array([(GAME_OVERFLOW if d["overflow"] else 0)
                       | (GAME_LEAF_TURN if d["nodes"][d["leaf"]]["turn"] else 0)
                       | (GAME_LEAF_TERMINAL if d["nodes"][d["leaf"]]["terminal"] else 0) for d in dump], dtype=np.uint32)
    assert np.array_equal(games["flags"], gflags), (games["flags"], gflags)
    for g, d in enumerate(dump):
        for k, (i, a) in enumerate(d["path"]):
            assert games["path_node"][g, k] == i and games["path_action"][g, k] == a, (g, k)
    live = np.arange(capacity)[None, :] < used[:, None]
    dev = nodes[live]
    flat = [n for d in dump for n in d["nodes"]]
    P, Q = tree_layout.pack_positions([n["rec"] for n in flat], device)
    flags = np.array([(0 if n["P"] is None else tree_layout.NODE_PRIORS)
                      | (tree_layout.NODE_UNIFORM if isinstance(n["P"], str) else 0)
                      | (tree_layout.NODE_TERMINAL if n["terminal"] else 0) | (tree_layout.NODE_TURN if n["turn"] else 0)
                      | ((n["winner"] + 1) << 8) for n in flat], dtype=np.uint32)
    for key, ref in (("P", P), ("Q", Q), ("legal", np.array([n["legal"] for n in flat], dtype=np.uint64)),
                     ("Ntot", np.array([n["Ntot"] for n in flat], dtype=np.uint32)), ("flags", flags)):
        assert np.array_equal(dev[key], ref), (key, np.nonzero(dev[key] != ref)[0][:8])
    N = np.array([n["N"] for n in flat], dtype=np.uint32).reshape(-1, 36)
    assert np.array_equal(dev["slots"]["N"], N), np.argwhere(dev["slots"]["N"] != N)[:8]
    W = np.array([n["W"] for n in flat], dtype=np.float64).reshape(-1, 36)
    assert np.array_equal(dev["slots"]["W"].view(np.int64), W.view(np.int64)), \
        np.argwhere(dev["slots"]["W"].view(np.int64) != W.view(np.int64))[:8]
    assert all(len(c) < 2 or c[1] == c[0] + 1 for n in flat for c in n["children"])
    child = np.array([[-1 if not c else (c[0] | (CHILD_PAIR if len(c) == 2 else 0)) for c in n["children"]] for n in flat],
                     dtype=np.int32).reshape(-1, 36)
    assert np.array_equal(dev["slots"]["child"], child), np.argwhere(dev["slots"]["child"] != child)[:8]
    network = np.array([isinstance(n["P"], np.ndarray) for n in flat], dtype=bool)
    if network.any():
        ref = np.stack([n["P"] for n in flat if isinstance(n["P"], np.ndarray)]).astype(np.float32)
        pri = priors[live][network]
        assert np.array_equal(pri.view(np.uint32), ref.view(np.uint32)), np.argwhere(pri.view(np.uint32) != ref.view(np.uint32))[:8]
    return network.sum()

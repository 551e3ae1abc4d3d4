"""CPU tests of the search trees' compaction (include/qttt_tree_compact.h, TreeSearch.compact): the Python model of the
stable renumbering (TreeModel.compact, tests/tree_model.py) against the node counts the reference's own MCTS leaves after its
sync has pruned (tests/golden/tree_traces.npz), a search that compacts after every move against one that never does,
the header, the binding table and the argument errors.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tree_traces.npz")
HEADER = os.path.join(ROOT, "include", "qttt_tree_compact.h")


def test_model_compact_leaves_the_node_count_the_reference_has_after_its_sync_pruned():
    """The fixture's last record is taken `after` rollouts after the reference's sync, whose _prune (mcts.py:222-231,
    330-337) has dropped every node outside the new root's subtree: len(strat.nodes) there is the kept subtree plus
    what those rollouts added.  The model reaches that count only with compact() after its sync."""
    import tree_model
    shrank = 0
    for grp in tree_model.golden_groups(GOLDEN):
        m = tree_model.TreeModel(grp["n_sims"], seed=grp["seed"], board_offset=grp["offset"])
        m.reset(grp["roots"])
        rec = grp["records"]
        done = 0
        for ci, c in enumerate(grp["checkpoints"]):
            for _ in range(c - done):
                m.rollout()
            done = c
            assert np.array_equal(m.root_stats()["nodes_used"], rec["n_nodes"][:, ci]), (ci, c)
        new, _ = tree_model.after_move(m.root_positions(), grp["sync_action"], grp["sync_bit"])
        m.sync(new)
        moved = grp["sync_action"] != 255
        before = m.root_stats()
        kept = m.reachable_counts()
        m.compact()
        st = m.root_stats()
        assert np.array_equal(st["nodes_used"], kept)
        assert (st["nodes_used"][moved] < before["nodes_used"][moved]).all()        # the old root, at the least
        assert np.array_equal(st["nodes_used"][~moved], before["nodes_used"][~moved])
        for k in ("N", "W", "Q", "P", "Ntot", "choose", "overflow"):
            assert np.array_equal(st[k], before[k]), k
        shrank += int(moved.sum())
        for _ in range(grp["after"]):
            m.rollout()
        st = m.root_stats()
        assert np.array_equal(st["nodes_used"], rec["n_nodes"][:, -1])
        for k in ("N", "W", "Q", "Ntot", "choose"):
            assert np.array_equal(st[k], rec[k][:, -1]), k
    assert shrank >= 40


def test_compact_is_a_stable_renumbering_that_keeps_the_tree_invariants():
    import tree_model
    grp = tree_model.golden_groups(GOLDEN)[0]
    m = tree_model.TreeModel(grp["n_sims"], seed=grp["seed"], board_offset=grp["offset"])
    m.reset(grp["roots"])
    for _ in range(40):
        m.rollout()
    # already compact (root 0, every node reachable): nothing changes, the recorded path included
    snap = [tree_model.game_view(d) for d in m.dump()]
    m.compact()
    assert snap == [tree_model.game_view(d) for d in m.dump()]
    new, _ = tree_model.after_move(m.root_positions(), grp["sync_action"], grp["sync_bit"])
    m.sync(new)
    old = [(tree_model.reachable(st), list(st["nodes"])) for st in m.games]
    stats = m.root_stats()
    m.compact()
    pairs = 0
    for g, st in enumerate(m.games):
        keep, nodes = old[g]
        assert [id(n) for n in st["nodes"]] == [id(nodes[i]) for i in keep], g       # the old order, nothing else
        assert st["root"] == 0 and (grp["sync_action"][g] == 255 or (st["path"] == [] and st["leaf"] == 0))
        for i, n in enumerate(st["nodes"]):
            for kids in n.children:
                for c in (kids or ()):
                    assert i < c < len(st["nodes"])                                  # a child lies above its parent
                if kids and len(kids) == 2:
                    assert kids[1] == kids[0] + 1                                    # a pair stays adjacent
                    pairs += 1
    assert pairs > 0
    after = m.root_stats()
    for k in ("N", "W", "Q", "P", "Ntot", "choose"):
        assert np.array_equal(stats[k], after[k]), k
    snap = [tree_model.game_view(d) for d in m.dump()]
    m.compact()                                                                      # twice: nothing left to do
    assert snap == [tree_model.game_view(d) for d in m.dump()]


def test_a_search_that_compacts_after_every_sync_goes_on_as_one_that_never_does():
    """Full games from the empty board, S = 4: model A never compacts, model B compacts after every sync.  Even games
    play choose(), odd games the least visited legal action (often a child never expanded: a fresh root, 1 node)."""
    import oracle
    import tree_model
    G, R, S = 6, 24, 4
    A = tree_model.TreeModel(S, seed=21, board_offset=3)
    B = tree_model.TreeModel(S, seed=21, board_offset=3)
    A.reset(oracle.OracleBoards(G))
    B.reset(oracle.OracleBoards(G))
    fresh = moves = 0
    while True:
        roots = [st["nodes"][st["root"]] for st in A.games]
        frozen = [n.terminal or not n.legal for n in roots]
        if all(frozen):
            break
        assert moves < 9
        for _ in range(R):
            A.rollout()
            B.rollout()
        sa, sb = A.root_stats(), B.root_stats()
        for k in ("N", "W", "Q", "P", "Ntot", "choose", "overflow"):
            assert np.array_equal(sa[k], sb[k]), (k, moves)
        act = np.full(G, 255, dtype=np.uint8)
        for g, n in enumerate(roots):
            if not frozen[g]:
                act[g] = sa["choose"][g] if g % 2 == 0 else min(n.legal, key=lambda a: n.N[a])
        new, _ = tree_model.after_move(A.root_positions(), act, ((np.arange(G) // 2 + moves) % 2).astype(np.uint8))
        A.sync(new)
        B.sync(new)
        B.compact()
        kept = A.reachable_counts()
        assert np.array_equal(B.root_stats()["nodes_used"], kept), moves
        fresh += int((kept == 1).sum())
        sa, sb = A.root_stats(), B.root_stats()
        for k in ("N", "W", "Q", "P", "Ntot", "choose", "overflow"):
            assert np.array_equal(sa[k], sb[k]), (k, moves)
        # the kept subtrees are the same trees, node for node, up to the renumbering
        for a, b in zip(A.games, B.games):
            keep = tree_model.reachable(a)
            fwd = {o: i for i, o in enumerate(keep)}
            for i, o in enumerate(keep):
                na, nb = a["nodes"][o], b["nodes"][i]
                assert (na.rec.tobytes(), na.Ntot, na.N, na.W, na.P) == (nb.rec.tobytes(), nb.Ntot, nb.N, nb.W, nb.P)
                assert [None if c is None else [fwd[x] for x in c] for c in na.children] == nb.children
        moves += 1
    assert moves >= 5 and fresh > 0
    assert max(len(st["nodes"]) for st in A.games) > 2 * R + 1            # A really did keep what B gave back


# ---------------------------------------------------------------- header, binding table, argument errors
def test_header_is_plain_c99_and_included_by_qttt_h():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_tree.h"') < src.index('#include "qttt_tree_compact.h"')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"],
                         input='#include "qttt.h"\nint main(void){int (*f)(void *, int64_t, int64_t, void *, void *) = '
                               'qttt_tree_compact;\nint64_t (*b)(int64_t, int64_t) = qttt_tree_compact_bytes;\n'
                               'return f == 0 || b == 0;}\n', capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_binding_header_exports_and_documents_agree():
    from qtttgym_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.TREE_COMPACT_SIGNATURES) == {"qttt_tree_compact", "qttt_tree_compact_bytes"}
    assert not names & (set(_native.SIGNATURES) | set(_native.TREE_SIGNATURES))
    lib = ctypes.CDLL(_native.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    assert _native.lib().qttt_abi_version() == _native.ABI_VERSION           # an additive entry: the ABI number stays
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in names:
        assert "`%s`" % n in integ, n
    for doc in ("include/qttt_tree.h", "qtttgym_amd/tree.py", "DESIGN.md", "INTEGRATION.md"):
        assert "no compaction" not in open(os.path.join(ROOT, doc)).read().lower(), doc


def test_compact_bytes():
    from qtttgym_amd import _native
    L = _native.lib()
    assert L.qttt_tree_compact_bytes(0, 1) == 0
    assert L.qttt_tree_compact_bytes(1, 1) == 4
    assert L.qttt_tree_compact_bytes(5, 96) == 4 * 5 * 96
    assert L.qttt_tree_compact_bytes(-1, 1) == -2
    assert L.qttt_tree_compact_bytes(1, 0) == -2
    assert L.qttt_tree_compact_bytes(1, (1 << 30) + 1) == -2
    assert L.qttt_tree_compact_bytes(1 << 40, 1 << 30) == -2


def test_return_codes_in_documented_order_without_device_work():
    from qtttgym_amd import _native
    L = _native.lib()
    fake = 0x1000                       # never dereferenced: every call below fails its checks first
    ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3
    # sizes first, even with null or misaligned pointers
    assert L.qttt_tree_compact(None, -1, 1, None, None) == ERR_SIZE
    assert L.qttt_tree_compact(None, 1, 0, None, None) == ERR_SIZE
    assert L.qttt_tree_compact(fake + 1, 1, (1 << 30) + 1, fake + 1, None) == ERR_SIZE
    # games == 0: nothing to do, no pointer looked at
    assert L.qttt_tree_compact(None, 0, 1, None, None) == 0
    assert L.qttt_tree_compact(fake + 1, 0, 8, fake + 1, None) == 0
    # then null pointers, before any alignment
    assert L.qttt_tree_compact(None, 1, 1, fake, None) == ERR_NULL
    assert L.qttt_tree_compact(fake, 1, 1, None, None) == ERR_NULL
    assert L.qttt_tree_compact(fake + 1, 1, 1, None, None) == ERR_NULL
    assert L.qttt_tree_compact(None, 1, 1, fake + 1, None) == ERR_NULL
    # then alignment: the tree 16 bytes, the scratch 4
    assert L.qttt_tree_compact(fake + 8, 1, 1, fake, None) == ERR_ACTION
    assert L.qttt_tree_compact(fake, 1, 1, fake + 2, None) == ERR_ACTION
    assert L.qttt_tree_compact(fake, 1, 1, fake + 1, None) == ERR_ACTION


def test_python_compact_needs_a_reset_and_keeps_or_replaces_the_bound():
    from qtttgym_amd import tree
    # a TreeSearch without a device: only the host-side bookkeeping is exercised
    t = tree.TreeSearch.__new__(tree.TreeSearch)
    t.num_games, t.capacity, t.num_simulations = 4, 21, 10
    t.rollout_idx, t._bound, t._scratch = 7, None, None
    with pytest.raises(RuntimeError, match="reset"):
        t.compact()
    calls = []
    t._scratch = object.__new__(type("Scratch", (), {"data_ptr": lambda self: 64}))
    t.tree = t._scratch
    t._call = lambda name, *args: calls.append((name,) + args)
    t.nodes_used = lambda: pytest.fail("update_bound=False must not read anything back")
    t._bound = 19
    t.compact(update_bound=False)
    assert calls == [("qttt_tree_compact", 64, 4, 21, 64)] and t._bound == 19 and t.rollout_idx == 7
    t.nodes_used = lambda: np.array([3, 9, 1, 5])
    t.compact()
    assert t._bound == 9 and t.rollout_idx == 7 and len(calls) == 2
    with pytest.raises(ValueError, match="capacity"):
        t.contemplate(7)                            # 9 + 2 * 7 > 21: the bound is the one read back
    t.num_games = 0
    t.compact()
    assert t._bound == 1

"""The network search and the self-play batch against the reference's own classes, without a device: the float64 tree
model (tests/tree_model.py, TreeModel(net=...), its playouts by tests/policy_playout_model.py) reproduces what the
reference's AlphaZero class recorded (tests/golden/az_tree_traces.npz), tests/selfplay_model.py what its play_game on
QTTTGame and the batch statements of self_play.py recorded (tests/golden/selfplay_traces.npz), and where the reference
is present a part of each fixture is regenerated and compared with the committed file.  tests/test_az_reference_gpu.py
holds the device to the same two files."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import selfplay_model
import tree_model
from nn_reference64 import EXACT_NETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
AZ_TREE = os.path.join(GOLDEN, "az_tree_traces.npz")
SELFPLAY = os.path.join(GOLDEN, "selfplay_traces.npz")
NETS = sorted(EXACT_NETS)
STATS = ("N", "W", "Q", "P", "Ntot", "choose")


def _assert_record(m, rec, ci, with_nodes):
    st = m.root_stats()
    for k in STATS:
        assert st[k].tobytes() == rec[k][:, ci].astype(st[k].dtype).tobytes(), (k, ci)        # W, Q, P bit for bit
    assert np.array_equal(m.root_children_ntot(), rec["child_Ntot"][:, ci]), ci
    if with_nodes:
        assert np.array_equal(st["nodes_used"], rec["n_nodes"][:, ci]), ci


def test_the_fixtures_hold_what_the_tests_rest_on():
    groups = tree_model.az_golden_groups(AZ_TREE)
    assert sorted({g["net"] for g in groups}) == NETS and len(groups) == 2 * len(NETS)
    assert max(g["offset"] for g in groups) > 1 << 32 and {g["n_sims"] for g in groups} == {4, 10}
    for g in groups:
        assert g["checkpoints"] == [1, 2, 3, 10, 60] and g["after"] == 40
        rec, moved = g["records"], g["sync_action"] != 255
        # the first rollout ends on the root itself and leaves its priors there, the second is the first to descend
        assert rec["P"][moved, 0].any(1).all() and not rec["Ntot"][:, 0].any() and (rec["Ntot"][moved, 1] == 1).all()
        assert not rec["P"][~moved].any()                                        # a finished root never gets any
        assert (rec["child_Ntot"][moved, -2].max((1, 2)) > 0).all()              # and a level below the root is recorded
        if g["group"] == 0:
            assert (~moved).sum() == 3 and g["roots"].n == 20
    P = {g["net"]: g["records"]["P"][:, -2] for g in groups if g["group"] == 0}
    uniform = np.unique(P["zero"][P["zero"] > 0])                                # f32(1 / k) widened, not the double 1 / k
    assert len(uniform) >= 3 and all(p != 1.0 / round(1.0 / p) for p in uniform)
    assert set(np.unique(P["greedy"])) == {0.0, 1.0}
    sharp = np.unique(P["sharp"][P["sharp"] > 0])
    assert 1.0 in sharp and len(sharp) >= 3                                      # m = 1 and several m > 1
    assert not any(float(np.float32(p)) != p for p in np.unique(np.concatenate(list(P.values()))))
    for fx in selfplay_model.golden_games(SELFPLAY):
        assert fx["n_sims"] == 10 and fx["G"] == 6 and len(set(fx["length"].tolist())) >= 2
    assert max(os.path.getsize(p) for p in (AZ_TREE, SELFPLAY)) < 200 * 1024


@pytest.mark.parametrize("net", NETS)
def test_tree_model_reproduces_the_reference_alphazero_class(net):
    """Every checkpoint of both groups: N, W, Q, P, Ntot, choose, the root children's Ntot and the node count; after the
    move, sync and compact() the reference's len(nodes), and the last record 40 rollouts later.  The compacting model
    has a pool that the search without compaction overflows."""
    shrank = 0
    for grp in (g for g in tree_model.az_golden_groups(AZ_TREE) if g["net"] == net):
        rec, last = grp["records"], len(grp["checkpoints"])
        capacity = tree_model.az_tight_capacity(grp)
        kw = dict(seed=grp["seed"], board_offset=grp["offset"], net=EXACT_NETS[net]())
        m = tree_model.TreeModel(grp["n_sims"], capacity=capacity, **kw)
        m.reset(grp["roots"])
        done = 0
        for ci, c in enumerate(grp["checkpoints"]):
            for _ in range(c - done):
                m.rollout()
            done = c
            _assert_record(m, rec, ci, True)
        moved = grp["sync_action"] != 255
        assert np.array_equal(m.root_stats()["choose"][moved], grp["sync_action"][moved])
        new, _ = tree_model.after_move(m.root_positions(), grp["sync_action"], grp["sync_bit"])
        m.sync(new)
        before = m.root_stats()["nodes_used"]
        m.compact()
        assert np.array_equal(m.root_stats()["nodes_used"], grp["n_synced"])
        shrank += int((grp["n_synced"] < before).sum())
        for _ in range(grp["after"]):
            m.rollout()
        _assert_record(m, rec, last, True)
        assert not m.root_stats()["overflow"].any()
        assert (before + rec["n_nodes"][:, last] - grp["n_synced"]).max() > capacity     # without compact(): overflow
    assert shrank >= 20


@pytest.mark.parametrize("net", NETS)
def test_selfplay_model_reproduces_the_reference_play_game(net):
    fx = [f for f in selfplay_model.golden_games(SELFPLAY) if f["net"] == net][0]
    G = fx["G"]
    out, env = selfplay_model.play(G, fx["n_rollouts"], fx["n_sims"], seed=fx["seed"], net=EXACT_NETS[net]())
    selfplay_model.assert_games_equal_reference(fx, out["action36"], out["length"], out["winner"])
    rows = [(g, t) for g in range(G) for t in range(int(fx["length"][g]))]
    for g, t in rows:
        if t < fx["length"][g] - 1:
            assert fx["bits"][g, t] == oracle.collapse_bit(fx["seed"], g, t)
    recs = oracle.OracleBoards.from_records([out["recs"][t][g] for g, t in rows])
    g_, t_ = (np.array(x) for x in zip(*rows))
    selfplay_model.assert_rows_equal_reference(fx, oracle.to_vector(recs).astype(np.float32), out["pi"][t_, g_],
                                               out["mask"][t_, g_], out["v"][t_, g_], out["done"][t_, g_])
    assert oracle.node_info(env)[1].all()


@pytest.mark.parametrize("script", ["make_golden_az_tree.py", "make_golden_selfplay.py"])
def test_a_part_of_each_fixture_regenerates_from_the_reference(script):
    """In a process of its own: loading the reference parks placeholder modules and the reference's top-level modules
    in sys.modules."""
    import ref_shim
    if not ref_shim.reference_available():
        pytest.skip("the reference is not on this machine")
    out = subprocess.run([sys.executable, os.path.join(GOLDEN, script), "--check"], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "regenerated and equal" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])

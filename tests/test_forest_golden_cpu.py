"""tests/golden/step_forest_traces.npz (make_golden_forest.py: the unmodified reference on forced forest shapes, every
closing move recorded once per collapse bit): that the committed file reaches what it was built to reach — re-root walks of
every length 0..8, computed with tests/forest_model.py — and the C oracle and oracle/py_env.PyEnv against every array of
it, as tests/test_oracle_golden.py holds them against step_traces.npz."""
import os
import subprocess
import sys

import numpy as np
import pytest

import forest_model as F
import test_oracle_golden as og

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def forest():
    with np.load(os.path.join(GOLDEN, "step_forest_traces.npz")) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def model(forest):
    return F.walks(forest)


def test_the_fixture_has_the_arrays_of_step_traces_and_is_no_larger(forest, golden):
    assert set(forest) == set(golden) | {"twin"}
    for k in golden:
        assert forest[k].dtype.kind == golden[k].dtype.kind and forest[k].shape[1:] == golden[k].shape[1:], k
        if k != "kind":
            assert forest[k].dtype == golden[k].dtype, k
    assert forest["twin"].shape == forest["kind"].shape and forest["twin"].dtype.kind == "i"
    assert set(forest["kind"].tolist()) >= {"path", "tree", "pairs", "noisy"}
    size = lambda name: os.path.getsize(os.path.join(GOLDEN, name))
    assert size("step_forest_traces.npz") <= size("step_traces.npz")


def test_the_model_counts_the_components_the_reference_recorded(forest, model):
    """The model is told actions and bits alone: that it follows the reference's games shows in n_q and, on every legal
    step, in the moves the reference appended."""
    assert np.array_equal(model["n_q"], forest["n_q"])
    played = np.diff(forest["n_moves"].astype(np.int64), axis=1, prepend=0) > 0
    assert np.array_equal(model["kind"] != F.NOOP, played)
    assert np.array_equal(model["kind"] == F.CYCLE, forest["consumed"] == 1)


def test_coverage_walks_of_every_length(forest, model):
    kind, walk = model["kind"], model["walk"]
    cyc = np.bincount(walk[kind == F.CYCLE], minlength=9)
    assert len(cyc) == 9 and (cyc >= 20).all(), cyc.tolist()
    uni = np.bincount(walk[kind == F.UNION], minlength=9)
    assert uni[4:].sum() >= 20 and uni[5:].sum() >= 1, uni.tolist()
    assert not walk[kind == F.GROW].any() and not walk[kind == F.NOOP].any()


def test_coverage_full_slots_and_nine_square_collapses(forest, model):
    assert int((forest["n_q"] == 4).sum()) >= 200
    assert int(((model["kind"] == F.CYCLE) & (model["size"] == 9)).sum()) >= 100


def test_every_closing_row_has_a_twin_that_differs_in_the_closing_bit_only(forest, model):
    twin = forest["twin"].astype(np.int64)
    E = len(twin)
    paired = np.nonzero(twin != np.arange(E))[0]
    assert len(paired) >= 2000 and np.array_equal(twin[twin], np.arange(E))
    assert (np.abs(twin[paired] - paired) == 1).all()                                    # neighbouring rows
    assert all(str(k) in ("path", "tree", "pairs", "noisy") for k in forest["kind"][paired])
    close = F.closing_steps(forest)
    for e in paired:
        o, t = twin[e], close[e]
        assert np.array_equal(forest["actions"][e], forest["actions"][o])
        assert int((forest["bits"][e] != forest["bits"][o]).sum()) == 1
        assert model["kind"][e, t] == F.CYCLE and not (model["kind"][e, :t] == F.CYCLE).any(), e
        assert forest["consumed"][e, t] == 1
        if t:
            for k in ("board", "moves", "n_moves", "qmask", "n_q"):
                assert np.array_equal(forest[k][e, t - 1], forest[k][o, t - 1]), (e, k)
        assert not np.array_equal(forest["board"][e, t], forest["board"][o, t]), e
        # the same squares collapse, other rounds land on them
        assert np.array_equal(forest["board"][e, t] >= 0, forest["board"][o, t] >= 0), e


def test_oracle_matches_the_forest_fixture_state_and_outputs(forest):
    og.check_oracle_state_and_outputs(forest)


def test_oracle_matches_the_forest_fixture_observation(forest):
    og.check_oracle_observation(forest)


def test_forest_fixture_reward_is_negative_zero_or_minus_one(forest):
    og.check_reward_is_negative_zero_or_minus_one(forest)


def test_pure_python_restatement_matches_the_forest_fixture(forest):
    og.check_pure_python_restatement(forest, every=1, every_full=1)


def test_the_fixture_regenerates_from_the_reference(forest, tmp_path):
    """In a process of its own: loading the reference parks placeholder modules in sys.modules."""
    import ref_shim
    if not ref_shim.reference_available():
        pytest.skip("the reference is not on this machine")
    out = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_forest.py"), "--out", str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    with np.load(str(tmp_path / "step_forest_traces.npz")) as d:
        again = {k: d[k] for k in d.files}
    assert set(again) == set(forest)
    for k in forest:
        assert again[k].dtype == forest[k].dtype and again[k].shape == forest[k].shape, k
        if k == "reward":
            assert np.array_equal(again[k].view(np.uint64), forest[k].view(np.uint64))
        else:
            assert np.array_equal(again[k], forest[k]), k

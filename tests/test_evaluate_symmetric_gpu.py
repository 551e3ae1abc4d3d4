"""The symmetry-averaged evaluation on the MI355X (include/qttt_nn_symmetric.h): evaluate(symmetries=S) against the
definition — the numpy model (tests/symmetric_eval_model.py) applied to the eight transformed(k).evaluate(net) results,
bit for bit with NaNs matched — for both precisions, four networks, six lists, the tile tails of both forms and every
subset of outputs; the per-board form; invariance under the group within the bound of two summation orders; and the
search and self-play built on it, tree bytes against a plain tree whose rounds the test drives by hand.  transformed is
pinned to mirrored reference games and evaluate to Model.forward by their own tests, so this pins the new kernel to the
reference transitively."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import symmetric_eval_model as M
import tree_harness as H
from nn_reference64 import (concat_envs, counting_state_dict, golden_state_dict, load_golden, random_play_env,
                            random_state_dict, zero_state_dict)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("value", "logits", "probs")
DTYPES = [torch.float32, torch.bfloat16]
NETS = ("fixture", "random", "zero", "counting")
EVERY = tuple(range(8))
LISTS = ((0,), (5,), (0, 2), (0, 6, 2, 4), EVERY, (3, 6, 0, 5, 7, 1, 4, 2))     # {0, 2} and {0, 2, 4, 6} are subgroups
SIZES_8 = (1, 7, 8, 9, 15, 16, 17, 257)          # n_sym = 8: a tile holds 8 boards in f32, 16 in bf16
SIZES_1 = (63, 64, 65, 127, 128, 129)            # n_sym = 1: 64 and 128


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert M.same_bits(got[k], want[k]), (what, k)


class Pool:
    """The positions (the fixture's 800, all-masked rows included, and 257 of random play with auto-reset), and per
    (network, precision) the eight images' evaluations: computed once, shared, never changed."""

    def __init__(self):
        from qtttgym_amd import VecEnv, symmetry
        g = load_golden()
        fx = VecEnv(len(g["value"]), device=DEV)
        fx.import_boards(g["moves"], g["n_moves"], g["board"], g["qmask"].astype("int16"), g["n_q"])
        self.env = concat_envs([fx, random_play_env(257, 31)])
        self.n = self.env.num_envs
        self.state0 = self.env.state.clone()
        self.actions = symmetry.tables()[1]
        self.images = [self.env.transformed(k) for k in range(8)]
        self.perm = torch.randperm(self.n, generator=torch.Generator().manual_seed(9))
        self.sds = {"fixture": golden_state_dict(g), "random": random_state_dict(2024), "zero": zero_state_dict(),
                    "counting": counting_state_dict()}
        self._nets, self._refs = {}, {}

    def net(self, name, dtype):
        from qtttgym_amd import PolicyValueNet
        if (name, dtype) not in self._nets:
            self._nets[name, dtype] = PolicyValueNet(self.sds[name], device=DEV, dtype=dtype)
        return self._nets[name, dtype]

    def ref(self, name, dtype):
        """images[k] = the numpy rows of transformed(k).evaluate(net): the composed route's evaluations."""
        if (name, dtype) not in self._refs:
            net = self.net(name, dtype)
            self._refs[name, dtype] = [_np(img.evaluate(net, rows=ALL)) for img in self.images]
        return self._refs[name, dtype]

    def rows(self, images, index):
        return [{k: v[index] for k, v in im.items()} for im in images]


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    assert int(torch.isnan(p.env.evaluate(p.net("zero", torch.float32), rows=("probs",))["probs"]).all(1).sum()) >= 47
    return p


# ---------------------------------------------------------------- fused against composed
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("name", NETS)
def test_fused_equals_the_model_on_the_composed_evaluations(pool, name, dtype):
    net, images = pool.net(name, dtype), pool.ref(name, dtype)
    for S in LISTS:
        got = _np(pool.env.evaluate(net, rows=ALL, symmetries=S))
        _assert_same(got, M.symmetric_mean(images, S, pool.actions), S)
    assert torch.equal(pool.env.state, pool.state0)           # the state buffer is not written


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("name", ("fixture", "random"))
def test_tile_tails_of_both_forms(pool, name, dtype):
    net, images = pool.net(name, dtype), pool.ref(name, dtype)
    for sizes, lists in ((SIZES_8, (EVERY, LISTS[-1])), (SIZES_1, ((0,), (5,)))):
        for n in sizes:
            idx = pool.perm[:n]
            sub = pool.env.take(idx.to(DEV))
            part = pool.rows(images, idx.numpy())
            for S in lists:
                got = _np(sub.evaluate(net, rows=ALL, symmetries=S))
                assert got["logits"].shape == (n, 36)
                _assert_same(got, M.symmetric_mean(part, S, pool.actions), (n, S))
    for n in (7, 9, 17, 65):                                  # the sizes between, for the lists of two and four
        idx = pool.perm[:n]
        sub, part = pool.env.take(idx.to(DEV)), pool.rows(images, idx.numpy())
        for S in ((4, 0), (1, 3, 0, 2)):
            _assert_same(_np(sub.evaluate(net, rows=ALL, symmetries=S)), M.symmetric_mean(part, S, pool.actions), (n, S))


def test_every_subset_of_outputs_and_out_reuse(pool):
    for dtype in DTYPES:
        net = pool.net("random", dtype)
        want = M.symmetric_mean(pool.ref("random", dtype), LISTS[-1], pool.actions)
        for r in (1, 2, 3):
            for rows in itertools.combinations(ALL, r):
                got = _np(pool.env.evaluate(net, rows=rows, symmetries=LISTS[-1]))
                _assert_same(got, {k: want[k] for k in rows}, rows)
        out = pool.env.evaluate(net, rows=("value", "probs"), symmetries=(0,))
        ptrs = {k: v.data_ptr() for k, v in out.items()}
        again = pool.env.evaluate(net, out=out, symmetries=LISTS[-1])
        assert again is out and {k: v.data_ptr() for k, v in out.items()} == ptrs
        _assert_same(_np(out), {k: want[k] for k in ("value", "probs")}, "out=")
    assert torch.equal(pool.env.state, pool.state0)


# ---------------------------------------------------------------- further checks on the entry
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_per_board_form_equals_transformed_evaluate_mapped_back(pool, dtype):
    net = pool.net("random", dtype)
    sym = torch.randint(0, 12, (pool.n,), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    sym[:4] = torch.tensor([0, 7, 8, 255], dtype=torch.uint8)
    assert int((sym > 7).sum()) > 100 and len(sym.unique()) >= 12
    composed = _np(pool.env.transformed(sym.to(DEV)).evaluate(net, rows=ALL))
    tau = np.asarray(pool.actions, dtype=np.int64)[np.where(sym.numpy() < 8, sym.numpy(), 0)]
    want = {"value": composed["value"], "logits": np.take_along_axis(composed["logits"], tau, 1),
            "probs": np.take_along_axis(composed["probs"], tau, 1)}
    _assert_same(want, M.per_board(pool.ref("random", dtype), sym.numpy(), pool.actions), "the model's per-board form")
    for n in (pool.n, 65, 1):
        idx = pool.perm[:n] if n < pool.n else torch.arange(pool.n)
        sub = pool.env.take(idx.to(DEV))
        got = _np(sub.evaluate(net, rows=ALL, symmetries=sym[idx].to(DEV).contiguous()))
        _assert_same(got, {k: v[idx.numpy()] for k, v in want.items()}, n)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_identity_list_is_plain_evaluate_and_the_zero_network_is_invariant(pool, dtype):
    for name in NETS:
        net = pool.net(name, dtype)
        plain = _np(pool.env.evaluate(net, rows=ALL))
        _assert_same(_np(pool.env.evaluate(net, rows=ALL, symmetries=(0,))), plain, name)
        ident = torch.full((pool.n,), 9, dtype=torch.uint8, device=DEV)
        _assert_same(_np(pool.env.evaluate(net, rows=ALL, symmetries=ident)), plain, name)
    net = pool.net("zero", dtype)
    _assert_same(_np(pool.env.evaluate(net, rows=ALL, symmetries=EVERY)), _np(pool.env.evaluate(net, rows=ALL)), "zero")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("name", ("fixture", "random"))
def test_the_full_group_mean_is_invariant_within_two_summation_orders(pool, name, dtype):
    """F = evaluate(symmetries = the full group in list order).  F of the transformed(k) boards, mapped back through
    tau_k, sums the same eight terms as F of the boards in another order: each pairwise sum of eight terms is off by at
    most 3 * 2^-24 * sum |x_j| before the scale by 1/8, so the two differ by at most 8 * 2^-24 * max_j |x_j| per element;
    infinite and NaN entries fall at the same places."""
    net = pool.net(name, dtype)
    base = _np(pool.env.evaluate(net, rows=ALL, symmetries=EVERY))
    terms = M.mapped_terms(pool.ref(name, dtype), EVERY, pool.actions)
    worst = 0.0
    for k in range(1, 8):
        other = _np(pool.images[k].evaluate(net, rows=ALL, symmetries=EVERY))
        for row in ALL:
            b = base[row]
            o = other[row] if row == "value" else M.map_back(other[row], pool.actions[k])
            fin = np.isfinite(b)
            assert np.array_equal(fin, np.isfinite(o)) and np.array_equal(np.isnan(b), np.isnan(o)), (k, row)
            assert np.array_equal(b[~fin & ~np.isnan(b)], o[~fin & ~np.isnan(o)]), (k, row)
            with np.errstate(invalid="ignore"):
                bound = 8.0 * 2.0 ** -24 * np.abs(terms[row].astype(np.float64)).max(0)
            d = np.abs(b[fin].astype(np.float64) - o[fin].astype(np.float64))
            ratio = d / np.maximum(bound[fin], 1e-300)
            worst = max(worst, float(ratio.max())) if d.size else worst
            assert (d <= bound[fin]).all(), (k, row, float(ratio.max()))
    print("%s %s: largest difference / bound = %.3f" % (name, dtype, worst))


# ---------------------------------------------------------------- search
CAP, ROLLOUTS = 64, 12


def _tree(env, net, leaves, **kw):
    """A TreeSearch over a sentinel-filled buffer (so that two trees' bytes compare whole), reset at env."""
    from qtttgym_amd import TreeSearch
    t = TreeSearch(env.num_envs, capacity=CAP, net=net, seed=5, board_offset=17, device=DEV, leaf_eval="value", leaves=leaves,
                   **kw)
    t.tree = torch.full((int(t._lib.qttt_tree_bytes(env.num_envs, CAP)) + H.TAIL,), H.SENTINEL, dtype=torch.uint8, device=DEV)
    t.reset(env)
    return t


def _round_by_hand(t, k, evaluate):
    """TreeSearch._round with the leaves' rows written by `evaluate(leaf env) -> {value, probs}` (numpy)."""
    b = t._round_buffers(k)
    G, cap, tree = t.num_games, t.capacity, t.tree.data_ptr()
    t._call("qttt_tree_select_batch", tree, G, cap, t.seed, t.rollout_idx, k, t.board_offset, t.c_puct, t.virtual_loss,
            b["paths"].data_ptr(), b["leaf"].state.data_ptr())
    rows = evaluate(b["leaf"])
    for key in ("value", "probs"):
        b["out"][key].copy_(torch.from_numpy(np.ascontiguousarray(rows[key])).to(DEV))
    t._call("qttt_tree_backup_batch", tree, G, cap, k, b["paths"].data_ptr(), b["out"]["value"].data_ptr(),
            b["out"]["probs"].data_ptr())
    t.rollout_idx += k


def _assert_same_search(a, b):
    """The trees of a search through the fused value rollout (a) and of one through rounds (b): every used node record and
    prior row byte for byte, and the headers' counts, roots and flags.  (The headers' recorded path is what differs between
    a rollout and a round, which leaves it as a compaction does: tests/test_tree_leaves_gpu.py.)"""
    import tree_layout
    G = a.num_games
    ga, na, pa, _ = tree_layout.decode(a.tree.cpu().numpy(), G, a.capacity)
    gb, nb, pb, _ = tree_layout.decode(b.tree.cpu().numpy(), G, b.capacity)
    assert np.array_equal(ga["used"], gb["used"]) and np.array_equal(ga["root"], gb["root"]) and ga["used"].max() >= ROLLOUTS
    assert np.array_equal(ga["flags"] & 1, gb["flags"] & 1)
    live = np.arange(a.capacity)[None, :] < ga["used"][:, None]
    assert np.array_equal(na[live].view(np.uint8), nb[live].view(np.uint8))
    assert np.array_equal(pa[live].view(np.uint8), pb[live].view(np.uint8))


def _schedule(leaves):
    """The rounds contemplate(ROLLOUTS) takes after a reset under eval_symmetries."""
    if leaves == 1:
        return [1] * ROLLOUTS
    r = ROLLOUTS - 1
    return [1] + [leaves] * (r // leaves) + [r % leaves] * (r % leaves > 0)


@pytest.fixture(scope="module")
def search_net():
    from qtttgym_amd import PolicyValueNet
    return PolicyValueNet(random_state_dict(2024), device=DEV, dtype=torch.float32)


@pytest.mark.parametrize("leaves", (1, 4))
@pytest.mark.parametrize("G", (3, 65))
def test_search_over_all_symmetries_equals_a_plain_tree_fed_the_composed_evaluation(search_net, G, leaves):
    from qtttgym_amd import symmetry
    actions = symmetry.tables()[1]
    env = H.env_from_arrays(H.random_positions(G, seed=G))

    def composed(leaf):
        images = [_np(leaf.transformed(k).evaluate(search_net, rows=("value", "probs"))) for k in range(8)]
        return M.symmetric_mean(images, EVERY, actions)

    fused = _tree(env, search_net, leaves, eval_symmetries="all")
    fused.contemplate(ROLLOUTS)
    plain = _tree(env, search_net, leaves)
    for k in _schedule(leaves):
        _round_by_hand(plain, k, composed)
    assert fused.rollout_idx == plain.rollout_idx == ROLLOUTS
    assert torch.equal(fused.tree, plain.tree)
    assert int(fused.root_stats()["Ntot"].max()) >= ROLLOUTS - 1


@pytest.mark.parametrize("leaves", (1, 4))
@pytest.mark.parametrize("G", (3, 65))
def test_search_under_the_identity_or_the_zero_network_is_the_plain_search(search_net, G, leaves):
    from qtttgym_amd import PolicyValueNet
    env = H.env_from_arrays(H.random_positions(G, seed=G))
    zero = PolicyValueNet(zero_state_dict(), device=DEV, dtype=torch.float32)
    for net, kw in ((search_net, dict(eval_symmetries=(0,))), (H.net(torch.bfloat16), dict(eval_symmetries=(0,))),
                    (zero, dict(eval_symmetries="all"))):
        plain, sym = _tree(env, net, leaves), _tree(env, net, leaves, **kw)
        plain.contemplate(ROLLOUTS)                          # leaves == 1: the fused value rollout
        sym.contemplate(ROLLOUTS)                            # every rollout a round, of one leaf where leaves == 1
        _assert_same_search(plain, sym)


# ---------------------------------------------------------------- self-play and the examples
def test_selfplay_under_the_identity_gives_the_plain_batch(search_net):
    from qtttgym_amd import SelfPlay
    from qtttgym_amd.selfplay import SelfPlayBatch
    kw = dict(n_rollouts=6, net=search_net, seed=3, device=DEV, leaf_eval="value", value_targets=(1.0, -1.0))
    plain = SelfPlay(3, **kw).play()
    sym = SelfPlay(3, eval_symmetries=(0,), **kw).play()
    for f in SelfPlayBatch._FIELDS:
        a, b = getattr(plain, f), getattr(sym, f)
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f
    assert int(plain.length.min()) >= 5
    every = SelfPlay(3, eval_symmetries="all", leaves=4, **kw).play()
    assert int(every.length.min()) >= 5 and bool(torch.isfinite(every.v).all())


def test_examples_run_with_the_new_flag(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "selfplay_train.py"), "--games", "64", "--rollouts", "8",
                          "--epochs", "2", "--runs", "1", "--leaf-eval", "value", "--value-targets", "1,-1",
                          "--eval-symmetries", "all", "--out", str(tmp_path / "model.pt")],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    assert re.search(r"run 0: (\d+) samples of 64 games", out.stdout), out.stdout
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tree_tournament.py"), "--p1", "azv:8", "--p2", "azv:8",
                          "--games", "64", "--eval-symmetries", "0,4"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    m = re.search(r"(\d+) games.*wins (\d+), losses (\d+), draws (\d+)", out.stdout)
    assert m and int(m.group(1)) == 64 and sum(map(int, m.groups()[1:])) == 64, out.stdout

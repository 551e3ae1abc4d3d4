"""The board's symmetries on the MI355X (include/qttt_symmetry.h): the image of a state is, in all 16 bytes, the state
the mirrored game reaches — games played in pairs, the group's laws on reached states, the reference's recorded games
(tests/golden/symmetry_traces.npz) — and SelfPlayBatch.augment against a torch restatement of it, field by field."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import symmetry_model as M
from tree_harness import DEV
from tree_harness import net as _net

from qtttgym_amd import SelfPlay, VecEnv, symmetry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 10
FIELDS = ("pi", "mask", "done", "v", "action36", "length", "winner", "actions")


def words(env_or_state, n):
    """The n boards' plane words, int64[2, n], of a VecEnv or of one state buffer."""
    st = env_or_state.state if isinstance(env_or_state, VecEnv) else env_or_state
    return st.view(torch.int64).view(2, -1)[:, :n]


def same(a, b):
    """Equal bit for bit (floats compared as their words: a NaN row equals itself)."""
    if a.dtype.is_floating_point:
        a, b = (x.contiguous().view({4: torch.int32, 8: torch.int64}[x.element_size()]) for x in (a, b))
    return a.shape == b.shape and bool(torch.equal(a, b))


# ---------------------------------------------------------------- games played in pairs
def _paired_games(n, ks, seed):
    """Env A plays sampled legal actions with explicit bits, env B the mirrored actions with the mapped bits, nine
    plies; after every ply A's image is compared with B."""
    cells, _ = symmetry.device_tables(DEV)
    cells = cells.to(torch.int64)
    k64 = ks.to(torch.int64)
    sigma = cells[k64]                                                            # [n, 9]
    tau = torch.tensor(M.ACTIONS, device=DEV)[k64]                                # [n, 36]
    A, B = VecEnv(n, device=DEV, seed=seed), VecEnv(n, device=DEV, seed=seed + 1)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    k_arg = int(ks[0]) if n > 0 and bool((ks == ks[0]).all()) and seed % 2 else ks     # the uniform form on odd seeds
    for ply in range(9):
        a = A.sample_actions().to(torch.int64)                                    # lo < hi, or (0, 0): a noop
        bits = torch.randint(0, 2, (n,), generator=gen, dtype=torch.uint8).to(DEV)
        land = torch.where(bits.bool(), a.max(1).values, a.min(1).values)
        ma = torch.gather(sigma, 1, a)
        mbits = (torch.gather(sigma, 1, land[:, None])[:, 0] == ma.max(1).values).to(torch.uint8)
        A.step_raw(a.to(torch.uint8).contiguous(), bits)
        B.step_raw(ma.to(torch.uint8).contiguous(), mbits)
        T = A.transformed(k_arg)
        assert torch.equal(words(T, n), words(B, n)), (n, ply, torch.nonzero((words(T, n) != words(B, n)).any(0))[:6].tolist())
        va, la = A.encode()
        vt, lt = T.encode()
        ref = torch.empty_like(va)
        idx = torch.cat([sigma, sigma + 9], 1)[:, :, None].expand(-1, -1, 10)
        ref.scatter_(1, idx, va)                                                  # ref[i, sigma(v)] = va[i, v], both halves
        assert torch.equal(vt, ref), (n, ply)
        la8 = la.to(torch.uint8)
        assert torch.equal(lt.to(torch.uint8), torch.zeros_like(la8).scatter_(1, tau, la8)), (n, ply)     # mask'[tau(a)] = mask[a]
        ia, it, ib = A.node_info(python_key=False), T.node_info(python_key=False), B.node_info(python_key=False)
        assert torch.equal(it["winner"], ia["winner"]) and torch.equal(it["terminal"], ia["terminal"]), (n, ply)
        assert torch.equal(it["state_key"], ib["state_key"]) and torch.equal(it["legal"], ib["legal"]), (n, ply)
    C = VecEnv.from_state(A.state.clone(), n)
    assert C.transformed(k_arg, out=C) is C and torch.equal(words(C, n), words(B, n))      # in place
    assert bool(A.node_info(python_key=False)["terminal"].all())
    return A, B


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1040])
def test_paired_games_with_a_symmetry_per_board(n):
    _paired_games(n, (torch.arange(n, device=DEV) % 8).to(torch.uint8), seed=2 * n)


@pytest.mark.parametrize("k", range(8))
def test_paired_games_with_one_symmetry_for_all(k):
    _paired_games(130, torch.full((130,), k, dtype=torch.uint8, device=DEV), seed=2 * k + 1)


def test_a_symmetry_past_seven_leaves_the_board_as_it_is():
    n = 70
    env = VecEnv(n, device=DEV, seed=3)
    env.step_random_many(5)
    ks = (torch.arange(n, device=DEV) % 16).to(torch.uint8)
    ks[3] = 255
    T = env.transformed(ks)
    keep = ks > 7
    good = ks.clamp(max=7)
    ref = env.transformed(good)
    assert torch.equal(words(T, n)[:, keep], words(env, n)[:, keep]) and torch.equal(words(T, n)[:, ~keep], words(ref, n)[:, ~keep])
    with pytest.raises(ValueError):
        env.transformed(8)
    with pytest.raises(ValueError):
        env.transformed(ks[:-1])
    with pytest.raises(ValueError):
        env.transformed(0, out=VecEnv(n + 1, device=DEV))


# ---------------------------------------------------------------- the group on reached states
@pytest.mark.parametrize("depth", [3, 5, 8])
def test_the_group_laws_hold_on_reached_states(depth):
    n = 1040
    env = VecEnv(n, device=DEV, seed=40 + depth)
    env.step_random_many(depth)
    assert torch.equal(words(env.transformed(0), n), words(env, n))
    images = [env.transformed(a) for a in range(8)]
    for a in range(8):
        assert torch.equal(words(images[a].transformed(symmetry.inverse(a)), n), words(env, n)), a
        for b in range(8):
            assert torch.equal(words(images[a].transformed(b), n), words(images[symmetry.compose(a, b)], n)), (a, b)
    assert len({tuple(words(x, n)[:, 7].tolist()) for x in images}) > 1           # the images differ


# ---------------------------------------------------------------- the reference's recorded games
def test_the_reference_positions_map_onto_the_recorded_mirrored_positions():
    with np.load(os.path.join(ROOT, "tests", "golden", "symmetry_traces.npz")) as z:
        tr = {k: z[k] for k in z.files}
    g, t = np.nonzero(np.arange(9)[None, :] < tr["n_plies"][:, None])
    n = len(g)
    assert n >= 4000
    env = VecEnv(n, device=DEV)
    env.import_boards(tr["a_moves"][g, t], tr["a_n_moves"][g, t], tr["a_board"][g, t], tr["a_qmask"][g, t].astype(np.int16),
                      tr["a_n_q"][g, t])
    ks = torch.as_tensor(tr["k"][g], device=DEV)
    ex = {k: v.cpu().numpy() for k, v in env.transformed(ks).export_boards().items()}
    order = 0
    for key in ("board", "moves", "n_moves", "qmask", "n_q"):
        want = tr["b_" + key][g, t]
        assert np.array_equal(ex[key], want.astype(ex[key].dtype)), (key, np.nonzero((ex[key] != want).reshape(n, -1).any(1))[0][:8])
    for i in range(n):
        order += [M.map_mask(int(m), int(tr["k"][g[i]])) for m in tr["a_qmask"][g[i], t[i]]] != ex["qmask"][i].tolist()
    assert order >= 20                                       # the list order that a permutation of the masks gets wrong
    # and the image is the imported mirrored position, bit for bit
    mirrored = VecEnv(n, device=DEV)
    mirrored.import_boards(tr["b_moves"][g, t], tr["b_n_moves"][g, t], tr["b_board"][g, t], tr["b_qmask"][g, t].astype(np.int16),
                           tr["b_n_q"][g, t])
    assert torch.equal(words(env.transformed(ks), n), words(mirrored, n))


# ---------------------------------------------------------------- augment
def _restated(batch, sym):
    """batch.augment(sym) with torch and the public calls: a dict of the fields and the states' words [10, 2, K G]."""
    G = batch.num_games
    live = torch.arange(ROWS, device=DEV)[:, None] < batch.length.to(torch.int64)[None, :]
    out = {k: [] for k in FIELDS + ("words",)}
    cells, _ = symmetry.device_tables(DEV)
    for k in sym:
        tau = torch.tensor(M.ACTIONS[k], device=DEV)
        pi, mask = torch.zeros_like(batch.pi), torch.zeros_like(batch.mask)
        pi[:, :, tau] = batch.pi                              # pi'[tau(a)] = pi[a]: a gather by tau's inverse
        mask[:, :, tau] = batch.mask
        out["pi"].append(pi)
        out["mask"].append(mask)
        out["action36"].append(torch.where(live, symmetry.transform_action36(batch.action36, k), torch.zeros_like(batch.action36)))
        a = batch.actions.to(torch.int64)
        out["actions"].append(torch.where(a < 9, cells[k].to(torch.int64)[a.clamp(max=8)], a).to(torch.uint8))
        for f in ("done", "v", "length", "winner"):
            out[f].append(getattr(batch, f))
        out["words"].append(torch.stack([words(batch.row_env(t).transformed(k), G) for t in range(ROWS)]))
    cat = {f: torch.cat(v, dim=0 if f in ("length", "winner", "actions") else 1) for f, v in out.items() if f != "words"}
    cat["words"] = torch.cat(out["words"], dim=2)
    return cat


def _assert_augmented(batch, sym, aug):
    G, K = batch.num_games, len(sym)
    assert aug.num_games == K * G and aug.states.shape == (ROWS, (K * G + 63) // 64 * 64 * 16)
    ref = _restated(batch, sym)
    for f in FIELDS:
        assert same(getattr(aug, f), ref[f]), f
    w = aug.states.view(torch.int64).view(ROWS, 2, -1)
    assert torch.equal(w[:, :, :K * G], ref["words"]) and not bool(w[:, :, K * G:].any())
    past = ~(torch.arange(ROWS, device=DEV)[:, None] < aug.length.to(torch.int64)[None, :])
    for f in ("pi", "mask", "done", "v", "action36"):
        assert not bool(getattr(aug, f)[past].any()), f
    assert not bool(w[:, :, :K * G].permute(0, 2, 1)[past].any())
    assert torch.equal(aug.length, batch.length.repeat(K)) and torch.equal(aug.winner, batch.winner.repeat(K))
    for s, k in enumerate(sym):
        if k == 0:                                           # the identity block is the input again
            for f in FIELDS:
                x = getattr(aug, f)
                blk = x[s * G:(s + 1) * G] if f in ("length", "winner", "actions") else x[:, s * G:(s + 1) * G]
                assert same(blk, getattr(batch, f)), f
            assert torch.equal(w[:, :, s * G:(s + 1) * G], batch.states.view(torch.int64).view(ROWS, 2, -1)[:, :, :G])


def _played(G, net=None):
    return SelfPlay(G, n_rollouts=8, num_simulations=2, net=net, seed=7, device=DEV).play()


@pytest.mark.parametrize("G", [1, 3, 65])
def test_augment_is_the_torch_restatement(G):
    batch = _played(G)
    before = {f: getattr(batch, f).clone() for f in FIELDS + ("states",)}
    aug = batch.augment()
    _assert_augmented(batch, tuple(range(8)), aug)
    assert all(same(getattr(batch, f), before[f]) for f in before)               # the input is read only
    # flat(): eight times the samples, block by block the original's, every pi row the same numbers in another order
    s0, pi0, mask0, v0, done0 = batch.flat()
    s8, pi8, mask8, v8, done8 = aug.flat()
    n = len(s0)
    assert n == int(batch.length.sum()) and len(s8) == 8 * n and s8.shape == (8 * n, 18, 10) and pi8.dtype == torch.float64
    assert same(s8[:n], s0) and same(pi8[:n], pi0) and torch.equal(mask8[:n], mask0)
    for s in range(8):
        blk = slice(s * n, (s + 1) * n)
        assert same(v8[blk], v0) and torch.equal(done8[blk], done0)
        assert same(pi8[blk].sort(-1).values, pi0.sort(-1).values) and same(pi8[blk].sort(-1).values.sum(-1), pi0.sort(-1).values.sum(-1))
        assert torch.equal(mask8[blk].sum(-1), mask0.sum(-1)) and not bool(pi8[blk][~mask8[blk]].any())
    # a choice of symmetries gives those blocks only
    for sym in ([0, 5], [3]):
        part = batch.augment(sym)
        _assert_augmented(batch, tuple(sym), part)
        for f in FIELDS:
            x, y = getattr(aug, f), getattr(part, f)
            per_game = f in ("length", "winner", "actions")
            blocks = [x[k * G:(k + 1) * G] if per_game else x[:, k * G:(k + 1) * G] for k in sym]
            assert same(y, torch.cat(blocks, dim=0 if per_game else 1)), (sym, f)


def test_augment_of_games_searched_with_the_network():
    batch = _played(65, _net(torch.float32))
    _assert_augmented(batch, tuple(range(8)), batch.augment())


# ---------------------------------------------------------------- the example
def test_selfplay_train_example_with_symmetries_trains_on_eight_times_the_samples(tmp_path):
    counts = []
    for flag in ([], ["--symmetries"]):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "selfplay_train.py"), "--games", "64",
                              "--rollouts", "8", "--sims", "2", "--epochs", "2", "--runs", "1", "--out",
                              str(tmp_path / "model.pt")] + flag, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        m = re.search(r"run 0: (\d+) samples of 64 games .*L: (\S+), J: (\S+)", out.stdout)
        assert m, out.stdout
        assert np.isfinite(float(m.group(2))) and np.isfinite(float(m.group(3))), out.stdout
        counts.append(int(m.group(1)))
    assert counts[1] == 8 * counts[0] and 64 * 6 <= counts[0] <= 64 * 10, counts

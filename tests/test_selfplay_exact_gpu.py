"""GPU tests of the exact targets of a self-play batch (include/qttt_selfplay_exact.h, SelfPlayBatch.exact_targets,
SelfPlay(exact_targets=M)), every comparison bit for bit: relabelled batches against tests/selfplay_exact_model.py's
float64 model and against VecEnv.solve; untouched bytes; the options; the rows override; guard bytes, a nullable `exact`
and idempotence on a staging batch of fixture boards; the stream; composition with exact leaves and the Gumbel root; the
trainer.  The golden network with value leaves and 8 rollouts per move.  tests/test_selfplay_exact_cpu.py asserts,
without a GPU, that the recorded plain batches and the fixture batch compared here are not vacuous."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import selfplay_exact_model as M  # noqa: E402
import test_selfplay_stream_gpu as S  # noqa: E402  (Watch, arrays, assert_ring: the stream tests' own drivers)
import tree_harness as H  # noqa: E402
from qtttgym_amd import ReplayBuffer, SelfPlay, Trainer, _native  # noqa: E402
from qtttgym_amd.selfplay import SelfPlayBatch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV, ROWS, SEED = H.DEV, M.ROWS, M.SEED
FIELDS = SelfPlayBatch._FIELDS
GUARD, SENTINEL = 256, 0xA5


def _sp(G, **kw):
    kw = dict(dict(n_rollouts=M.ROLLOUTS, net=S.golden_net(), seed=SEED, device=DEV, leaf_eval="value",
                   value_targets=(1.0, -1.0)), **kw)
    return SelfPlay(G, **kw)


def _np(batch):
    """Every field of a batch as numpy, floats as their bits."""
    out = {f: M.bits(getattr(batch, f).cpu().numpy()) for f in FIELDS}
    if hasattr(batch, "exact"):
        out["exact"] = batch.exact.cpu().numpy()
    return out


def _rows(batch):
    return [H.export(batch.row_env(t)) for t in range(ROWS)]


@functools.lru_cache(maxsize=None)
def _plain(G, **kw):
    """play(SEED) without exact targets: (the batch, its fields as numpy, its rows' boards), computed once and left alone."""
    b = _sp(G, **kw).play(SEED)
    return b, _np(b), _rows(b)


def _model(G, m, policy=True, rows=None, **kw):
    _, a, boards = _plain(G, **kw)
    L = a["length"] if rows is None else rows
    pi, v, exact = M.relabel(boards, L, a["done"], a["mask"], a["pi"].view(np.float64), a["v"].view(np.float32), m, policy)
    return M.bits(pi), M.bits(v), exact


def _assert_is_model(got, G, m, policy=True, rows=None, **kw):
    """pi, v and exact are the model's; every other field, and so every row that is not relabelled, is the plain batch's."""
    pi, v, exact = _model(G, m, policy, rows, **kw)
    _, a, _ = _plain(G, **kw)
    assert np.array_equal(got["exact"], exact)
    assert np.array_equal(got["v"], v), np.argwhere(got["v"] != v)[:6]
    assert np.array_equal(got["pi"], pi), np.argwhere(got["pi"] != pi)[:6]
    for f in FIELDS:
        if f not in ("pi", "v"):
            assert np.array_equal(got[f], a[f]), f
    keep = exact == 0
    assert np.array_equal(got["v"][keep], a["v"][keep]) and np.array_equal(got["pi"][keep], a["pi"][keep])
    return exact


# ---------------------------------------------------------------- the inputs are the recorded ones
@pytest.mark.parametrize("G", M.PLAIN_GAMES)
def test_the_device_plays_the_recorded_plain_batches(G):
    """What the CPU floor asserts of tests/golden/selfplay_exact_plain.npz it asserts of the batches relabelled here."""
    _, a, boards = _plain(G)
    ref = M.plain(G)
    for k in ("length", "done", "mask", "winner"):
        assert np.array_equal(a[k], ref[k]), k
    assert np.array_equal(a["pi"], M.bits(ref["pi"])) and np.array_equal(a["v"], M.bits(ref["v"]))
    for t in range(ROWS):
        for k in ("board", "n_moves", "moves"):
            assert np.array_equal(boards[t][k], ref["rows"][t][k]), (t, k)


# ---------------------------------------------------------------- the model: the tests that fail without the feature
@pytest.mark.parametrize("G,m", [(1, 7), (1, 8), (3, 6), (3, 7), (3, 8), (65, 7), (65, 8)])
def test_play_with_exact_targets_is_the_model_applied_to_the_plain_batch(G, m):
    sp = _sp(G, exact_targets=m)
    got = _np(sp.play(SEED))
    exact = _assert_is_model(got, G, m)
    assert int(got["exact"].sum()) == int(exact.sum()) == M.RELABELLED[G, m]      # the count the CPU floor pins


# ---------------------------------------------------------------- the solver
@pytest.mark.parametrize("G", [65, 130])
def test_relabelled_rows_hold_the_solver_s_value_and_its_argmax_set(G):
    b, a, _ = _plain(G)
    ex = _sp(G, exact_targets=6).play(SEED)
    live = (torch.arange(ROWS, device=DEV)[:, None] < b.length[None, :].long()) & (b.done == 0)
    seen = 0
    for t in range(ROWS):
        res = b.row_env(t).solve(min_ply=6)
        n = (res.nodes > 1) & res.solved                         # solved and no leaf
        want = live[t] & n & torch.isfinite(res.q).any(1)
        assert torch.equal(ex.exact[t].bool(), want), t
        hit = want.nonzero()[:, 0]
        seen += len(hit)
        assert torch.equal(ex.v[t][hit].view(torch.int32), res.value[hit].view(torch.int32))
        best = res.q[hit] == res.value[hit][:, None]
        assert torch.equal(ex.pi[t][hit] > 0, best)
        k = best.sum(1, keepdim=True).double()
        assert torch.equal(ex.pi[t][hit], torch.where(best, 1.0 / k, torch.zeros_like(k)))
        keep = (~want).nonzero()[:, 0]
        assert torch.equal(ex.v[t][keep].view(torch.int32), b.v[t][keep].view(torch.int32))
        assert torch.equal(ex.pi[t][keep].view(torch.int64), b.pi[t][keep].view(torch.int64))
    assert seen >= 2 * G
    assert np.array_equal(_np(b)["v"], a["v"])                   # the shared plain batch was left alone


# ---------------------------------------------------------------- options
def _count_calls(monkeypatch):
    L = _native.lib()
    inner, calls = L.qttt_selfplay_exact_targets, []

    def counted(*args):
        calls.append(args)
        return inner(*args)
    monkeypatch.setattr(L, "qttt_selfplay_exact_targets", counted)
    return calls


def test_options_value_only_min_ply_nine_and_none(monkeypatch):
    G = 65
    calls = _count_calls(monkeypatch)
    _, a, _ = _plain(G)
    got = _np(_sp(G, exact_targets=6, exact_policy=False).play(SEED))
    assert len(calls) == 1                                       # one launch per play()
    exact = _assert_is_model(got, G, 6, policy=False)
    assert exact.sum() > 0 and np.array_equal(got["pi"], a["pi"]) and not np.array_equal(got["v"], a["v"])
    nine = _np(_sp(G, exact_targets=9).play(SEED))
    assert len(calls) == 2 and not nine["exact"].any()
    for f in FIELDS:
        assert np.array_equal(nine[f], a[f]), f
    sp = _sp(G)
    b = sp.play(SEED)
    assert len(calls) == 2 and not hasattr(b, "exact") and sp.exact_targets is None
    for f in FIELDS:
        assert np.array_equal(_np(b)[f], a[f]), f
    sp.stream(ReplayBuffer(512, device=DEV), 3)
    assert len(calls) == 2                                       # nor does stream() call it
    ex = _sp(G, exact_targets=7)
    ex.stream(ReplayBuffer(512, device=DEV), 3)
    assert len(calls) == 5 and all(c[4] and not c[10] for c in calls[2:])      # one per ply, rows given, no exact buffer


# ---------------------------------------------------------------- the rows override
def test_a_rows_vector_selects_the_games_that_change():
    G = 65
    _, a, _ = _plain(G)
    b = _sp(G).play(SEED)
    rows = a["length"].copy()
    rows[1::2] = 0
    rows[4] = 7                                                  # and a game looked at below its length only
    exact = b.exact_targets(6, rows=torch.as_tensor(rows, device=DEV))
    got = _np(b)
    got["exact"] = exact.cpu().numpy()
    ex = _assert_is_model(got, G, 6, rows=rows)
    assert ex[:, 0::2].sum() > 0 and not ex[:, 1::2].any() and not ex[7:, 4].any()
    full = _model(G, 6)[2]
    assert full[:, 1::2].sum() > 0                               # the games left out do have rows to relabel
    with pytest.raises(ValueError):
        b.exact_targets(6, rows=torch.zeros(G, dtype=torch.int32, device=DEV))
    for bad in (5, 10, 6.5, True):
        with pytest.raises(ValueError):
            b.exact_targets(bad)


# ---------------------------------------------------------------- buffers: a staging batch of fixture boards
def _guarded(shape, dtype, fill=None):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    inner = raw[GUARD:GUARD + n].view(dtype).view(shape)
    if fill is not None:
        inner.copy_(torch.as_tensor(fill, device=DEV))
    return raw, inner


@pytest.mark.parametrize("m", [6, 7, 8])
def test_fixture_batch_guard_bytes_nullable_exact_and_idempotence(m):
    G = 65
    fb = M.fixture_batch(G)
    L = _native.lib()
    batch = SelfPlayBatch(G, torch.device(DEV), L.qttt_state_bytes(G))
    for t in range(ROWS):
        batch.states[t].copy_(H.env_from_arrays(fb["rows"][t]).state)
    for k in ("mask", "done", "length"):
        getattr(batch, k).copy_(torch.as_tensor(fb[k], device=DEV))
    raws = {}
    raws["pi"], batch.pi = _guarded((ROWS, G, 36), torch.float64, fb["pi"])
    raws["v"], batch.v = _guarded((ROWS, G), torch.float32, fb["v"])
    raws["exact"], exact = _guarded((ROWS, G), torch.uint8)
    before = {f: getattr(batch, f).clone() for f in ("states", "mask", "done", "length")}
    pi0, v0 = batch.pi.clone(), batch.v.clone()
    want_pi, want_v, want_exact = M.relabel(fb["rows"], fb["length"], fb["done"], fb["mask"], fb["pi"], fb["v"], m, True)

    def check():
        for raw in raws.values():
            assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all()
        for f, t in before.items():
            assert torch.equal(getattr(batch, f), t), f
        assert np.array_equal(M.bits(batch.pi.cpu().numpy()), M.bits(want_pi))
        assert np.array_equal(M.bits(batch.v.cpu().numpy()), M.bits(want_v))

    batch._exact_targets(m, True, None, exact)
    check()
    assert np.array_equal(exact.cpu().numpy(), want_exact) and want_exact.sum() > 0
    batch._exact_targets(m, True, None, exact)                   # idempotent: the same bytes
    check()
    assert np.array_equal(exact.cpu().numpy(), want_exact)
    batch.pi.copy_(pi0)
    batch.v.copy_(v0)
    batch._exact_targets(m, True, None, None)                    # exact = NULL
    check()
    assert np.array_equal(exact.cpu().numpy(), want_exact)       # and not written
    v = batch.v.cpu().numpy()
    assert not np.signbit(v[v == 0]).any()                       # never -0.0


def test_a_full_list_and_a_one_board_list_in_one_launch():
    """A hand-built staging batch of 65 games whose row 0 holds 65 distinct boards of tests/golden/solve_positions.npz
    with six or more moves played and a root that is no leaf; length 1, nothing done.  Record r = t * 65 + g, so records
    0..63 are one workgroup whose list is full (64 boards, 2 304 items) and record 64 opens a workgroup that lists one
    board.  Every row of row 0 holds the solver's value and the uniform policy over its argmax set, bit for bit."""
    G, m = 65, 6
    with np.load(os.path.join(M.GOLDEN, "solve_positions.npz")) as z:
        pick = np.flatnonzero((z["played"] >= m) & (z["best"] != 255))[:G]
        arrays = {k: z[k][pick] for k in M.ARRAYS}
    assert len(pick) == G
    env = H.env_from_arrays(arrays)
    planes = env.state.cpu().numpy().view(np.uint64).reshape(2, -1)[:, :G]
    assert len({(int(p), int(q)) for p, q in planes.T}) == G      # 65 distinct boards
    res = env.solve(min_ply=m)
    assert res.solved.all() and (res.nodes > 1).all()
    batch = SelfPlayBatch(G, torch.device(DEV), _native.lib().qttt_state_bytes(G))
    batch.states[0].copy_(env.state)
    batch.length.fill_(1)
    rng = np.random.default_rng(11)
    raws = {}
    raws["pi"], batch.pi = _guarded((ROWS, G, 36), torch.float64, rng.random((ROWS, G, 36)))
    raws["v"], batch.v = _guarded((ROWS, G), torch.float32, rng.choice(np.array([-1.0, 0.0, 1.0, 0.3125], np.float32), (ROWS, G)))
    raws["exact"], exact = _guarded((ROWS, G), torch.uint8)
    before = {f: getattr(batch, f).clone() for f in ("states", "mask", "done", "length")}
    pi0, v0 = batch.pi.clone(), batch.v.clone()
    batch._exact_targets(m, True, None, exact)
    for raw in raws.values():
        assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all()
    for f, t in before.items():
        assert torch.equal(getattr(batch, f), t), f
    assert (exact[0] == 1).all() and not exact[1:].any()
    assert torch.equal(batch.v[0].view(torch.int32), res.value.view(torch.int32))
    best = res.q == res.value[:, None]
    k = best.sum(1, keepdim=True).double()
    assert (k >= 1).all() and torch.equal(batch.pi[0], torch.where(best, 1.0 / k, torch.zeros_like(k)))
    assert torch.equal(batch.v[1:].view(torch.int32), v0[1:].view(torch.int32))
    assert torch.equal(batch.pi[1:].view(torch.int64), pi0[1:].view(torch.int64))


# ---------------------------------------------------------------- the stream
@pytest.mark.parametrize("G", [3, 65])
def test_the_stream_hands_the_ring_the_model_s_rows(G):
    plies, m = 12, 7
    plain, ex = _sp(G), _sp(G, exact_targets=m)
    wp, we = S.Watch(plain), S.Watch(ex)
    ring_p, ring_e = ReplayBuffer(4096, device=DEV), ReplayBuffer(4096, device=DEV)
    plain.stream(ring_p, plies, seed=SEED)
    stats = ex.stream(ring_e, plies, seed=SEED)
    relabelled = harvested = 0
    for (fin, hl, a), (fin2, hl2, a2) in zip(wp.plies, we.plies):
        assert np.array_equal(fin, fin2) and np.array_equal(hl, hl2)
        pi, v = a["pi"], a["v"]
        if fin.any():
            boards = [H.export(H.env_of_planes(a["states"][t, 0], a["states"][t, 1])) for t in range(ROWS)]
            pi, v, exact = M.relabel(boards, hl, a["done"], a["mask"], a["pi"].view(np.float64), a["v"].view(np.float32), m, True)
            assert not exact[:, fin == 0].any()                  # a game in progress: nothing relabelled in staging
            relabelled += int(exact.sum())
            harvested += int(fin.sum())
        assert np.array_equal(a2["pi"].view(np.uint64), M.bits(pi).view(np.uint64))
        assert np.array_equal(a2["v"].view(np.uint32), M.bits(v).view(np.uint32))
        for k in ("states", "mask", "done", "action36", "length", "winner"):
            assert np.array_equal(a2[k], a[k]), k
    assert harvested >= G and relabelled > 0
    S.assert_ring(ring_e, we, 4096)
    assert not torch.equal(ring_e.buffer, ring_p.buffer) and int(stats.samples) == int(ring_e.views()["written"].item())
    end_p, end_e = S.arrays(plain._stream["batch"]), S.arrays(ex._stream["batch"])
    for k in end_p:
        assert np.array_equal(end_p[k], end_e[k]), k             # the games still in progress: untouched


# ---------------------------------------------------------------- composition
@pytest.mark.parametrize("kw,m", [(dict(exact_from=7, leaves=4), 6),
                                  (dict(root_policy="gumbel", n_rollouts=9, leaves=4), 7)],
                         ids=["exact_from", "gumbel"])
def test_exact_targets_compose_with_exact_leaves_and_the_gumbel_root(kw, m):
    G = 3
    got = _np(_sp(G, exact_targets=m, **kw).play(SEED))
    exact = _assert_is_model(got, G, m, **kw)
    assert exact.sum() > 0


# ---------------------------------------------------------------- the trainer
def test_the_trainer_takes_a_relabelled_batch():
    import nn_reference64 as R
    b = _sp(65, exact_targets=6).play(SEED)
    s, pi, mask, v, done = b.flat()
    assert pi.dtype == torch.float64 and v.dtype == torch.float32 and int(b.exact.sum()) > 0
    tr = Trainer(R.golden_state_dict(R.load_golden()), device=DEV)
    L, J = tr.step(s, pi, mask, v, done)
    assert torch.isfinite(L).all() and torch.isfinite(J).all() and L.numel() == v.numel()

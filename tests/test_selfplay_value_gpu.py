"""GPU tests of the search-value targets (include/qttt_selfplay_value.h, SelfPlay(value_mix= / td_lambda=)), every
comparison with tests/selfplay_value_model.py bit for bit: the target kernel on hand-filled batches (no search), the record
kernel against root_stats() and, for the sign, against Reanalyser's torch formula, and play() / stream() end to end on the
golden network with value leaves and 8 rollouts per move."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import selfplay_value_model as M  # noqa: E402
import test_selfplay_stream_gpu as S  # noqa: E402  (Watch, arrays, assert_ring, golden_net: the stream tests' own drivers)
import tree_harness as H  # noqa: E402
from qtttgym_amd import ReplayBuffer, SelfPlay, _native  # noqa: E402
from qtttgym_amd._host import LibCaller  # noqa: E402
from qtttgym_amd.selfplay import SelfPlayBatch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV, ROWS, SEED = H.DEV, M.ROWS, 2026
FIELDS = SelfPlayBatch._FIELDS
GUARD, SENTINEL = 256, 0xA5


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    inner = raw[GUARD:GUARD + n].view(dtype).view(shape)
    inner.copy_(torch.as_tensor(fill, device=DEV))
    return raw, inner


def _guards_hold(*raws):
    return all(bool((raw[:GUARD] == SENTINEL).all()) and bool((raw[-GUARD:] == SENTINEL).all()) for raw in raws)


def _dev(x, dtype=None):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def _f32bits(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------- the target kernel on hand-filled batches
def _hand(G, b):
    batch = SelfPlayBatch(G, torch.device(DEV), _native.lib().qttt_state_bytes(G))
    batch.length.copy_(_dev(b["length"]))
    batch.done.copy_(_dev(b["done"]))
    raw_v, batch.v = _guarded((ROWS, G), torch.float32, b["v"])
    raw_q, batch.q = _guarded((ROWS, G), torch.float32, b["q"])
    return batch, raw_v, raw_q


@pytest.mark.parametrize("G", [1, 3, 64, 65, 257])
def test_value_targets_is_the_model_on_hand_filled_batches(G):
    seen_change = 0
    for sixteenths in (True, False):
        for kind in ("none", "zero", "late"):
            b = M.hand_batch(G, 100 * G + 7 * sixteenths + len(kind), sixteenths, kind, short_rows=True, random_v=True)
            if G >= ROWS:
                assert sorted(set(b["length"].tolist())) == list(range(1, ROWS + 1))
                assert (b["rows"] == 0).any() and ((b["rows"] > 0) & (b["rows"] < b["length"])).any()
            batch, raw_v, raw_q = _hand(G, b)
            exact, rows_t = _dev(b["exact"]), _dev(b["rows"])
            for rows, rows_np in ((None, None), (rows_t, b["rows"])):
                for mode in ("mix", "td"):
                    for lam in (0.0, 0.5, 0.8, 1.0):
                        batch.v.copy_(_dev(b["v"]))
                        batch.value_targets(mode, lam, rows=rows, exact=exact)
                        want = M.value_targets(mode, lam, rows_np, b["length"], b["done"], b["exact"], b["q"], b["v"])
                        got = batch.v.cpu().numpy()
                        assert np.array_equal(M.bits(got), M.bits(want)), (sixteenths, kind, rows is None, mode, lam,
                                                                          np.argwhere(M.bits(got) != M.bits(want))[:4])
                        seen_change += int((M.bits(got) != M.bits(b["v"])).sum())
                        L = b["length"] if rows_np is None else rows_np
                        past = np.arange(ROWS)[:, None] >= L[None, :]
                        assert np.array_equal(M.bits(got)[past], M.bits(b["v"])[past])         # rows at or past L
                        assert not np.signbit(got[got == 0]).any() and not np.isnan(got).any()
                        assert _guards_hold(raw_v, raw_q)
            # every byte of q, done, length, rows and exact
            assert np.array_equal(M.bits(batch.q.cpu().numpy()), M.bits(b["q"]))
            assert np.array_equal(batch.done.cpu().numpy(), b["done"]) and np.array_equal(batch.length.cpu().numpy(), b["length"])
            assert np.array_equal(rows_t.cpu().numpy(), b["rows"])
            assert exact is None or np.array_equal(exact.cpu().numpy(), b["exact"])
    assert seen_change > 0


@pytest.mark.parametrize("G", [1, 3, 64, 65, 257])
def test_td_with_lambda_one_and_mix_with_lambda_zero_leave_every_bit(G):
    for sixteenths in (True, False):
        for kind in ("none", "zero"):
            b = M.hand_batch(G, 31 * G + sixteenths, sixteenths, kind, short_rows=True)           # v: the record's outcome
            batch, raw_v, raw_q = _hand(G, b)
            for rows in (None, _dev(b["rows"])):
                for mode, lam in (("td", 1.0), ("mix", 0.0)):
                    batch.value_targets(mode, lam, rows=rows, exact=_dev(b["exact"]))
                    assert np.array_equal(M.bits(batch.v.cpu().numpy()), M.bits(b["v"])), (sixteenths, kind, mode)
            batch.value_targets("td", 0.0)                                                        # and the kernel does write
            assert G == 1 or not np.array_equal(M.bits(batch.v.cpu().numpy()), M.bits(b["v"]))
            assert _guards_hold(raw_v, raw_q)
    b = M.hand_batch(G, 5, True, random_v=True)                                                   # mix(0): any v
    batch, _, _ = _hand(G, b)
    batch.value_targets("mix", 0.0)
    assert np.array_equal(M.bits(batch.v.cpu().numpy()), M.bits(b["v"]))


def test_value_targets_checks_its_arguments():
    G = 3
    batch = SelfPlayBatch(G, torch.device(DEV), _native.lib().qttt_state_bytes(G))
    with pytest.raises(ValueError, match="has no q"):
        batch.value_targets("td", 0.5)
    batch.alloc_q()
    for bad in (-0.1, 1.1, float("nan"), True, "1"):
        with pytest.raises(ValueError, match=r"lam must be a number in \[0, 1\]"):
            batch.value_targets("td", bad)
    with pytest.raises(ValueError, match="mode must be"):
        batch.value_targets("nstep", 0.5)
    with pytest.raises(ValueError):
        batch.value_targets("td", 0.5, rows=torch.zeros(G, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        batch.value_targets("td", 0.5, exact=torch.zeros((ROWS, G + 1), dtype=torch.uint8, device=DEV))
    assert not hasattr(batch.augment([0]), "q")


# ---------------------------------------------------------------- the record kernel
def _sp(G, net, **kw):
    kw = dict(dict(n_rollouts=16, num_simulations=2, seed=SEED, device=DEV, value_targets=(1.0, -1.0)), **kw)
    if net:
        kw.update(net=S.golden_net(), leaf_eval="value")
    return SelfPlay(G, **kw)


def _random_rows(G, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-16, 17, (ROWS, G)) / 16.0).astype(np.float32) + np.float32(0.0)


def _check_record(sp, tree, ply, length, seed, expect_visits=True):
    """One record_value on a fresh guarded batch with the given lengths; q against the model on root_stats()."""
    G = sp.num_games
    batch = SelfPlayBatch(G, torch.device(DEV), _native.lib().qttt_state_bytes(G))
    batch.length.copy_(_dev(np.asarray(length, np.uint8)))
    v0, q0 = _random_rows(G, seed), _random_rows(G, seed + 1)
    raw_v, batch.v = _guarded((ROWS, G), torch.float32, v0)
    raw_q, batch.q = _guarded((ROWS, G), torch.float32, q0)
    before = tree.tree.clone()
    st = tree.root_stats()
    sp.record_value(tree, ply, batch)
    got = batch.q.cpu().numpy()
    W, N = st["W"].cpu().numpy(), st["N"].cpu().numpy()
    want = M.record_value(W, N, ply, np.asarray(length, np.uint8), q0, v0)
    assert np.array_equal(M.bits(got), M.bits(want)), np.argwhere(M.bits(got) != M.bits(want))[:6]
    assert torch.equal(tree.tree, before)                                    # the tree's bytes
    assert np.array_equal(M.bits(batch.v.cpu().numpy()), M.bits(v0)) and _guards_hold(raw_v, raw_q)
    assert np.array_equal(batch.length.cpu().numpy(), np.asarray(length, np.uint8))
    assert not np.signbit(got[got == 0]).any() and not np.isnan(got).any()
    written = M.bits(want) != M.bits(q0)
    rows = np.asarray(length, np.int64) if ply is None else np.full(G, ply)
    ok = (rows < ROWS) & (np.asarray(length) == rows)
    assert not written[:, ~ok].any()                                         # the other games, and below: the other rows
    for g in np.flatnonzero(ok):
        assert not np.delete(written[:, g], rows[g]).any()
    total = N.sum(1)
    if expect_visits:
        assert (total[ok] > 0).all() and written.any()
        # Reanalyser's own lines on the same statistics: the sign, not the bits
        Nd = st["N"].double()
        searched = torch.where(Nd > 0, Nd * st["Q"], torch.zeros_like(Nd)).sum(1) / Nd.sum(1).clamp(min=1.0)
        mine = torch.as_tensor(got, device=DEV)[torch.as_tensor(np.minimum(rows, ROWS - 1), device=DEV), torch.arange(G, device=DEV)]
        sel = torch.as_tensor(ok, device=DEV)
        assert float((mine.double() - searched)[sel].abs().max()) <= 1e-6
        assert float(searched[sel].abs().max()) > 1e-3
    else:
        assert (total == 0).all()
        assert np.array_equal(M.bits(got)[rows[ok], np.flatnonzero(ok)], M.bits(v0)[rows[ok], np.flatnonzero(ok)])
    return got


@pytest.mark.parametrize("G", [8, 65])
@pytest.mark.parametrize("net", [True, False], ids=["golden", "uniform"])
def test_record_value_is_the_model_on_the_roots_statistics(G, net):
    for compact in (False, True):
        sp = _sp(G, net, compact=compact)
        env, tree = sp._new_game_objects(SEED)
        batch = sp.new_batch()
        assert not hasattr(batch, "q")                                       # the keywords were not given
        sp._search(tree)
        if not compact:
            _check_record(sp, tree, 0, np.zeros(G), 1)                       # after a reset
            _check_record(sp, tree, None, np.zeros(G), 2)                    # the stream form at length 0
        for ply in range(2):                                                 # two moves with sync [and compact()]
            if ply:
                sp._search(tree)
            env.step_raw(sp.record(tree, ply, batch))
            tree.sync(env)
            if compact:
                tree.compact()
        sp._search(tree)
        _check_record(sp, tree, 2, np.full(G, 2), 3)
        mixed = np.where(np.arange(G) % 2 == 0, 3, 5)
        _check_record(sp, tree, 3, mixed, 4)                                 # lockstep: only the games whose length is the ply
        lengths = (np.arange(G) * 3 + 1) % (ROWS + 1)                        # the stream form: every game its own row, 10: none
        assert G < 11 or (lengths == ROWS).any()
        _check_record(sp, tree, None, lengths, 5)
        if compact:
            continue
        for ply in range(2, ROWS):                                           # play the games out: every root is terminal
            if 2 < ply < ROWS - 1:
                sp._search(tree)
            env.step_raw(sp.record(tree, ply, batch))
            tree.sync(env)
        assert bool((batch.done.sum(0) == 1).all())
        _check_record(sp, tree, 7, np.full(G, 7), 6, expect_visits=False)    # a terminal root takes the row's v
        _check_record(sp, tree, None, (np.arange(G) % ROWS), 7, expect_visits=False)


# ---------------------------------------------------------------- end to end
def _e2e(G, **kw):
    kw = dict(dict(n_rollouts=8, net=S.golden_net(), seed=SEED, device=DEV, leaf_eval="value", value_targets=(1.0, -1.0)), **kw)
    return SelfPlay(G, **kw)


def _np(batch):
    out = {f: M.bits(getattr(batch, f).cpu().numpy()) for f in FIELDS}
    for f in ("exact", "q"):
        if hasattr(batch, f):
            out[f] = getattr(batch, f).cpu().numpy()
    return out


_PLAIN = {}


def _plain(G, **kw):
    key = (G, tuple(sorted(kw.items())))
    if key not in _PLAIN:
        _PLAIN[key] = _np(_e2e(G, **kw).play(SEED))
    return _PLAIN[key]


@pytest.mark.parametrize("kw,extra", [(dict(td_lambda=0.8), {}), (dict(td_lambda=0.8), dict(exact_targets=7)),
                                      (dict(value_mix=0.5), {}), (dict(value_mix=0.5), dict(exact_targets=7)),
                                      (dict(td_lambda=0.0), {})],
                         ids=["td", "td_exact", "mix", "mix_exact", "one_step"])
def test_play_rewrites_v_by_the_model_and_nothing_else(kw, extra):
    G = 16
    plain = _plain(G, **extra)
    assert "q" not in plain
    got = _np(_e2e(G, **kw, **extra).play(SEED))
    for f in FIELDS:
        if f != "v":
            assert np.array_equal(got[f], plain[f]), f
    exact = plain.get("exact")
    assert (exact is None) == (not extra) and (exact is None or np.array_equal(got["exact"], exact))
    mode, lam = ("td", kw["td_lambda"]) if "td_lambda" in kw else ("mix", kw["value_mix"])
    want = M.value_targets(mode, lam, None, plain["length"], plain["done"], exact, got["q"], plain["v"].view(np.float32))
    assert np.array_equal(got["v"], M.bits(want)), np.argwhere(got["v"] != M.bits(want))[:6]
    v, pv = got["v"].view(np.float32), plain["v"].view(np.float32)
    live = (np.arange(ROWS)[:, None] < plain["length"][None, :]) & (plain["done"] == 0)
    assert (got["v"] != plain["v"])[live].any() and np.array_equal(got["v"][~live], plain["v"][~live])
    assert np.isfinite(got["q"]).all() and (got["q"][live] != 0).any() and (np.abs(v) <= 1).all()
    if exact is not None:
        assert exact.sum() > 0 and np.array_equal(got["v"][exact == 1], plain["v"][exact == 1])    # late rows are exact
        early = live & (exact == 0)
        # and the early rows are bootstrapped through them: not what the same rule gives without the exact mask
        blind = M.value_targets(mode, lam, None, plain["length"], plain["done"], None, got["q"], pv)
        assert early.any() and ((M.bits(blind) != got["v"]) & early).any() == (mode == "td")
    if mode == "td" and lam == 0.0:                                          # the one-step target of a searched row
        t, g = np.argwhere(live[1:] & live[:-1] & (True if exact is None else exact[1:] == 0))[0]
        assert v[t, g] == -got["q"][t + 1, g] or got["q"][t + 1, g] == 0


@pytest.mark.parametrize("plies", [14, 26])           # 26: second incarnations too, whose slots hold the q of the game before
def test_the_stream_hands_the_ring_the_model_s_values(plies):
    G, lam = 8, 0.8
    sp = _e2e(G, td_lambda=lam)
    w = S.Watch(sp)
    ring = ReplayBuffer(4096, device=DEV)
    stats = sp.stream(ring, plies, seed=SEED)
    refs = {}
    assert len(w.games) >= G
    for g, start, ply, got in w.games:
        if start not in refs:
            pb = _e2e(G).play(SEED, start_ply=start)
            plain = _np(pb)
            withq = _np(_e2e(G, td_lambda=lam).play(SEED, start_ply=start))
            want = M.value_targets("td", lam, None, plain["length"], plain["done"], None, withq["q"], plain["v"].view(np.float32))
            assert np.array_equal(M.bits(want), withq["v"])
            refs[start] = (S.arrays(pb), M.bits(want).view(np.int32))
        ref, want = refs[start]
        ref_game = S.game(ref, g)
        assert got["v"] == want[:got["length"], g].tolist(), (g, start, ply)
        assert got["v"] != ref_game["v"] or got["length"] < 3
        for k in ("length", "winner", "states", "pi", "mask", "done", "action36"):
            assert got[k] == ref_game[k], (g, start, k)
    assert plies == 14 or len(refs) > 2
    S.assert_ring(ring, w, 4096)                                             # the ring holds the staging rows as appended
    assert int(stats.samples) == int(ring.views()["written"].item())


def test_the_stream_composes_exact_targets_and_the_mix():
    G, plies = 8, 12
    ex, both = _e2e(G, exact_targets=7), _e2e(G, exact_targets=7, value_mix=0.5)
    we, wb = S.Watch(ex), S.Watch(both)
    ex.stream(ReplayBuffer(2048, device=DEV), plies, seed=SEED)
    both.stream(ReplayBuffer(2048, device=DEV), plies, seed=SEED)
    harvested = changed = 0
    for (fin, hl, a), (fin2, hl2, a2) in zip(we.plies, wb.plies):
        assert np.array_equal(fin, fin2) and np.array_equal(hl, hl2)
        for k in a:
            if k != "v":
                assert np.array_equal(a[k], a2[k]), k
        harvested += int(fin.sum())
        changed += int((a["v"] != a2["v"])[:, fin != 0].sum())
        assert np.array_equal(a["v"][:, fin == 0], a2["v"][:, fin == 0])     # a game in progress keeps its staging rows
    assert harvested >= G and changed > 0
    exact = both._stream["exact"].cpu().numpy()                              # the mask of the last ply's relabel
    assert exact.shape == (ROWS, G) and set(np.unique(exact)) <= {0, 1}


# ---------------------------------------------------------------- the defaults issue the parent's calls
def test_without_the_keywords_play_and_stream_issue_the_calls_they_always_did(monkeypatch):
    G = 8
    log = []
    inner = LibCaller._call

    def logged(self, name, *args):
        log.append(name)
        return inner(self, name, *args)
    monkeypatch.setattr(LibCaller, "_call", logged)
    L = _native.lib()
    counts = {}
    for name in _native.SELFPLAY_VALUE_SIGNATURES:
        def counted(*args, _fn=getattr(L, name), _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _fn(*args)
        monkeypatch.setattr(L, name, counted)

    sp = _e2e(G, exact_targets=7)
    b = sp.play(SEED)
    played, log[:] = list(log), []
    assert not hasattr(b, "q") and sp.value_mode is None and counts == {}
    # the parent commit's loop, entry by entry
    old = _e2e(G, exact_targets=7)
    env, tree = old._new_game_objects(SEED)
    batch = old.new_batch()
    for ply in range(ROWS):
        if ply < ROWS - 1:
            tree.contemplate(old.n_rollouts)
        env.step_raw(old.record(tree, ply, batch))
        tree.sync(env)
    assert played == log and "qttt_selfplay_record" in played and not any("value_targets" in n or "record_value" in n for n in played)
    log[:] = []
    sp.stream(ReplayBuffer(512, device=DEV), 3, seed=SEED)
    assert counts == {} and not hasattr(sp._stream["batch"], "q") and "exact" not in sp._stream
    assert log.count("qttt_selfplay_record_stream") == 3 and log.count("qttt_selfplay_harvest") == 3
    assert not any("record_value" in n for n in log)

    log[:] = []
    td = _e2e(G, td_lambda=0.8)
    td.play(SEED)
    assert counts == {"qttt_selfplay_record_value": ROWS - 1, "qttt_selfplay_value_targets": 1}
    at = [i for i, n in enumerate(log) if n == "qttt_selfplay_record_value"]
    assert all(log[i + 1] == "qttt_selfplay_record" for i in at)             # before the ply's record, every time
    counts.clear()
    log[:] = []
    td.stream(ReplayBuffer(512, device=DEV), 3, seed=SEED)
    assert counts == {"qttt_selfplay_record_value": 3, "qttt_selfplay_value_targets": 3}
    at = [i for i, n in enumerate(log) if n == "qttt_selfplay_record_value"]
    assert all(log[i + 1] == "qttt_selfplay_record_stream" for i in at)

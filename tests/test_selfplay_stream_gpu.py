"""SelfPlay.stream on the MI355X (include/qttt_selfplay_stream.h): finished games restart in place and
feed the ring.  The contract is two equalities with play(): (A) until a slot first finishes, its game is play(seed)'s in
that slot; (B) a game that starts at stream ply p is play(seed, start_ply=p)'s.  Both are checked bit for bit on all eight
fields of every harvested game; then the ring against tests/replay_model.py, the restart's neighbours, continuation,
play()'s unchanged defaults, and compaction.  R = 8 rollouts, num_simulations = 2: every case takes a few seconds."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_model as RM  # noqa: E402
import tree_harness as H  # noqa: E402
from qtttgym_amd import ReplayBuffer, SelfPlay, _native  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = H.DEV
ROWS = RM.ROWS
SEED = 2026
GUARD, SENTINEL = 256, 0xA5


_NET = []


def golden_net():
    """The golden model_eval.npz network, loaded once."""
    if not _NET:
        _NET.append(H.net(torch.float32))
    return _NET[0]


def config(name):
    """The constructor arguments of the configurations the issue names."""
    base = dict(n_rollouts=8, num_simulations=2, seed=SEED, device=DEV)
    if name == "uniform":
        return dict(base, net=None)
    if name == "value":
        return dict(base, net=golden_net(), leaf_eval="value", leaves=4)
    if name == "gumbel":          # nine rollouts: the one that gives the root its priors, then a budget of eight
        return dict(base, n_rollouts=9, net=golden_net(), leaf_eval="value", leaves=4, root_policy="gumbel")
    if name == "noise":           # the noise and sampled-move counters run across restarts
        return dict(base, net=None, root_noise=(0.25, 0.3), sample_plies=2)
    raise KeyError(name)


def arrays(batch):
    """A SelfPlayBatch as numpy words: the eight fields that make a game, floats as their bits."""
    G = batch.num_games
    stride = (G + 63) // 64 * 64
    return {"states": batch.states.cpu().numpy().view(np.uint64).reshape(ROWS, 2, stride)[:, :, :G].copy(),
            "pi": batch.pi.view(torch.int64).cpu().numpy(), "mask": batch.mask.cpu().numpy(),
            "done": batch.done.cpu().numpy(), "v": batch.v.view(torch.int32).cpu().numpy(),
            "action36": batch.action36.cpu().numpy(), "length": batch.length.cpu().numpy(),
            "winner": batch.winner.cpu().numpy()}


def game(a, g):
    """Game g of arrays(): its rows below its length, field by field."""
    n = int(a["length"][g])
    out = {"length": n, "winner": int(a["winner"][g]), "states": a["states"][:n, :, g].tolist()}
    for k in ("pi", "mask", "done", "v", "action36"):
        out[k] = a[k][:n, g].tolist()
    return out


def assert_same_game(got, want, what):
    for k in ("length", "winner", "states", "pi", "mask", "done", "v", "action36"):
        assert got[k] == want[k], (what, k)


class Watch:
    """Wraps the restart of a SelfPlay's stream: per stream ply, the staging batch as it is appended (after the harvest,
    before the restart), the finished and harvest_len arrays, and the start ply of every harvested game."""

    def __init__(self, sp, neighbours=False):
        self.sp, self.plies, self.start, self.games, self.neighbours = sp, [], None, [], neighbours
        inner = sp._stream_restart

        def restart(st):
            fin = st["finished"].cpu().numpy().copy()
            hl = st["harvest_len"].cpu().numpy().copy()
            a = arrays(st["batch"])
            raw = self.raw(st) if neighbours else None
            inner(st)
            if neighbours:
                self.check_neighbours(st, raw, self.raw(st), fin)
            self.note(len(self.plies), fin, hl, a)
        sp._stream_restart = restart

    def note(self, ply, fin, hl, a):
        G = len(fin)
        if self.start is None:
            self.start = np.zeros(G, np.int64)
        assert np.array_equal(hl != 0, fin != 0) and np.array_equal(hl[fin != 0], a["length"][fin != 0])
        for g in np.nonzero(fin)[0]:
            self.games.append((int(g), int(self.start[g]), ply, game(a, g)))
            self.start[g] = ply + 1
        self.plies.append((fin, hl, a))

    def raw(self, st):
        """Every byte the restart may write: the trees, the packed states, the staging rows."""
        b = st["batch"]
        return {"tree": st["tree"].tree.cpu().numpy().copy(), "state": st["env"].state.cpu().numpy().copy(),
                **{f: getattr(b, f).view(-1).view(torch.uint8).cpu().numpy().copy() for f in b._FIELDS}}

    def check_neighbours(self, st, before, after, fin):
        G, cap = len(fin), st["tree"].capacity
        keep = np.nonzero(fin == 0)[0]
        stride = (G + 63) // 64 * 64
        hdr = _native.TREE_GAME_BYTES * G
        nodes = _native.TREE_NODE_BYTES * G * cap
        for what, lo, per in (("header", 0, _native.TREE_GAME_BYTES), ("nodes", hdr, _native.TREE_NODE_BYTES * cap),
                              ("priors", hdr + nodes, _native.TREE_PRIOR_BYTES * cap)):
            b = before["tree"][lo:lo + per * G].reshape(G, per)
            a = after["tree"][lo:lo + per * G].reshape(G, per)
            assert np.array_equal(a[keep], b[keep]), what
        assert np.array_equal(after["tree"][hdr + nodes + _native.TREE_PRIOR_BYTES * cap * G:],
                              before["tree"][hdr + nodes + _native.TREE_PRIOR_BYTES * cap * G:]), "behind the trees"
        sb, sa = (x["state"].view(np.uint64).reshape(2, stride) for x in (before, after))
        assert np.array_equal(sa[:, keep], sb[:, keep]) and np.array_equal(sa[:, G:], sb[:, G:])
        assert not sa[:, np.nonzero(fin)[0]].any()                          # the finished slots: the empty board
        per_game = {"pi": 36 * 8, "mask": 36, "done": 1, "v": 4, "action36": 1}
        for f, n in per_game.items():
            b, a = (x[f].reshape(ROWS, G, n) for x in (before, after))
            assert np.array_equal(a[:, keep], b[:, keep]), f
            assert not a[:, np.nonzero(fin)[0]].any(), f                    # every row of a restarted slot is zero
        pb, pa = (x["states"].view(np.uint64).reshape(ROWS, 2, stride) for x in (before, after))
        assert np.array_equal(pa[:, :, keep], pb[:, :, keep]) and np.array_equal(pa[:, :, G:], pb[:, :, G:])
        for f, n in (("length", 1), ("winner", 1), ("actions", 2)):
            b, a = (x[f].reshape(G, n) for x in (before, after))
            assert np.array_equal(a[keep], b[keep]), f
        assert not after["length"][np.nonzero(fin)[0]].any()


_REF = {}


def reference(name, G, p=0):
    """play(SEED, start_ply=p) of the configuration, computed once and shared."""
    key = (name, G, p)
    if key not in _REF:
        sp = SelfPlay(G, **config(name))
        _REF[key] = arrays(sp.play(SEED, start_ply=p))
    return _REF[key]


# ---------------------------------------------------------------- (A) first incarnations
@pytest.mark.parametrize("G", [1, 63, 64, 65])
@pytest.mark.parametrize("name", ["uniform", "value", "gumbel"])
def test_until_a_slot_first_finishes_its_game_is_plays(name, G):
    sp = SelfPlay(G, **config(name))
    w = Watch(sp)
    ring = ReplayBuffer(4096, device=DEV)
    ref = reference(name, G)
    seen = set()
    for ply in range(ROWS - 1):                     # a game is nine moves at most: by ply 8 every slot has finished once
        sp.stream(ring, 1, seed=SEED)
    for g, start, ply, got in w.games:
        if start == 0:
            assert g not in seen
            seen.add(g)
            assert_same_game(got, game(ref, g), (name, G, g, ply))
            assert got["length"] == ply + 2         # harvested at the ply of its last move, the terminal row included
    assert seen == set(range(G))                    # no slot is left out


# ---------------------------------------------------------------- (B) every later incarnation
def run_and_check_every_game(name, G, plies, capacity=4096, neighbours=False, **extra):
    sp = SelfPlay(G, **dict(config(name), **extra))
    w = Watch(sp, neighbours=neighbours)
    ring = ReplayBuffer(capacity, device=DEV)
    stats = sp.stream(ring, plies, seed=SEED)
    assert len(w.plies) == plies
    restarts = np.zeros(G, np.int64)
    for g, start, ply, got in w.games:              # every harvested game
        assert_same_game(got, game(reference(name, G, start), g), (name, G, g, start, ply))
        restarts[g] += 1
    assert restarts.min() >= 2 and len({start for _, start, _, _ in w.games}) > 2
    assert np.array_equal(stats.games.cpu().numpy(), restarts)
    assert int(stats.samples) == sum(got["length"] for _, _, _, got in w.games)
    wins = [sum(1 for *_, got in w.games if got["winner"] == k) for k in (1, 0, -1)]
    assert stats.winners.cpu().tolist() == wins
    return sp, w, ring


@pytest.mark.parametrize("name", ["uniform", "value", "noise"])
@pytest.mark.parametrize("G,plies", [(8, 30), (64, 24)])
def test_a_game_that_starts_at_ply_p_is_play_from_start_ply_p(name, G, plies):
    sp, w, ring = run_and_check_every_game(name, G, plies)
    if G == 64:                                     # the ring: the staging batch under the masked lengths, ply by ply
        assert_ring(ring, w, 4096)


# ---------------------------------------------------------------- the ring
def assert_ring(ring, w, capacity):
    model = RM.Ring(capacity)
    for fin, hl, a in w.plies:
        G = len(fin)
        stride = (G + 63) // 64 * 64
        planes = np.zeros((ROWS, 2, stride), np.uint64)
        planes[:, :, :G] = a["states"]
        model.append(planes.reshape(ROWS, -1).view(np.uint8), a["pi"].view(np.float64), a["mask"], a["done"],
                     a["v"].view(np.float32), hl)
    v = ring.views()
    assert int(v["written"].item()) == model.written
    got = {k: v[k].cpu().numpy() for k in ("P", "Q", "mask", "done")}
    got["pi"] = v["pi"].view(torch.int64).cpu().numpy()
    got["v"] = v["v"].view(torch.int32).cpu().numpy()
    for k, x in got.items():
        want = getattr(model, k)
        assert np.array_equal(x.view(want.dtype), want), k


@pytest.mark.parametrize("G,plies,capacity", [(257, 12, 4096), (64, 24, 37)])
def test_the_ring_is_the_model_with_two_scan_levels_and_when_it_wraps_mid_stream(G, plies, capacity):
    sp = SelfPlay(G, **config("uniform"))
    w = Watch(sp)
    ring = ReplayBuffer(capacity, device=DEV)
    stats = sp.stream(ring, plies, seed=SEED)
    assert_ring(ring, w, capacity)
    assert int(stats.samples) == int(ring.views()["written"].item()) > capacity * (capacity == 37)


# ---------------------------------------------------------------- the restart leaves its neighbours alone
def test_restart_leaves_unfinished_slots_and_guard_bytes_alone():
    G, plies = 8, 20
    sp = SelfPlay(G, **config("uniform"))
    ring = ReplayBuffer(4096, device=DEV)
    sp.stream(ring, 0, seed=SEED)                   # the stream's buffers exist; none has been written
    st = sp._stream
    guarded = {}

    def guard(t):
        raw = torch.full((t.numel() * t.element_size() + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        inner = raw[GUARD:GUARD + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
        inner.copy_(t)
        guarded[id(inner)] = raw
        return inner
    for k in ("harvest_len", "finished", "games_done", "tally"):
        st[k] = guard(st[k])
    for f in st["batch"]._FIELDS:
        setattr(st["batch"], f, guard(getattr(st["batch"], f)))
    st["tree"].tree = guard(st["tree"].tree)
    st["env"].state = guard(st["env"].state)
    w = Watch(sp, neighbours=True)
    sp.stream(ring, plies)
    assert sum(int(f.sum()) for f, _, _ in w.plies) >= 2 * G
    for raw in guarded.values():
        assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all()


# ---------------------------------------------------------------- continuation
def stream_state(sp, ring):
    st = sp._stream
    out = {"ring": ring.buffer.cpu().numpy().copy(), "state": st["env"].state.cpu().numpy().copy(),
           "games": st["games_done"].cpu().numpy().copy(), "tally": st["tally"].cpu().numpy().copy(),
           "counters": (st["env"].step_idx, st["tree"].rollout_idx, st["tree"].noise_idx, st["tree"].gumbel_idx, st["ply"])}
    out.update({k: v.tolist() for k, v in arrays(st["batch"]).items()})
    out["roots"] = {k: v.cpu().numpy().tolist() for k, v in st["tree"].root_stats().items()}
    return out


@pytest.mark.parametrize("name", ["uniform", "noise"])
def test_seven_plies_then_five_are_twelve_and_a_reset_reproduces_the_ring(name):
    G = 8
    one, ring1 = SelfPlay(G, **config(name)), ReplayBuffer(512, device=DEV)
    one.stream(ring1, 12, seed=SEED)
    two, ring2 = SelfPlay(G, **config(name)), ReplayBuffer(512, device=DEV)
    two.stream(ring2, 7, seed=SEED)
    s = two.stream(ring2, 5)
    a, b = stream_state(one, ring1), stream_state(two, ring2)
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    assert int(s.samples) == int(ring2.views()["written"].item()) > 0
    with pytest.raises(ValueError):
        two.stream(ring2, 1, seed=SEED + 1)          # another seed while games are in progress
    with pytest.raises(ValueError):
        two.stream(ring2.buffer, 1)                  # not a ReplayBuffer
    two.stream_reset()
    ring3 = ReplayBuffer(512, device=DEV)
    two.stream(ring3, 12, seed=SEED)
    assert np.array_equal(ring3.buffer.cpu().numpy(), a["ring"])


def test_a_fresh_seed_when_the_counters_run_out_and_games_after_it_are_plays():
    """stream_epoch_plies = 11 stands in for the counters' limits: ply 11 runs with seed + 2**32 and the counters at 0."""
    G = 8
    sp = SelfPlay(G, **config("noise"))
    sp.stream_epoch_plies = 11
    w = Watch(sp)
    sp.stream(ReplayBuffer(512, device=DEV), 22, seed=SEED)
    st = sp._stream
    assert st["epoch"] == 1 and st["env"].seed == SEED + (1 << 32) and st["tree"].seed == 2 * st["env"].seed + 1
    assert (st["env"].step_idx, st["tree"].rollout_idx, st["tree"].noise_idx) == (11, 88, 11)
    checked = 0
    for g, start, ply, got in w.games:
        if start >= 11:                              # born under the second seed, at its ply start - 11
            ref = SelfPlay(G, **config("noise"))
            assert_same_game(got, game(arrays(ref.play(SEED + (1 << 32), start_ply=start - 11)), g), (g, start))
            checked += 1
    assert checked > 0


# ---------------------------------------------------------------- play()'s defaults
@pytest.mark.parametrize("name", ["uniform", "value", "gumbel", "noise"])
def test_play_without_start_ply_is_the_lockstep_record_of_the_old_entries(name):
    G = 65
    a = reference(name, G)
    sp = SelfPlay(G, **config(name))
    b = arrays(sp.play(SEED))
    # the parent commit's loop, entry by entry
    old = SelfPlay(G, **config(name))
    env, tree = old._new_game_objects(SEED)
    batch = old.new_batch()
    bufs = [getattr(batch, f).data_ptr() for f in batch._FIELDS]
    for ply in range(ROWS):
        if ply < ROWS - 1:
            if old.root_noise is None:
                tree.contemplate(old.n_rollouts)
            else:
                tree.contemplate(1)
                tree.add_root_noise(*old.root_noise)
                tree.contemplate(old.n_rollouts - 1)
        head = (tree.tree.data_ptr(), G, tree.capacity, ply, old.n_rollouts, old.alpha, old.v_first, old.v_second, *bufs)
        if name == "gumbel":
            old._call("qttt_selfplay_record_gumbel", *head, tree._gumbel["rec"].data_ptr(), tree.c_visit, tree.c_scale)
        elif name == "noise":
            old._call("qttt_selfplay_record_sampled", *head, tree.seed, tree.board_offset, old.temperature, old.sample_plies)
        else:
            old._call("qttt_selfplay_record", *head)
        env.step_raw(batch.actions)
        tree.sync(env)
    c = arrays(batch)
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), (name, k)
    assert a["length"].min() >= 6 and (a["done"].sum(0) == 1).all()


def test_a_lockstep_batch_through_the_stream_record_is_the_lockstep_batch():
    """play(start_ply=p) with sampled moves records through qttt_selfplay_record_stream_sampled: at draw_index = ply its
    rows are the lockstep entry's, finished games riding along included."""
    G = 65
    sp = SelfPlay(G, **config("noise"))
    a = reference("noise", G)
    env, tree = sp._new_game_objects(SEED)
    batch = sp.new_batch()
    for ply in range(ROWS):
        if ply < ROWS - 1:
            sp._search(tree)
        env.step_raw(sp.record(tree, ply, batch, draw_index=ply))
        tree.sync(env)
    b = arrays(batch)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- compaction
def test_compaction_harvests_the_same_games():
    G, plies = 8, 20
    plain, ring1 = SelfPlay(G, **config("uniform")), ReplayBuffer(512, device=DEV)
    plain.stream(ring1, plies, seed=SEED)
    # (the kept subtrees of 20 plies of always-live slots pass the default carry of 2 R + 2 = 18 nodes once, which stream()
    # refuses as play() does, before a node is lost; 64 is room enough and still less than half the uncompacted pool)
    comp, ring2 = SelfPlay(G, compact=True, carry=64, **config("uniform")), ReplayBuffer(512, device=DEV)
    assert comp.capacity == 80 < plain.capacity == 171
    s = comp.stream(ring2, plies, seed=SEED)
    assert np.array_equal(ring1.buffer.cpu().numpy(), ring2.buffer.cpu().numpy())
    assert int(s.games.sum()) >= 2 * G

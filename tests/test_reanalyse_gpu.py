"""Reanalysis on the device (include/qttt_replay_reanalyse.h, ReplayBuffer.gather / update, qtttgym_amd.Reanalyser) against
its model (tests/reanalyse_model.py) and against the composed route: the gathered window and the updated ring bit for
bit, the staleness guard under appends in between, and a whole Reanalyser.run() against gather -> fresh TreeSearch ->
contemplate -> record by hand.  Floats are compared as words."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reanalyse_model as M  # noqa: E402
import tree_harness  # noqa: E402
from qtttgym_amd import (Reanalyser, ReplayBuffer, SelfPlay, SelfPlayBatch, TreeSearch, VecEnv, _native)  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = _native.SELFPLAY_ROWS
SEED = 2026
NAN_PAYLOAD = 0x7FF8000000000123


# ---------------------------------------------------------------- rings (the recipe of test_replay_gpu.py's fixture)
def random_play_batch(G, seed, full=False):
    """Boards stepped at random to plies 0..9 with random pi / v / done; length 1..10, or 10 everywhere."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    env = VecEnv(G, device=DEV, seed=seed)
    b = SelfPlayBatch(G, torch.device(DEV), env.state.numel())
    for t in range(ROWS):
        b.states[t].copy_(env.state)
        b.mask[t].copy_(env.encode()[1])
        env.step_random_many(1)
    b.pi.copy_(torch.rand(b.pi.shape, dtype=torch.float64, device=DEV, generator=gen))
    b.v.copy_(torch.rand(b.v.shape, device=DEV, generator=gen) * 2 - 1)
    b.done.copy_(torch.randint(0, 2, b.done.shape, device=DEV, generator=gen).to(torch.uint8))
    b.length.copy_(torch.randint(1, 11, (G,), device=DEV, generator=gen).to(torch.uint8))
    if full:
        b.length.fill_(ROWS)
    return b


@pytest.fixture(scope="module")
def sources():
    """The two sources of every ring here: one real self-play of 64 games at 8 rollouts, and random-play rows."""
    return SelfPlay(64, n_rollouts=8, num_simulations=2, seed=5, device=DEV).play(), random_play_batch(64, 11)


def first_samples(batch, count):
    """A length tensor under which add() appends the first `count` samples of the batch (game-major)."""
    left, out = count, []
    for n in batch.length.clamp(max=ROWS).tolist():
        out.append(min(n, left))
        left -= out[-1]
    assert left == 0
    return torch.tensor(out, dtype=torch.uint8, device=DEV)


def build_ring(sources, capacity, n_played, n_random, seed=SEED):
    rb = ReplayBuffer(capacity, device=DEV, seed=seed)
    rb.add(sources[0], length=first_samples(sources[0], n_played))
    rb.add(sources[1], length=first_samples(sources[1], n_random))
    assert int(rb.views()["written"].item()) == n_played + n_random
    return rb


# capacity -> (samples of the self-play, of the random play): 7 and 37 wrapped, 64 exactly full, 300 not full
RINGS = {7: (40, 30), 37: (40, 30), 64: (34, 30), 300: (100, 80)}


def image(rb):
    """(written, the ring's buffer as a numpy image, writable views of its arrays as words)."""
    buf = rb.buffer.cpu().numpy().copy()
    C, off = rb.capacity, rb.offsets

    def view(name, dtype, size, cols=1):
        a = buf[off[name]:off[name] + size * C * cols].view(dtype)
        return a.reshape(C, cols) if cols > 1 else a
    arrays = {"P": view("P", np.uint64, 8), "Q": view("Q", np.uint64, 8), "pi": view("pi", np.uint64, 8, 36),
              "mask": view("mask", np.uint64, 8), "v": view("v", np.uint32, 4), "done": view("done", np.uint8, 1)}
    return int(buf[:8].view(np.uint64)[0]), buf, arrays


def random_targets(n, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    pi = torch.randint(0, 256, (n, 36 * 8), dtype=torch.uint8, device=DEV, generator=gen).view(torch.float64)
    if n > 1:
        pi[1].view(torch.int64).fill_(NAN_PAYLOAD)            # a NaN row with a payload
    v = torch.randint(0, 256, (n, 4), dtype=torch.uint8, device=DEV, generator=gen).view(torch.float32).view(n)
    return pi.contiguous(), v.contiguous()


def words(t, dtype):
    return t.contiguous().view(-1).view(torch.uint8).cpu().numpy().view(dtype)


def assert_window_is_model(win, want, what):
    state, slot, number, v, done = want
    assert win.slot.dtype == torch.int32 and win.number.dtype == torch.int64 and win.v.dtype == torch.float32
    assert np.array_equal(words(win.env.state, np.uint64), state), what
    assert np.array_equal(win.slot.cpu().numpy(), slot), what
    assert np.array_equal(win.number.cpu().numpy(), number), what
    assert np.array_equal(words(win.v, np.uint32), v), what
    assert np.array_equal(win.done.cpu().numpy(), done), what


# ---------------------------------------------------------------- gather
@pytest.mark.parametrize("capacity", [7, 37, 64, 300])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_gather_is_the_model(sources, capacity, n):
    rb = build_ring(sources, capacity, *RINGS[capacity])
    written, buf, arrays = image(rb)
    F = min(written, capacity)
    assert (written > capacity) == (capacity in (7, 37)) and (written == capacity) == (capacity == 64)
    # the hashed start, twice (two draws), then given starts: 0, one that crosses the wrap, one past F (taken modulo F)
    for k, start in enumerate((None, None, 0, F - 2, 3 * F + F - 1)):
        draw = rb.gathers
        win = rb.gather(n, start)
        assert rb.gathers == draw + 1
        want = M.gather(arrays, written, capacity, n, start, SEED, draw)
        assert_window_is_model(win, want, (capacity, n, start))
        held = want[1][want[1] >= 0]
        assert len(held) == min(n, F) and len(set(held.tolist())) == len(held)
        if n > F:                                             # the excess: no slot, the empty board
            assert (want[1][F:] == -1).all() and not win.env.state.view(torch.int64)[F:n].any()
            fresh = VecEnv(n - F, device=DEV)
            assert torch.equal(VecEnv.from_state(win.env.state, n).encode()[0][F:], fresh.encode()[0])
        if start == F - 2 and n >= 3 and F >= 3:              # this window crosses the wrap
            assert want[1][:3].tolist() == [F - 2, F - 1, 0]
        mask = win.mask                                       # the mask words: a torch index of views(), on request
        assert np.array_equal(mask.cpu().numpy().view(np.uint64)[:len(held)], arrays["mask"][held])
        assert not mask[len(held):].any()
    assert np.array_equal(rb.buffer.cpu().numpy(), buf)       # the ring is read only
    # the window into a caller's environment, and the checks of the arguments
    env = VecEnv(n, device=DEV)
    assert rb.gather(n, 1, env=env).env is env
    assert np.array_equal(words(env.state, np.uint64), M.gather(arrays, written, capacity, n, 1)[0])
    draw = rb.gathers
    for bad in (dict(n=-1), dict(n=n, start=-2), dict(n=n + 1, env=env), dict(n=n, env="env")):
        with pytest.raises(ValueError):
            rb.gather(**bad)
    assert rb.gathers == draw                                 # a refused call draws nothing
    with pytest.raises(ValueError):
        ReplayBuffer(8, device=DEV).gather(1)                 # before any add


def test_an_empty_ring_through_the_c_entry_gives_no_slots_and_empty_boards():
    L = _native.lib()
    n, cap = 70, 8
    ring = torch.zeros(int(L.qttt_replay_bytes(cap)), dtype=torch.uint8, device=DEV)
    sizes = (int(L.qttt_state_bytes(n)), 4 * n, 8 * n, 4 * n, n)
    for start in (-1, 0, 5):
        outs = [torch.full((s,), 0x55, dtype=torch.uint8, device=DEV) for s in sizes]
        with torch.cuda.device(DEV):
            stream = torch.cuda.current_stream().cuda_stream
            rc = L.qttt_replay_gather(ring.data_ptr(), cap, n, 1, 0, start, *[t.data_ptr() for t in outs], stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert not bool(outs[0].any()) and not bool(outs[3].any()) and not bool(outs[4].any())
        assert outs[1].view(torch.int32).tolist() == [-1] * n and outs[2].view(torch.int64).tolist() == [-1] * n
    assert not bool(ring.any())


# ---------------------------------------------------------------- update
@pytest.mark.parametrize("form", ["pi", "v", "both"])
@pytest.mark.parametrize("capacity,n", [(37, 20), (37, 37), (37, 45), (300, 1), (300, 65), (300, 257)])
def test_update_is_the_model(sources, capacity, n, form):
    rb = build_ring(sources, capacity, *RINGS[capacity])
    win = rb.gather(n, capacity - 3)
    pi, v = random_targets(n, 7 * n + capacity)
    written, buf, arrays = image(rb)
    pi_in, v_in = (pi if form != "v" else None), (v if form != "pi" else None)
    want = M.update(arrays, written, capacity, win.slot.cpu().numpy(), win.number.cpu().numpy(),
                    None if pi_in is None else words(pi, np.uint64).reshape(n, 36), None if v_in is None else words(v, np.uint32))
    got = rb.update(win, pi=pi_in, v=v_in)
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want != 0)
    assert np.array_equal(rb.buffer.cpu().numpy(), buf)       # the whole ring: nothing but the written pi / v moved
    slot, done = win.slot.cpu().numpy(), win.done.cpu().numpy()
    assert np.array_equal(want != 0, (slot >= 0) & (done == 0))          # nothing was appended: only done rows are kept
    if n >= 20:
        assert want.any() and not want[slot >= 0].all()       # both kinds: refreshed slots and terminal rows left alone
    if n > 1 and want[1] and form != "v":                     # the NaN's payload survives
        assert int(rb.views()["pi"].view(torch.int64)[int(slot[1]), 0]) == NAN_PAYLOAD
    for bad in (dict(), dict(pi=pi[:, :35]), dict(v=v.double()), dict(pi=pi.float()), dict(v=v[:-1]) if n > 1 else dict()):
        with pytest.raises(ValueError):
            rb.update(win, **bad)
    with pytest.raises(ValueError):
        build_ring(sources, capacity, *RINGS[capacity]).update(win, v=v)           # another ring's window


@pytest.mark.parametrize("appended", [9, 45])
def test_a_sample_appended_over_since_the_gather_is_left_alone(sources, appended):
    """Capacity 37, a window of 20 that starts five slots before the next append's first: 9 appended samples go over nine
    slots of the window, 45 lap the ring and go over all of it."""
    capacity, n = 37, 20
    rb = build_ring(sources, capacity, *RINGS[capacity])
    written0 = sum(RINGS[capacity])
    win = rb.gather(n, (written0 - 5) % capacity)
    extra = random_play_batch(64, 99)
    rb.add(extra, length=first_samples(extra, appended))
    written, buf, arrays = image(rb)
    assert written == written0 + appended
    after_append = buf.copy()
    pi, v = random_targets(n, 5)
    slot, number = win.slot.cpu().numpy(), win.number.cpu().numpy()
    want = M.update(arrays, written, capacity, slot, number, words(pi, np.uint64).reshape(n, 36), words(v, np.uint32))
    stale = np.array([M.holder(int(s), written, capacity) != int(w) for s, w in zip(slot, number)])
    if appended == 9:
        assert stale.sum() == 9 and stale[5:14].all()         # both kinds occur, as the model says
        assert want.any() and not want[stale].any()
    else:
        assert stale.all() and not want.any() and np.array_equal(buf, after_append)
    got = rb.update(win, pi=pi, v=v)
    assert np.array_equal(got.cpu().numpy(), want != 0)
    assert np.array_equal(rb.buffer.cpu().numpy(), buf)       # the stale slots keep the appended bytes, the rest are refreshed


# ---------------------------------------------------------------- Reanalyser, end to end
CAPACITY, N = 500, 48


@pytest.fixture(scope="module")
def net():
    return tree_harness.net(torch.float32)


def selfplay(net, G=64, **kw):
    return SelfPlay(G, n_rollouts=8, net=net, leaf_eval="value", value_targets=(1.0, -1.0), seed=5, device=DEV, **kw)


def states_of(P, Q):
    n = len(P)
    stride = (n + 63) // 64 * 64
    st = torch.zeros(2 * stride, dtype=torch.int64, device=P.device)
    st[:n], st[stride:stride + n] = P, Q
    return VecEnv.from_state(st.view(torch.uint8), n)


def composed(rb, sp, slots, seed):
    """The route a caller had before: the slots' states as a VecEnv, a fresh TreeSearch with sp's settings, contemplate,
    the record into a fresh batch.  Returns (the batch, the tree)."""
    v = rb.views()
    idx = torch.as_tensor(slots, device=DEV).to(torch.int64)
    env = states_of(v["P"][idx], v["Q"][idx])
    n = len(idx)
    tree = TreeSearch(n, capacity=2 * sp.n_rollouts + 2, c_puct=sp.c_puct, net=sp.net, seed=seed, device=DEV,
                      leaf_eval=sp.leaf_eval, root_policy=sp.root_policy, exact_from=sp.exact_from, prove=sp.prove)
    tree.reset(env)
    tree.contemplate(sp.n_rollouts)
    rec = selfplay(sp.net, G=n, root_policy=sp.root_policy, exact_from=sp.exact_from, exact_targets=sp.exact_targets)
    batch = rec.new_batch()
    rec.record(tree, 0, batch)
    return batch, tree


@pytest.mark.parametrize("root_policy", ["puct", "gumbel"])
def test_a_run_is_the_composed_route_and_touches_nothing_else(sources, net, root_policy):
    sp = selfplay(net, root_policy=root_policy)
    rb = ReplayBuffer(CAPACITY, device=DEV, seed=SEED)
    played = sp.play()
    rb.add(played)
    rb.add(sources[1])
    assert int(rb.views()["written"].item()) > CAPACITY       # wrapped, and both sources are held
    ra = Reanalyser(sp, rb, N, seed=3)
    assert ra.tree.capacity == 2 * 8 + 2 and ra.env.num_envs == N and ra.batch.num_games == N
    seeds = []
    for k, start in enumerate((CAPACITY - 10, None)):         # the first window crosses the wrap
        written, buf, arrays = image(rb)
        stats = ra.run(start)
        assert ra.runs == k + 1 and ra.tree.seed == ra.tree_seed(k)
        seeds.append(ra.tree.seed)
        slot = stats.slot.cpu().numpy()
        assert stats.exact is None and (slot >= 0).all() and len(set(slot.tolist())) == N
        if start is not None:
            assert slot.tolist() == [(start + i) % CAPACITY for i in range(N)]
        batch, _ = composed(rb, sp, slot, ra.tree_seed(k))
        pi = words(batch.pi[0], np.uint64).reshape(N, 36)
        want = M.update(arrays, written, CAPACITY, slot, np.array([M.holder(int(s), written, CAPACITY) for s in slot]), pi, None)
        assert np.array_equal(stats.updated.cpu().numpy(), want != 0)
        assert want.sum() >= 8 and not want.all()             # refreshed samples, and terminal rows left alone
        assert np.array_equal(rb.buffer.cpu().numpy(), buf)   # the refreshed pi rows, and every other byte as before
        fresh = rb.views()["pi"][torch.as_tensor(slot[want != 0], device=DEV).to(torch.int64)]
        assert torch.allclose(fresh.sum(1), torch.ones_like(fresh.sum(1)), atol=1e-9) and bool((fresh >= 0).all())
    assert seeds[0] != seeds[1]                               # a second run searches with another seed


def late_positions(rb):
    """Slots of a ring that hold a position with eight moves played that is not over, under a stored done byte of 0."""
    v = rb.views()
    F = min(int(v["written"].item()), rb.capacity)
    env = states_of(v["P"][:F], v["Q"][:F])
    moves = env.export_boards()["n_moves"].to(torch.int64)
    live = v["P"][:F] >= 0                                    # the done bit is bit 63 of plane P
    return torch.nonzero((moves == 8) & live & (v["done"][:F] == 0))[:, 0], env


@pytest.fixture(scope="module")
def late_ring():
    rb = ReplayBuffer(2000, device=DEV, seed=SEED)
    rb.add(random_play_batch(128, 21, full=True))
    assert int(rb.views()["written"].item()) == 1280
    return rb


def test_value_mix_one_writes_the_movers_exact_value_at_eight_moves(late_ring, net):
    """value_mix = 1 with exact_from = 8 on positions with eight moves played.  The tree's child of a collapse is one
    outcome of the coin, not the solver's mean over both (README: W / N equals the solver's q for every action that is no
    collapse), so the written v is held to sum N Q / sum N of root_stats() everywhere, and to the solver's q and value —
    which pins the sign — on the positions whose visited actions are no collapses."""
    rb = late_ring
    sp = selfplay(net, exact_from=8)
    late, env = late_positions(rb)
    assert len(late) >= 4
    solved = env.solve(min_ply=8)
    n = 1280
    ra = Reanalyser(sp, rb, n, value_mix=1.0, seed=1)
    written, buf, arrays = image(rb)
    stats = ra.run(0)
    assert stats.slot.tolist() == list(range(n)) and bool(stats.updated[late].all())
    got = rb.views()["v"]
    # the written v is sum N Q / sum N over the root's actions, the same search's root_stats()
    _, tree = composed(rb, sp, list(range(n)), ra.tree_seed(0))
    st = tree.root_stats()
    N_, Q_ = st["N"][late].double(), st["Q"][late]
    q = solved.q[late].double()
    visited = N_ > 0
    assert bool(visited.any(1).all()) and bool(torch.isfinite(q[visited]).all())
    model = (torch.where(visited, N_ * Q_, torch.zeros_like(q)).sum(1) / N_.sum(1)).float()
    assert torch.equal(got[late].view(torch.int32), model.view(torch.int32))
    # The sign.  Every child of these roots is terminal or solved, so Q of an action that is no collapse is the solver's q
    # (a collapse's child is one outcome of the coin, the solver's q its mean): where no visited action is a collapse the
    # written v is sum N q / sum N with the solver's q, the mover's, and not all of those are zero
    clean = torch.where(visited, Q_ == q, torch.ones_like(visited)).all(1)
    assert int(clean.sum()) >= 4 and bool((q[clean][visited[clean]] != 0).any())
    exact = (torch.where(visited, N_ * q, torch.zeros_like(q)).sum(1) / N_.sum(1)).float()
    assert torch.equal(got[late][clean].view(torch.int32), exact[clean].view(torch.int32))
    # and where one action is legal, or all legal actions are worth the same, that is the position's exact value
    value = solved.value[late]
    same = clean & torch.where(torch.isfinite(q), q, value.double()[:, None]).eq(value.double()[:, None]).all(1)
    assert torch.equal(got[late][same].view(torch.int32), value[same].view(torch.int32))
    # pi was refreshed too; v changed nowhere but in the updated slots
    keep = ~stats.updated
    assert torch.equal(got[:n][keep].view(torch.int32), torch.as_tensor(arrays["v"][:n].view(np.int32), device=DEV)[keep])


def test_exact_targets_relabel_the_late_rows_whatever_the_mix(late_ring, net):
    rb = late_ring
    sp = selfplay(net, exact_targets=8)
    late, env = late_positions(rb)
    assert len(late) >= 4
    n = 1280
    ra = Reanalyser(sp, rb, n, value_mix=0.5, seed=2)
    written, buf, arrays = image(rb)
    stats = ra.run(0)
    batch, tree = composed(rb, sp, list(range(n)), ra.tree_seed(0))
    exact = batch.exact_targets(8, True)[0].bool()            # SelfPlayBatch.exact_targets' own, on the same states
    assert torch.equal(stats.exact, exact) and bool(exact[late].all())
    both = exact & stats.updated
    assert int(both.sum()) >= 4
    v = rb.views()
    assert torch.equal(v["pi"][:n][both].view(torch.int64), batch.pi[0][both].view(torch.int64))
    assert torch.equal(v["v"][:n][both].view(torch.int32), batch.v[0][both].view(torch.int32))
    assert torch.equal(v["v"][late].view(torch.int32), env.solve(min_ply=8).value[late].view(torch.int32))
    # the other refreshed rows carry the mix of the stored and the searched value
    st = tree.root_stats()
    N_ = st["N"].double()
    searched = torch.where(N_ > 0, N_ * st["Q"], torch.zeros_like(N_)).sum(1) / N_.sum(1).clamp(min=1.0)
    old = torch.as_tensor(arrays["v"][:n].view(np.float32), device=DEV)
    mixed = torch.where(N_.sum(1) > 0, 0.5 * old.double() + 0.5 * searched, old.double()).float()
    rest = stats.updated & ~exact
    assert int(rest.sum()) >= 4
    assert torch.equal(v["v"][:n][rest].view(torch.int32), mixed[rest].view(torch.int32))


def test_refusals(sources, net):
    rb = build_ring(sources, 300, *RINGS[300])
    sp = selfplay(net)
    reference_targets = SelfPlay(64, n_rollouts=8, net=net, leaf_eval="value", value_targets=(1.0, 0.0), device=DEV)
    with pytest.raises(ValueError):
        Reanalyser(reference_targets, rb, N, value_mix=0.5)
    Reanalyser(reference_targets, rb, N)                      # without a mix the reference's targets are fine
    for mix in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            Reanalyser(sp, rb, N, value_mix=mix)
    for n in (0, -3):
        with pytest.raises(ValueError):
            Reanalyser(sp, rb, n)
    elsewhere = build_ring(sources, 300, *RINGS[300])
    elsewhere.device = torch.device("cuda", 1)                # a ring that says it lives on another device
    with pytest.raises(ValueError):
        Reanalyser(sp, elsewhere, N)
    with pytest.raises(ValueError):
        Reanalyser(sp, "ring", N)
    with pytest.raises(ValueError):
        Reanalyser("sp", rb, N)

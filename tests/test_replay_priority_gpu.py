"""Prioritised replay on the device (include/qttt_replay_priority.h, ReplayBuffer(prioritized=True)) against its integer
model (tests/priority_model.py): the table's bytes after every sync and update, and every output of the prioritised draw,
bit for bit; the rows of the drawn slots against the composed route of tests/test_replay_gpu.py.  No statistics and no
tolerance, except ReplayBuffer.weights, whose pow is torch's (one f32 ulp)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import priority_model as PM  # noqa: E402
import replay_model as RM  # noqa: E402
from test_replay_gpu import assert_minibatch, assert_ring_is_model, composed  # noqa: E402
from qtttgym_amd import ReplayBuffer, SelfPlayBatch, VecEnv, _native  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = RM.ROWS
SEED = 77
GUARD = 0xA5
FOUR_LEVELS = (1 << 24) + 257


@pytest.fixture(scope="module")
def batch():
    """64 games of reachable states (boards stepped at random to plies 0..9) with random pi / v / done and lengths 1..10."""
    G = 64
    gen = torch.Generator(device=DEV).manual_seed(5)
    env = VecEnv(G, device=DEV, seed=9)
    b = SelfPlayBatch(G, torch.device(DEV), env.state.numel())
    for t in range(ROWS):
        b.states[t].copy_(env.state)
        b.mask[t].copy_(env.encode()[1])
        env.step_random_many(1)
    b.pi.copy_(torch.rand(b.pi.shape, dtype=torch.float64, device=DEV, generator=gen))
    b.v.copy_(torch.rand(b.v.shape, device=DEV, generator=gen) * 2 - 1)
    b.done.copy_(torch.randint(0, 2, b.done.shape, device=DEV, generator=gen).to(torch.uint8))
    b.length.copy_(torch.randint(1, 11, (G,), device=DEV, generator=gen).to(torch.uint8))
    b.count = int(b.length.sum())
    assert b.count > 257
    return b


def guarded_table(rb):
    """Moves rb's (still fresh) table into the middle of a larger buffer of guard bytes; returns that buffer."""
    size = rb.priority.numel()
    big = torch.full((size + 128,), GUARD, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 64 == 0
    rb.priority = big[64:64 + size]
    rb.priority.zero_()
    return big


def assert_table(rb, table, big, what):
    img = rb.priority.cpu().numpy()
    want = table.image()
    if not np.array_equal(img, want):
        bad = np.nonzero(img != want)[0]
        raise AssertionError((what, "first differing byte", int(bad[0]), "of", len(bad)))
    assert bool((big[:64] == GUARD).all()) and bool((big[64 + len(img):] == GUARD).all()), what


def check_draw(rb, table, written, n, symmetries=None, rows=True):
    """One sample() of a prioritised ring against the model: the table after the sync, the slots, numbers, priorities and
    total of the draw, and (rows) the minibatch of those slots by the composed route."""
    draw = rb.draw
    got = rb.sample(n, symmetries)
    table.sync(written)
    slots, qs, T = table.draw(rb.seed, draw, n)
    F = min(written, rb.capacity)
    assert rb.last_index.tolist() == slots
    assert rb.last_number.tolist() == [PM.holder(s, written, rb.capacity) if s >= 0 else -1 for s in slots]
    assert (rb.last_priority.view(torch.int32).to(torch.int64) & 0xFFFFFFFF).tolist() == qs
    assert int(rb.last_total.item()) == T
    assert all(0 <= s < F for s in slots) or T == 0               # a slot past F has priority 0 and is never drawn
    if rows and T:
        k = rb.last_symmetry if symmetries is not None else torch.zeros(n, dtype=torch.uint8, device=DEV)
        if isinstance(symmetries, str):
            assert k.tolist() == RM.symmetry_stream(rb.seed, draw, n)
        assert_minibatch(got, composed(rb, rb.last_index, k))
    return got


def corner_priorities(n, seed):
    """Random priorities in (0, 8) with the quantiser's corner inputs among them."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.rand(n, generator=gen) * 8
    corners = [0.0, -1.0, float("nan"), float("inf"), 2.0 ** -17, 2.0 ** -16 * 1.5, 65536.0, 2.0 ** -16 * 2.5, 3.0e38]
    p[:min(n, len(corners))] = torch.tensor(corners[:n])
    return p.to(DEV)


# ---------------------------------------------------------------- the whole life of a table, at every level count
@pytest.mark.parametrize("capacity", [1, 255, 256, 257, 65537])
def test_table_and_draws_follow_the_model(batch, capacity):
    """Capacities 1..257 are wrapped by a single add (more than `capacity` samples between two syncs); 65 537 (three sum
    levels, a block boundary at every level) stays partly filled.  n > F wherever the ring is small: slots drawn twice."""
    rb = ReplayBuffer(capacity, device=DEV, seed=SEED, prioritized=True)
    big = guarded_table(rb)
    table = PM.Table(capacity)
    assert_table(rb, table, big, "fresh")
    written = 0
    n = 300
    for r in range(3):
        rb.add(batch)
        written += batch.count
        check_draw(rb, table, written, n, "random" if r == 1 else None)
        assert_table(rb, table, big, ("sync", r))
        index, number = rb.last_index, rb.last_number
        p = corner_priorities(n, 10 * capacity + r)
        if capacity <= 257:
            assert len(set(index.tolist())) < n                   # duplicates: the largest Q wins
        updated = rb.update_priorities(p)
        want = table.update(written, index.cpu().numpy(), number.cpu().numpy(), p.cpu().numpy())
        assert updated.dtype == torch.bool and updated.view(torch.uint8).tolist() == want.tolist() and want.all()
        assert_table(rb, table, big, ("update", r))
        assert table.pmax == PM.QMAX                               # the +inf entry
    # two syncs in a row change no byte
    rb.sync_priorities()
    before = rb.priority.clone()
    rb.sync_priorities()
    assert torch.equal(rb.priority, before)
    # a stale write-back: the draw's slots that the next add goes over keep the newcomers' pmax
    check_draw(rb, table, written, n)
    index, number = rb.last_index, rb.last_number
    rb.add(batch)
    written += batch.count
    p = torch.full((n,), 0.5, device=DEV)
    updated = rb.update_priorities(p, index, number)
    want = table.update(written, index.cpu().numpy(), number.cpu().numpy(), p.cpu().numpy())
    assert updated.view(torch.uint8).tolist() == want.tolist()
    if capacity <= 257:
        assert not want.any()                                      # every slot has been appended over
    else:
        assert want.all()                                          # the ring has not wrapped: every draw is still held
    assert_table(rb, table, big, "stale update")                   # seen is still the old `written`
    check_draw(rb, table, written, n, "random")
    assert_table(rb, table, big, "sync after the stale update")
    assert int((rb.priority_views()["q"] != 0).sum()) == min(written, capacity)


def test_four_level_table_through_sync_and_update():
    """capacity 2^24 + 257: four sum levels (65 538, 257, 2, 1 entries), driven through sync and update alone with a ring
    that is only its 64-byte header."""
    L, C = _native.lib(), FOUR_LEVELS
    off, size = PM.layout(C)
    assert len(off) == 5 and PM.level_sizes(C) == [C, 65538, 257, 2, 1]
    header = torch.zeros(8, dtype=torch.int64, device=DEV)
    big = torch.full((size + 128,), GUARD, dtype=torch.uint8, device=DEV)
    tab = big[64:64 + size]
    tab.zero_()
    table = PM.Table(C)
    stream = torch.cuda.current_stream().cuda_stream

    def check(what):
        img = tab.cpu().numpy()
        assert np.array_equal(img, table.image()), what
        assert bool((big[:64] == GUARD).all()) and bool((big[64 + size:] == GUARD).all())

    written = C - 5                                               # the last five slots hold nothing yet
    header[0] = written
    assert L.qttt_replay_priority_sync(header.data_ptr(), tab.data_ptr(), C, stream) == 0
    table.sync(written)
    check("sync")
    slots = [0, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, C - 6, C - 5, C - 1, 256, 256]
    slot = torch.tensor(slots, dtype=torch.int32, device=DEV)
    number = slot.to(torch.int64)
    p = torch.tensor([3.0, 0.0, 7.5, float("inf"), 2.0, 1.0, 9.0, 4.0, 4.0, 4.0, 11.0, 8.0], device=DEV)
    updated = torch.full((len(slots) + 4,), GUARD, dtype=torch.uint8, device=DEV)
    assert L.qttt_replay_priority_update(header.data_ptr(), tab.data_ptr(), C, len(slots), slot.data_ptr(), number.data_ptr(),
                                         p.data_ptr(), updated.data_ptr(), stream) == 0
    want = table.update(written, slot.cpu().numpy(), number.cpu().numpy(), p.cpu().numpy())
    assert want.tolist() == [1] * 8 + [0, 0] + [1, 1]              # slots C - 5 and C - 1 hold no sample
    assert updated.tolist() == want.tolist() + [GUARD] * 4
    assert table.q[256] == 11 * PM.ONE
    check("update")
    written = 2 * C + 3                                           # wrapped: every slot is new, at pmax = 2^32 - 1
    header[0] = written
    assert L.qttt_replay_priority_sync(header.data_ptr(), tab.data_ptr(), C, stream) == 0
    table.sync(written)
    assert table.total() == C * PM.QMAX > 1 << 55
    check("second sync")


# ---------------------------------------------------------------- draws at the edges of the arithmetic
def small_ring(batch, capacity, held):
    """A prioritised ring that holds the first `held` samples of game 0."""
    rb = ReplayBuffer(capacity, device=DEV, seed=SEED, prioritized=True)
    length = torch.zeros_like(batch.length)
    length[0] = held
    assert int(batch.length[0]) >= 0
    rb.add(batch, length=length)
    return rb


def test_every_draw_on_a_prefix_boundary(batch):
    """Five slots at priority 1 (2^-16): T = 5 and every t in 0..4 is itself a running sum."""
    rb = small_ring(batch, 300, 5)
    big = guarded_table(rb)
    table = PM.Table(300)
    check_draw(rb, table, 5, 64)
    rb.update_priorities(torch.full((64,), 2.0 ** -16, device=DEV))
    table.update(5, rb.last_index.cpu().numpy(), rb.last_number.cpu().numpy(), np.full(64, 2.0 ** -16, np.float32))
    assert table.q[:5].tolist() == [1] * 5 and table.total() == 5
    check_draw(rb, table, 5, 300)
    assert_table(rb, table, big, "ones")
    assert sorted(set(rb.last_index.tolist())) == [0, 1, 2, 3, 4]


def test_sums_past_forty_bits(batch):
    """257 slots at 2^32 - 1 among slots at 1: the level-1 sums exceed 2^40, and a slot at 1 is drawn next to never —
    the draw must still be the model's."""
    rb = ReplayBuffer(700, device=DEV, seed=SEED, prioritized=True)
    big = guarded_table(rb)
    table = PM.Table(700)
    rb.add(batch)
    written = batch.count
    F = min(written, 700)
    assert F >= 258
    rb.sync_priorities()
    table.sync(written)
    slot = torch.arange(F, dtype=torch.int32, device=DEV)
    number = torch.tensor([PM.holder(s, written, 700) for s in range(F)], dtype=torch.int64, device=DEV)
    p = torch.zeros(F, device=DEV)
    p[torch.randperm(F, generator=torch.Generator().manual_seed(1))[:257].to(DEV)] = float("inf")
    assert bool(rb.update_priorities(p, slot, number).all())
    table.update(written, slot.cpu().numpy(), number.cpu().numpy(), p.cpu().numpy())
    assert table.total() == 257 * PM.QMAX + (F - 257) > 1 << 40
    assert_table(rb, table, big, "mixed")
    check_draw(rb, table, written, 1025, "random")
    assert set(rb.last_priority.view(torch.int32).tolist()) == {-1}  # 2^32 - 1 as i32


def test_nothing_to_draw_from_is_the_empty_ring(batch):
    rb = ReplayBuffer(64, device=DEV, seed=SEED, prioritized=True)
    rb.add(batch, length=torch.zeros_like(batch.length))           # an add of games without rows: written stays 0
    got = check_draw(rb, PM.Table(64), 0, 33, "random")
    assert all(not bool(t.view(-1).view(torch.uint8).any()) for t in got)
    assert rb.last_index.tolist() == [-1] * 33 == rb.last_number.tolist() and int(rb.last_total.item()) == 0
    assert not bool(rb.last_symmetry.any())


# ---------------------------------------------------------------- beside the uniform ring
@pytest.mark.parametrize("symmetries", [None, "random"])
def test_equal_priorities_are_the_uniform_sample(batch, symmetries):
    a = ReplayBuffer(500, device=DEV, seed=SEED, prioritized=True)
    b = ReplayBuffer(500, device=DEV, seed=SEED)
    for rb in (a, b):
        rb.add(batch)
        rb.add(batch)
    assert torch.equal(a.buffer, b.buffer)                         # the ring's bytes do not know about the table
    for n in (1, 65, 257):
        x, y = a.sample(n, symmetries), b.sample(n, symmetries)
        assert torch.equal(a.last_index, b.last_index) and torch.equal(a.last_symmetry, b.last_symmetry)
        for s, t in zip(x, y):
            assert torch.equal(s.view(-1).view(torch.uint8), t.view(-1).view(torch.uint8))


def test_an_unprioritised_ring_is_what_it_was(batch):
    rb, model = ReplayBuffer(300, device=DEV, seed=SEED), RM.Ring(300)
    for r in range(2):
        rb.add(batch)
        model.append(*RM.batch_arrays(batch))
        assert_ring_is_model(rb, model, r)
    assert rb.buffer.numel() == RM.layout(300)[1]
    got = rb.sample(257, "random")
    assert rb.last_index.tolist() == RM.slot_stream(SEED, 0, 257, 300)
    assert rb.last_symmetry.tolist() == RM.symmetry_stream(SEED, 0, 257)
    assert_minibatch(got, composed(rb, rb.last_index, rb.last_symmetry))
    assert rb.last_number is None and rb.last_priority is None and rb.last_total is None
    for call in (lambda: rb.weights(1.0), lambda: rb.update_priorities(torch.ones(257, device=DEV)), rb.sync_priorities):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------- guard bytes behind every output
def test_outputs_end_where_they_should(batch):
    rb = ReplayBuffer(500, device=DEV, seed=SEED, prioritized=True)
    rb.add(batch)
    rb.sync_priorities()
    n = 65
    sizes = {"s": 720 * n, "pi": 288 * n, "mask": 36 * n, "v": 4 * n, "done": n, "index": 4 * n, "sym": n, "number": 8 * n,
             "q": 4 * n, "total": 8}
    bufs = {k: torch.full((b + 64,), GUARD, dtype=torch.uint8, device=DEV) for k, b in sizes.items()}
    rb._call("qttt_replay_sample_prioritized", rb.buffer.data_ptr(), rb.priority.data_ptr(), rb.capacity, n, rb.seed, 3, 0, 1,
             *[bufs[k].data_ptr() for k in sizes])
    table = PM.Table(500)
    table.sync(batch.count)
    slots, qs, T = table.draw(rb.seed, 3, n)
    for k, b in sizes.items():
        assert bool((bufs[k][b:] == GUARD).all()), k
    assert bufs["index"][:4 * n].view(torch.int32).tolist() == slots
    assert bufs["q"][:4 * n].view(torch.int32).tolist() == qs and bufs["total"][:8].view(torch.int64).item() == T
    assert bufs["number"][:8 * n].view(torch.int64).tolist() == [PM.holder(s, batch.count, 500) for s in slots]
    k = bufs["sym"][:n]
    assert k.tolist() == RM.symmetry_stream(rb.seed, 3, n)
    got = (bufs["s"][:720 * n].view(torch.float32).view(n, 18, 10), bufs["pi"][:288 * n].view(torch.float64).view(n, 36),
           bufs["mask"][:36 * n].view(torch.bool).view(n, 36), bufs["v"][:4 * n].view(torch.float32),
           bufs["done"][:n].view(torch.bool))
    assert_minibatch(got, composed(rb, bufs["index"][:4 * n].view(torch.int32), k))


# ---------------------------------------------------------------- weights
def test_weights_are_the_model(batch):
    rb = ReplayBuffer(500, device=DEV, seed=SEED, prioritized=True)
    rb.add(batch)
    rb.sample(257)
    w = rb.weights(0.7)
    assert w.dtype == torch.float32 and bool((w == 1.0).all())      # a uniform table: every weight is exactly 1
    rb.update_priorities(torch.rand(257, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)) * 4 + 0.01)
    rb.sample(257)
    q = (rb.last_priority.view(torch.int32).to(torch.int64) & 0xFFFFFFFF).cpu().numpy()
    F = min(batch.count, 500)
    for beta in (0.4, 1.0):
        want = PM.weights(q, int(rb.last_total.item()), F, beta)
        got = rb.weights(beta).cpu().numpy()
        assert got.max() == 1.0 and np.all(np.abs(got - want) <= 2.0 ** -23 * want)      # one f32 ulp: torch's pow, not numpy's
    assert len(set(q.tolist())) > 100

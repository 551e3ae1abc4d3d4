"""The replay ring on the device (include/qttt_replay.h, qtttgym_amd.ReplayBuffer) against its numpy model
(tests/replay_model.py), against SelfPlayBatch.flat() where no wrap occurs, and the sampled minibatch against the
composed route: gather the drawn slots, VecEnv.transformed(sym).encode(), torch scatter of pi / mask by tau.  Everything
is compared bit for bit, floats as words."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_model as M  # noqa: E402
from qtttgym_amd import ReplayBuffer, SelfPlay, SelfPlayBatch, VecEnv, _native, symmetry  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = M.ROWS
# QTTT_REPLAY_SCAN_BLOCK = 256 games per workgroup of a scan level: 1..256 games are one level, 257 (two workgroups, then
# a level of their two totals) are two, and 65 537 are three (257 totals need two workgroups of their own)
THREE_LEVEL_GAMES = 65537


def synthetic_batch(G, seed, sparse=False):
    """A SelfPlayBatch of random bytes: every field the append moves, NaNs and payloads included.  length is 0..13 (11..13
    pin the clamp to 10); sparse: most games have no rows at all."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    b = SelfPlayBatch(G, torch.device(DEV), _native.lib().qttt_state_bytes(G))
    for f in ("states", "pi", "mask", "done", "v"):
        raw = getattr(b, f).view(-1).view(torch.uint8)
        raw.copy_(torch.randint(0, 256, (raw.numel(),), dtype=torch.uint8, device=DEV, generator=gen))
    b.length.copy_(torch.randint(0, 14, (G,), device=DEV, generator=gen).to(torch.uint8))
    if sparse:
        keep = torch.randint(0, 16, (G,), device=DEV, generator=gen) == 0
        keep[0] = keep[G - 1] = keep[255] = keep[256] = True
        b.length.mul_(keep.to(torch.uint8))
        b.length[0] = 12
    b.length[G - 1] = max(int(b.length[G - 1]), 10) if G > 1 else 10
    b.pi[0, 0].view(torch.int64).fill_(0x7FF8000000000123)              # a NaN row with a payload (row 0 of game 0)
    b.length[0] = max(int(b.length[0]), 1)
    return b


def ring_arrays(rb):
    v = rb.views()
    out = {k: v[k].cpu().numpy() for k in ("P", "Q", "mask", "done")}
    out["pi"] = v["pi"].view(torch.int64).cpu().numpy()
    out["v"] = v["v"].view(torch.int32).cpu().numpy()
    return int(v["written"].item()), out


def assert_ring_is_model(rb, model, what):
    written, got = ring_arrays(rb)
    assert written == model.written, what
    for k, a in got.items():
        want = getattr(model, k)
        assert np.array_equal(a.view(want.dtype), want), (what, k)


def sample_count(batch):
    return int(batch.length.clamp(max=ROWS).sum())


def states_of(P, Q):
    """n packed boards from their two words (int64 tensors) as a VecEnv."""
    n = len(P)
    stride = (n + 63) // 64 * 64
    st = torch.zeros(2 * stride, dtype=torch.int64, device=P.device)
    st[:n], st[stride:stride + n] = P, Q
    return VecEnv.from_state(st.view(torch.uint8), n)


# ---------------------------------------------------------------- append
@pytest.mark.parametrize("capacity", ["larger", "equal", 37, 7])
@pytest.mark.parametrize("games", [1, 63, 64, 65, 257])
def test_append_is_the_model_after_each_of_three_appends(games, capacity):
    batches = [synthetic_batch(games, 100 * games + r) for r in range(3)]
    counts = [sample_count(b) for b in batches]
    if games >= 63:
        assert min(counts) >= 25                              # capacity 7: the skip rule, n > capacity by far
    cap = {"larger": sum(counts) + 5, "equal": counts[0]}.get(capacity, capacity)
    rb, model = ReplayBuffer(cap, device=DEV), M.Ring(cap)
    assert rb.size() == 0
    for r, b in enumerate(batches):
        rb.add(b)
        assert model.append(*M.batch_arrays(b)) == counts[r]
        assert_ring_is_model(rb, model, (games, capacity, r))
        assert rb.size() == model.filled
    if capacity != "larger":
        return
    # no wrap: the ring's first samples are the batches' flat() rows, in flat()'s order
    v = rb.views()
    at = 0
    for b, n in zip(batches, counts):
        s, pi, mask, vt, done = b.flat()
        sl = slice(at, at + n)
        assert len(s) == n
        assert torch.equal(states_of(v["P"][sl], v["Q"][sl]).encode(with_mask=False).view(torch.int32), s.view(torch.int32))
        assert torch.equal(v["pi"][sl].view(torch.int64), pi.view(torch.int64))
        assert torch.equal(((v["mask"][sl][:, None] >> torch.arange(36, device=DEV)) & 1).bool(), mask)
        assert torch.equal(v["v"][sl].view(torch.int32), vt.view(torch.int32))
        assert torch.equal(v["done"][sl] != 0, done)
        at += n
    assert at == int(v["written"].item())


def test_append_with_three_levels_of_the_scan():
    """65 537 games: the level of 257 block totals is itself scanned by two workgroups.  Most games are empty, so that the
    batch stays small; the third append wraps."""
    G = THREE_LEVEL_GAMES
    batches = [synthetic_batch(G, 7 + r, sparse=True) for r in range(3)]
    counts = [sample_count(b) for b in batches]
    assert min(counts) > 10000
    cap = counts[0] + counts[1] + counts[2] // 2
    rb, model = ReplayBuffer(cap, device=DEV), M.Ring(cap)
    for r, b in enumerate(batches):
        rb.add(b)
        assert model.append(*M.batch_arrays(b)) == counts[r]
        assert_ring_is_model(rb, model, r)
    assert model.written > cap


def test_add_checks_the_batch_and_leaves_it_unchanged():
    b = synthetic_batch(65, 5)
    before = {f: getattr(b, f).clone() for f in SelfPlayBatch._FIELDS}
    rb = ReplayBuffer(100, device=DEV)
    rb.add(b)
    for f, t in before.items():
        assert torch.equal(getattr(b, f).view(-1).view(torch.uint8), t.view(-1).view(torch.uint8)), f
    b.v = b.v.double()
    with pytest.raises(ValueError):
        rb.add(b)
    empty = SelfPlayBatch(0, torch.device(DEV), 0)
    rb.add(empty)                                             # no games: nothing happens
    assert rb.size() == 100 and rb.adds == 1


# ---------------------------------------------------------------- sample
SEED = 2026


CAPACITY = 500


def filled_ring(batches, seed):
    rb = ReplayBuffer(CAPACITY, device=DEV, seed=seed)
    for b in batches:
        rb.add(b)
    return rb


@pytest.fixture(scope="module")
def filled():
    """A wrapped ring of reachable states that holds BOTH sources: one real self-play of 64 games at 8 rollouts, appended
    first, then boards stepped at random to plies 0..9 with random pi / v / done.  The second batch is smaller than the
    ring, so all of it is held, beside the last of the self-play samples.  rb.batches are the two batches, rb.from_random
    bool[capacity] says which slots hold the second one's samples."""
    G = 64
    gen = torch.Generator(device=DEV).manual_seed(11)
    env = VecEnv(G, device=DEV, seed=3)
    b = SelfPlayBatch(G, torch.device(DEV), env.state.numel())
    for t in range(ROWS):
        b.states[t].copy_(env.state)
        b.mask[t].copy_(env.encode()[1])
        env.step_random_many(1)
    b.pi.copy_(torch.rand(b.pi.shape, dtype=torch.float64, device=DEV, generator=gen))
    b.v.copy_(torch.rand(b.v.shape, device=DEV, generator=gen) * 2 - 1)
    b.done.copy_(torch.randint(0, 2, b.done.shape, device=DEV, generator=gen).to(torch.uint8))
    b.length.copy_(torch.randint(1, 11, (G,), device=DEV, generator=gen).to(torch.uint8))
    played = SelfPlay(G, n_rollouts=8, num_simulations=2, seed=5, device=DEV).play()
    rb = filled_ring((played, b), SEED)
    rb.batches = (played, b)
    n_played, n_random = sample_count(played), sample_count(b)
    written = int(rb.views()["written"].item())
    assert written == n_played + n_random > CAPACITY == rb.size()                    # wrapped: F = capacity
    assert 100 <= n_random <= CAPACITY - 100                                         # both sources are held, 100 samples at least
    slots = (n_played + torch.arange(n_random, device=DEV)) % CAPACITY
    rb.from_random = torch.zeros(CAPACITY, dtype=torch.bool, device=DEV)
    rb.from_random[slots] = True
    # and the ring's bytes say so: the second batch's samples in flat()'s order, and before them the self-play's last ones
    v = rb.views()
    assert torch.equal(v["pi"][slots].view(torch.int64), b.flat()[1].view(torch.int64))
    assert (b.flat()[1] != 0).all()                                                  # random pi rows: all 36 entries non-zero
    keep = CAPACITY - n_random
    tail = (n_played - keep + torch.arange(keep, device=DEV)) % CAPACITY
    assert torch.equal(v["pi"][tail].view(torch.int64), played.flat()[1][-keep:].view(torch.int64))
    assert not rb.from_random[tail].any()
    return rb


def composed(rb, index, k):
    """The minibatch of slots `index` under symmetries k (u8, a value past 7: as stored) by the calls a caller had before:
    gather, transformed().encode(), scatter by tau."""
    v = rb.views()
    idx = index.to(torch.int64)
    s = states_of(v["P"][idx], v["Q"][idx]).transformed(k).encode(with_mask=False)
    keff = torch.where(k > 7, torch.zeros_like(k), k).to(torch.int64)
    tau = torch.tensor(symmetry.ACTIONS, dtype=torch.int64, device=idx.device)[keff]          # [n, 36]
    pi = torch.zeros((len(idx), 36), dtype=torch.int64, device=idx.device).scatter_(1, tau, v["pi"].view(torch.int64)[idx])
    bits = (v["mask"][idx][:, None] >> torch.arange(36, device=idx.device)) & 1
    mask = torch.zeros_like(bits).scatter_(1, tau, bits).bool()
    return s, pi, mask, v["v"].view(torch.int32)[idx], v["done"][idx] != 0, keff.to(torch.uint8)


def assert_minibatch(got, want):
    s, pi, mask, v, done = got
    assert s.dtype == torch.float32 and pi.dtype == torch.float64 and mask.dtype == torch.bool and done.dtype == torch.bool
    assert torch.equal(s.view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(pi.view(torch.int64), want[1])
    assert torch.equal(mask, want[2]) and torch.equal(mask.view(torch.uint8), want[2].to(torch.uint8))    # 0 / 1 bytes
    assert torch.equal(v.view(torch.int32), want[3])
    assert torch.equal(done, want[4]) and torch.equal(done.view(torch.uint8), want[4].to(torch.uint8))


@pytest.mark.parametrize("form", ["none", "given", "random"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sample_is_the_composed_route(filled, n, form):
    rb = filled
    draw = rb.draw
    given = (torch.arange(n, device=DEV) * 7 % 10).to(torch.uint8) if form == "given" else None     # every k, and 8, 9
    if form == "given" and n >= 63:
        assert set(given.tolist()) == set(range(10))
    got = rb.sample(n, {"none": None, "given": given, "random": "random"}[form])
    assert rb.draw == draw + 1
    assert rb.last_index.dtype == torch.int32 and rb.last_symmetry.dtype == torch.uint8
    assert rb.last_index.tolist() == M.slot_stream(SEED, draw, n, CAPACITY)                       # the model's stream, exactly
    k = {"none": torch.zeros(n, dtype=torch.uint8, device=DEV), "given": given,
         "random": torch.tensor(M.symmetry_stream(SEED, draw, n), dtype=torch.uint8, device=DEV)}[form]
    want = composed(rb, rb.last_index, k)
    assert torch.equal(rb.last_symmetry, want[5])
    assert_minibatch(got, want)
    if n >= 63:                                               # the minibatch draws from both sources of the ring
        drawn = rb.from_random[rb.last_index.to(torch.int64)]
        assert bool(drawn.any()) and not bool(drawn.all())


def test_the_permutation_is_the_tables_and_the_draw_is_reproducible(filled):
    rb = filled
    twin = filled_ring(rb.batches, SEED)
    assert torch.equal(twin.buffer, rb.buffer)
    n, draw = 200, rb.draw
    a = rb.sample(n, "random")
    ia, ka = rb.last_index.clone(), rb.last_symmetry.clone()
    b = rb.sample(n, "random")
    assert not torch.equal(ia, rb.last_index) and not torch.equal(ka, rb.last_symmetry)     # two calls: different draws
    twin.draw = draw
    c = twin.sample(n, "random")                                                            # the same (seed, draw)
    assert torch.equal(twin.last_index, ia) and torch.equal(twin.last_symmetry, ka)
    for x, y in zip(a, c):
        assert torch.equal(x.view(-1).view(torch.uint8), y.view(-1).view(torch.uint8))
    assert not torch.equal(a[0], b[0])
    # the same draw without symmetries, permuted by the model's tables, is the draw with them
    twin.draw = draw
    plain = twin.sample(n)
    assert torch.equal(twin.last_index, ia) and not bool(twin.last_symmetry.any())
    s2, pi2, mask2 = M.permute(plain[0].cpu().numpy(), plain[1].cpu().numpy().view(np.uint64), plain[2].cpu().numpy(),
                               ka.tolist())
    assert np.array_equal(s2.view(np.uint32), a[0].cpu().numpy().view(np.uint32))
    assert np.array_equal(pi2, a[1].cpu().numpy().view(np.uint64)) and np.array_equal(mask2, a[2].cpu().numpy())
    assert torch.equal(plain[3], a[3]) and torch.equal(plain[4], a[4])
    # another seed draws other slots
    other = filled_ring(rb.batches, SEED + 1)
    other.draw = draw
    other.sample(n, "random")
    assert not torch.equal(other.last_index, ia)


def test_sample_writes_into_the_tensors_of_an_earlier_call_and_checks_its_arguments(filled):
    rb = filled
    out = rb.sample(65)
    ptrs = [t.data_ptr() for t in out]
    again = rb.sample(65, "random", out=out)
    assert [t.data_ptr() for t in again] == ptrs
    assert_minibatch(again, composed(rb, rb.last_index, rb.last_symmetry))
    draw = rb.draw
    for bad in (dict(n=-1), dict(n=4, symmetries="all"), dict(n=4, symmetries=torch.zeros(5, dtype=torch.uint8, device=DEV)),
                dict(n=4, symmetries=torch.zeros(4, dtype=torch.int64, device=DEV)), dict(n=4, out=out), dict(n=65, out=out[:4])):
        with pytest.raises(ValueError):
            rb.sample(**bad)
    assert rb.draw == draw                                    # a refused call draws nothing
    assert all(len(t) == 0 for t in rb.sample(0)) and rb.draw == draw + 1
    with pytest.raises(ValueError):
        ReplayBuffer(8, device=DEV).sample(1)                 # before any add


def test_an_empty_ring_through_the_c_entry_gives_zeros_and_minus_one():
    L = _native.lib()
    n, cap = 33, 8
    ring = torch.zeros(int(L.qttt_replay_bytes(cap)), dtype=torch.uint8, device=DEV)
    outs = [torch.full(shape, 0x55, dtype=torch.uint8, device=DEV)
            for shape in ((n, 720), (n, 288), (n, 36), (n, 4), (n,), (n, 4), (n,))]
    sym = torch.full((n,), 3, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        stream = torch.cuda.current_stream().cuda_stream
        rc = L.qttt_replay_sample(ring.data_ptr(), cap, n, 1, 0, sym.data_ptr(), 1, *[t.data_ptr() for t in outs], stream)
    assert rc == 0
    torch.cuda.synchronize()
    for t in outs[:5] + outs[6:]:
        assert not bool(t.any())
    assert outs[5].view(torch.int32).view(-1).tolist() == [-1] * n
    assert not bool(ring.any())                               # and the ring is read only

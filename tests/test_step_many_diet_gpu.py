"""The output-free step_fused_kernel keeps the board in a form of its own between the plies of a launch (ResidentBoard,
csrc/qttt_step_core.h: "done" as a lane mask, the high nibble of comps and the classical mask in registers of their own)
and touches the packed 16 bytes only in front of and behind its ply loop.  The other step_many tests all enter that
kernel from the empty board; here it is entered and left where an unpack / pack pair can go wrong: at every depth of a
game, with four live components, with the last ply terminating / illegal / closing a cycle, with the done bit set without
cause, and across launches from a non-empty start.

The method is test_step_many_long_runs_gpu.py's: one trajectory per case is taken launch by launch (step_raw) with the C
oracle stepping beside it; a run of step_many(fused=True) then starts from a recorded state of that trajectory
(VecEnv.from_state, same seed and step index) and must end, bit for bit, in the recorded state, reward bits and
terminated of the trajectory, and in the oracle's boards and moves.  reward / terminated are pre-filled with 7.0 / True."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "qtttgym_amd", "csrc", "qttt_step_kernels.h")) as _f:
    C = int(re.search(r"constexpr int RESIDENT_MAX_PLIES = (\d+);", _f.read()).group(1))

DEPTHS = tuple(range(1, 11))                 # single steps in front of the run: mid-game, finished and nine-move boards
PLIES = (1, 2, 3, 16, C + 1)                 # below and above the prefetch depth, one full launch plus a ply


def _spoil(acts, gen):
    """about a quarter of the pairs replaced: swapped (unsorted), both squares the same, a square out of range, or any
    pair of squares at all (occupied ones among them)"""
    n = acts.shape[0]
    kind = torch.randint(0, 16, (n,), device="cuda", generator=gen)
    rnd = torch.randint(0, 9, (n, 2), device="cuda", generator=gen).to(torch.uint8)
    far = torch.randint(9, 256, (n,), device="cuda", generator=gen).to(torch.uint8)
    out = acts.clone()
    out[kind == 0] = acts[kind == 0].flip(1)
    out[kind == 1, 1] = acts[kind == 1, 0]
    out[kind == 2, 0] = far[kind == 2]
    out[kind == 3] = rnd[kind == 3]
    return out


def _plane_p(state, n):
    """plane P of a packed state tensor as int64[n]: the done bit is its sign, n at bits 40..43, the high nibble of comps
    at 44..47, the classical mask at 54..62 (csrc/qttt_state.h)"""
    return state.view(torch.int64)[:n]


def _done(state, n):
    return _plane_p(state, n) < 0


def _moves_played(state, n):
    return (_plane_p(state, n) >> 40) & 0xF


def _classical_count(state, n):
    cl = (_plane_p(state, n) >> 54) & 0x1FF
    return sum((cl >> v) & 1 for v in range(9))


class Trajectory:
    """`total` steps taken launch by launch from the empty board, the oracle beside them (asserted equal as it goes).
    first: actions u8[k, n, 2] (and first_bits u8[k, n]) that replace the head of the recorded uniform-legal stream."""

    def __init__(self, n, auto_reset, explicit_bits, spoiled, total, first=None, first_bits=None):
        import oracle
        from qtttgym_amd import VecEnv
        self.n, self.auto_reset, self.seed = n, auto_reset, 4100 + n % 911
        gen = torch.Generator(device="cuda").manual_seed(self.seed + 29)
        rec = VecEnv(n, seed=self.seed, auto_reset=auto_reset)
        ob = oracle.OracleBoards(n)
        self.acts = torch.empty((total, n, 2), dtype=torch.uint8, device="cuda")
        self.bits = torch.randint(0, 2, (total, n), dtype=torch.uint8, device="cuda", generator=gen) if explicit_bits else None
        if first_bits is not None:
            self.bits[:first_bits.shape[0]] = first_bits
        self.states, self.outs, self.boards = [rec.state.clone()], [None], [(ob.board.copy(), ob.moves.copy())]
        for t in range(total):
            if first is not None and t < first.shape[0]:
                self.acts[t] = first[t]
            else:
                rec.sample_actions(out=self.acts[t])
                if spoiled:
                    self.acts[t] = _spoil(self.acts[t], gen)
            r, tm = rec.step_raw(self.acts[t], None if self.bits is None else self.bits[t])
            r_or, t_or = ob.step(self.acts[t].cpu().numpy(), None if self.bits is None else self.bits[t].cpu().numpy(),
                                 self.seed, t, 0, auto_reset)
            assert np.array_equal(r.cpu().numpy().view(np.uint32), r_or.view(np.uint32)), t
            assert np.array_equal(tm.cpu().numpy().astype(np.uint8), t_or), t
            self.states.append(rec.state.clone())
            self.outs.append((r.view(torch.int32).clone(), tm.clone()))
            self.boards.append((ob.board.copy(), ob.moves.copy()))

    def resume(self, k, state=None):
        """a VecEnv of its own on a copy of the state after k steps, outputs pre-filled"""
        from qtttgym_amd import VecEnv
        env = VecEnv.from_state((self.states[k] if state is None else state).clone(), self.n, seed=self.seed,
                                auto_reset=self.auto_reset)
        env.step_idx = k
        env._reward.fill_(7.0)
        env._terminated.fill_(True)
        return env

    def run(self, k, T, tag=()):
        """steps k .. k + T - 1 in one step_many from the recorded state after k steps: everything equals the recording"""
        tag = (self.n, self.auto_reset, self.bits is not None, k, T) + tuple(tag)
        many = self.resume(k)
        r, tm = many.step_many(self.acts[k:k + T], None if self.bits is None else self.bits[k:k + T], fused=True)
        assert many.step_idx == k + T, tag
        assert torch.equal(many.state, self.states[k + T]), tag
        assert torch.equal(r.view(torch.int32), self.outs[k + T][0]) and torch.equal(tm, self.outs[k + T][1]), tag
        ex = many.export_boards()
        assert np.array_equal(ex["board"].cpu().numpy(), self.boards[k + T][0]), tag
        assert np.array_equal(ex["moves"].cpu().numpy(), self.boards[k + T][1]), tag
        return many


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 65, 513])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
@pytest.mark.parametrize("spoiled", [False, True])
def test_runs_entered_at_every_depth(n, auto_reset, explicit_bits, spoiled):
    tr = Trajectory(n, auto_reset, explicit_bits, spoiled, max(DEPTHS) + max(PLIES))
    entered_done = entered_midgame = entered_nine = False
    for k in DEPTHS:
        done, played = _done(tr.states[k], n), _moves_played(tr.states[k], n)
        entered_done |= bool(done.any())
        entered_midgame |= bool((~done & (played >= 2) & (played <= 6)).any())
        entered_nine |= bool((played == 9).any())
        for T in PLIES:
            tr.run(k, T)
    assert entered_done and entered_midgame, "the depths no longer reach finished and mid-game boards"
    if n == 513 and not auto_reset and not spoiled:
        assert entered_nine, "no board of nine moves among 513 games played to the end"


# after (0,1) (2,3) (4,5) (6,7): four components, the fourth in the high nibble of comps.  Three further moves per board:
# cycles on a pair, unions (a slot is popped), a cycle through a union, square 8 joining, each with both collapse bits
FOUR_PAIRS = ((0, 1), (2, 3), (4, 5), (6, 7))
SCRIPTS = (((0, 1), (2, 3), (4, 5)), ((1, 2), (3, 4), (0, 4)), ((7, 8), (6, 8), (0, 2)),
           ((5, 6), (4, 7), (0, 1)), ((0, 8), (1, 8), (2, 3)), ((6, 7), (4, 5), (0, 2)), ((6, 7), (0, 7), (1, 6)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 513])
@pytest.mark.parametrize("auto_reset", [False, True])
def test_four_live_components_at_entry_and_at_exit(n, auto_reset):
    S = len(SCRIPTS)
    first = torch.empty((7, n, 2), dtype=torch.uint8, device="cuda")
    for t, pair in enumerate(FOUR_PAIRS):
        first[t] = torch.tensor(pair, dtype=torch.uint8, device="cuda")
    which = torch.arange(n, device="cuda") % S
    scripts = torch.tensor(SCRIPTS, dtype=torch.uint8, device="cuda")            # [S, 3, 2]
    for t in range(3):
        first[4 + t] = scripts[which, t]
    # both values of the bit for every script, and both orders of them over the three moves
    ids = torch.arange(n, device="cuda") // S
    first_bits = torch.stack([torch.zeros_like(ids)] * 4 + [ids & 1, (ids >> 1) & 1, (ids >> 2) & 1]).to(torch.uint8)
    tr = Trajectory(n, auto_reset, True, False, 7 + 9, first=first, first_bits=first_bits)
    chi = (_plane_p(tr.states[4], n) >> 44) & 0xF
    assert bool((chi != 0).all()), "the hand-over state no longer has the high nibble of comps in use"
    assert bool(((_plane_p(tr.states[2], n) >> 44) & 0xF == 0).all())
    assert bool((_classical_count(tr.states[7], n) > 0).any()), "no scripted cycle collapsed"
    tr.run(0, 4)                       # exit with four live components
    tr.run(2, 2)                       # ... entered with two
    tr.run(4, 1)                       # entry with four: the first scripted move alone,
    tr.run(4, 3)                       # the script,
    tr.run(4, 12)                      # and on into the recorded stream
    tr.run(3, 2)                       # the fourth component appears and is used within one run
    tr.run(5, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_the_last_ply_terminates_is_illegal_and_closes_a_cycle(auto_reset, explicit_bits):
    n = 513
    tr = Trajectory(n, auto_reset, explicit_bits, True, 12)
    for k, T in ((4, 3), (5, 3), (7, 1), (7, 2), (6, 3)):
        before, after = tr.states[k + T - 1], tr.states[k + T]
        live = ~_done(before, n)
        assert bool((_done(after, n) & live).any()), ("no board terminates on the last ply", k, T)
        assert bool((live & (_moves_played(after, n) == _moves_played(before, n))).any()), ("no illegal last ply", k, T)
        assert bool((live & (_classical_count(after, n) > _classical_count(before, n))).any()), ("no cycle closed", k, T)
        if k >= 7:
            assert bool(_done(tr.states[k], n).any()), ("no board done at entry", k)
        tr.run(k, T)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 513])
@pytest.mark.parametrize("k", [0, 3])
def test_a_done_bit_set_without_cause_is_kept_or_restarts_the_board(n, k):
    """bit 63 of plane P set by hand on every board (empty boards, and boards of three moves): without auto-reset the run
    and noops keep it, everything else moving as on the untouched boards; with auto-reset the board restarts on the first
    ply, as a fresh environment's does."""
    from qtttgym_amd import VecEnv
    T = 5
    for auto_reset in (False, True):
        tr = Trajectory(n, auto_reset, False, False, k + T)
        marked = tr.states[k].clone()
        _plane_p(marked, n).bitwise_or_(torch.tensor(-(1 << 63), dtype=torch.int64, device="cuda"))
        acts = tr.acts[k:k + T]
        single = tr.resume(k, marked)
        for t in range(T):
            r1, t1 = single.step_raw(acts[t])
        many = tr.resume(k, marked)
        r, tm = many.step_many(acts, fused=True)
        assert torch.equal(many.state, single.state) and torch.equal(tm, t1), (n, k, auto_reset)
        assert torch.equal(r.view(torch.int32), r1.view(torch.int32)), (n, k, auto_reset)
        if not auto_reset:
            assert bool(_done(many.state, n).all()) and bool(tm.all())
            untouched = tr.states[k + T].clone()
            _plane_p(untouched, n).bitwise_or_(torch.tensor(-(1 << 63), dtype=torch.int64, device="cuda"))
            assert torch.equal(many.state, untouched), (n, k)
            many.step_many(torch.zeros((3, n, 2), dtype=torch.uint8, device="cuda"), fused=True)      # noops: (0, 0)
            assert torch.equal(many.state, untouched), (n, k)
        else:
            fresh = VecEnv(n, seed=tr.seed, auto_reset=True)
            fresh.step_idx = k
            rf, tf = fresh.step_many(acts, fused=True)
            assert torch.equal(many.state, fresh.state), (n, k)
            assert torch.equal(r.view(torch.int32), rf.view(torch.int32)) and torch.equal(tm, tf), (n, k)
            assert bool((_moves_played(many.state, n) <= T).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 513])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_a_run_split_over_launches_from_a_non_empty_start(n, auto_reset, explicit_bits):
    """2 C + 3 plies after k single steps: two launches without outputs and one with the last ply's; what the plies keep
    outside the packed planes crosses no launch boundary"""
    tr = Trajectory(n, auto_reset, explicit_bits, True, 6 + 2 * C + 3)
    for k in (1, 6):
        tr.run(k, 2 * C + 3)

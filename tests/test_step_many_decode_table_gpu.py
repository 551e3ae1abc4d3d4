"""The output-free step_fused_kernel no longer decodes the action's two bytes with arithmetic: the sorted squares, x at
`last x`'s place and the two-square mask come from an LDS table of 256 entries indexed by the two low nibbles
(csrc/qttt_step_core.h: action_lut_entry, action_lut_read), requested while the ply before runs; an action with a bit in
either high nibble aliases some entry and is rejected by the ply's one compare.  What can go wrong is an entry, the
aliasing, the byte order, and the request's place in the run: its first ply, its last, the launch boundary.

The method is test_step_many_diet_gpu.py's (its Trajectory): a trajectory taken launch by launch (step_raw) with the C
oracle stepping beside it; step_many(fused=True) from a recorded state of it must end, bit for bit, in the recorded state,
reward bits and terminated, and in the oracle's boards and moves.  reward / terminated are pre-filled with 7.0 / True."""
import pytest
import torch

from test_step_many_diet_gpu import C, FOUR_PAIRS, Trajectory, _classical_count, _done, _moves_played, _plane_p

N_ALL = 65536                                 # one board per value of the action's 16 bits
# what every board plays in front of "every action there is", and how many of the 65 536 pairs are then legal moves
STARTS = {
    "empty": ((), 9 * 8),
    "classical": (((0, 1), (0, 1), (2, 3)), 7 * 6),          # the second move closes a cycle: squares 0 and 1 go classical
    "four_components": (FOUR_PAIRS, 9 * 8),                    # the fourth component sits in the high nibble of comps
}


def _every_action(start, auto_reset, explicit_bits):
    """the trajectory (one per case, shared by its two run lengths): the start's moves on every board, then board i plays
    the byte pair (i & 255, i >> 8), then 17 recorded uniform-legal plies"""
    prefix = STARTS[start][0]
    first = torch.empty((len(prefix) + 1, N_ALL, 2), dtype=torch.uint8, device="cuda")
    for t, pair in enumerate(prefix):
        first[t] = torch.tensor(pair, dtype=torch.uint8, device="cuda")
    i = torch.arange(N_ALL, device="cuda")
    first[len(prefix), :, 0] = (i & 255).to(torch.uint8)
    first[len(prefix), :, 1] = (i >> 8).to(torch.uint8)
    return Trajectory(N_ALL, auto_reset, explicit_bits, False, len(prefix) + 1 + 17, first=first)


@pytest.mark.gpu
@pytest.mark.parametrize("start", list(STARTS))
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_every_action_there_is(start, auto_reset, explicit_bits):
    """all 65 536 byte pairs as the FIRST ply of a run — every aliasing index, both byte orders, equal squares, occupied
    squares, out-of-range bytes in either position — followed by 2 and by 17 legal plies"""
    tr = _every_action(start, auto_reset, explicit_bits)
    k, legal_pairs = len(STARTS[start][0]), STARTS[start][1]
    before, after = tr.states[k], tr.states[k + 1]
    assert not bool(_done(before, N_ALL).any())
    if start == "classical":
        assert bool((_classical_count(before, N_ALL) == 2).all()), "the start no longer has two classical squares"
    if start == "four_components":
        assert bool((((_plane_p(before, N_ALL) >> 44) & 0xF) != 0).all()), "the start no longer uses the high nibble of comps"
    moved = _moves_played(after, N_ALL) == _moves_played(before, N_ALL) + 1
    assert int(moved.sum()) == legal_pairs, "the recording itself does not accept exactly the legal pairs"
    idx = torch.arange(N_ALL, device="cuda")
    assert not bool((moved & (((idx & 255) > 8) | ((idx >> 8) > 8))).any())
    for follow in (2, 17):
        tr.run(k, 1 + follow, tag=(start,))


N_EDGE = 64 * 3 + 5                           # three full waves and one that is partly idle
EDGE_PLIES = (1, 2, 3, 16, C + 1)             # the request in front of the loop alone; one, two requests inside it; a launch
                                              # boundary between a ply and the request made for it


@pytest.mark.gpu
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_the_look_ahead_at_the_edges_of_a_run(auto_reset, explicit_bits):
    """a spoiled stream (unsorted pairs, equal squares, out-of-range bytes, occupied squares): runs of every length at
    which the request a ply ahead meets an edge, and a run of one launch plus a ply in which the last ply of the first
    launch and the first ply of the second carry illegal (with auto-reset also terminating) actions"""
    k0 = 2
    tr = Trajectory(N_EDGE, auto_reset, explicit_bits, True, k0 + C + 1)
    for k in (1, k0, 5):
        for T in EDGE_PLIES[:-1]:
            tr.run(k, T)
    for j in (k0 + C - 1, k0 + C):            # the plies on either side of the launch boundary
        before, after = tr.states[j], tr.states[j + 1]
        took_a_move = ~_done(before, N_EDGE) if auto_reset else torch.ones(N_EDGE, dtype=torch.bool, device="cuda")
        illegal = took_a_move & (_moves_played(after, N_EDGE) == _moves_played(before, N_EDGE))
        assert bool(illegal.any()), ("no illegal action on ply", j)
        if auto_reset:
            assert bool((_done(after, N_EDGE) & ~_done(before, N_EDGE)).any()), ("no board terminates on ply", j)
    tr.run(k0, C + 1)

"""The exact endgame solver's host side (include/qttt_solve.h): what VecEnv.solve returns, and how many
boards one launch takes."""
import torch

from . import _native

# Boards per launch by min_ply, so that one kernel launch stays short on a device other people share: the worst board
# measured at that depth, one resident workgroup per board at the compiler's occupancy (5 workgroups on each of 256 CUs
# = 1 280 boards a round), a factor 2 in hand, under one second per launch (tools/solvebench.py,
# profiles/solve/solvebench.jsonl; the arithmetic: DESIGN.md §23).
#   four moves played: the largest of 256 random boards (29.8 M positions) takes 339 ms alone on a CU and 679 ms as a
#     full round of 1 280 copies: twice a full round is over a second, twice one board per CU is 0.68 s -> 256 boards;
#   five moves played: the largest (1.25 M positions) takes 29.6 ms as a full round; 1 s / (2 x 29.6 ms) = 16 rounds
#     = 20 480 boards -> 16 384, the power of two below.
# From six moves played on the largest board seen is 5.1 * 10^4 positions (4 096 boards: 1 ms) and no split is needed.
BOARDS_PER_LAUNCH = {4: 256, 5: 16384}


def default_boards_per_launch(min_ply):
    """The default of VecEnv.solve's boards_per_launch for this min_ply; None = one launch."""
    return BOARDS_PER_LAUNCH.get(int(min_ply))


class SolveResult:
    """The exact solution of N positions, as device tensors: value f32[N] (the expectimax value for the player to
    move), q f32[N, 36] (the value of each action; -inf at illegal ones), best u8[N] (the lowest optimal action; 255
    for a leaf), nodes i64[N] (the positions the full enumeration visited) and solved bool[N].  A board with fewer than
    min_ply moves played that is no leaf is skipped: solved False, value and q NaN, best 255, nodes 0."""

    __slots__ = ("value", "q", "best", "nodes", "solved")

    def __init__(self, value, q, best, nodes, solved):
        self.value, self.q, self.best, self.nodes, self.solved = value, q, best, nodes, solved

    def regret(self, action36):
        """value - q[i, action36[i]]: what playing action36[i] on board i gives away, 0 for an optimal move, +inf for an
        illegal action, NaN for a skipped board.  action36: N ind2move indices 0..35."""
        a = torch.as_tensor(action36, device=self.q.device).to(torch.int64).reshape(-1)
        if a.shape != self.value.shape:
            raise ValueError("action36 must have shape %s" % (tuple(self.value.shape),))
        if a.numel() and not bool(((a >= 0) & (a < 36)).all()):
            raise ValueError("an action is 0..35")
        return self.value - self.q.gather(1, a[:, None])[:, 0]

    def __repr__(self):
        return "SolveResult(%d boards, %d solved)" % (self.value.numel(), int(self.solved.sum()))


def check_min_ply(min_ply):
    m = int(min_ply)
    if not _native.SOLVE_MIN_PLY <= m <= _native.SOLVE_MAX_PLY:
        raise ValueError("min_ply must be in %d..%d: below four moves played one board is 10^9 positions or more"
                         % (_native.SOLVE_MIN_PLY, _native.SOLVE_MAX_PLY))
    return m

"""The board's eight symmetries restated in plain Python (include/qttt_symmetry.h), for the tests: the
group and its tables from the definition, and the image of a position's Board attributes with the qstructs order taken
by replaying the un-collapsed moves.  A plain helper module; nothing here reads the library."""
import itertools

PAIRS = tuple(itertools.combinations(range(9), 2))
INDEX = {p: a for a, p in enumerate(PAIRS)}
LINES = ((0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6))


def sigma(k):
    """sigma_k as a tuple of nine squares: a mirror first if k & 4, then k & 3 quarter turns clockwise."""
    out = []
    for v in range(9):
        r, c = divmod(v, 3)
        if k & 4:
            c = 2 - c
        for _ in range(k & 3):
            r, c = c, 2 - r
        out.append(3 * r + c)
    return tuple(out)


def tau(k):
    s = sigma(k)
    return tuple(INDEX[tuple(sorted((s[i], s[j])))] for i, j in PAIRS)


CELLS = tuple(sigma(k) for k in range(8))
ACTIONS = tuple(tau(k) for k in range(8))
# COMPOSE[a][b]: a first, then b
COMPOSE = tuple(tuple(CELLS.index(tuple(CELLS[b][CELLS[a][v]] for v in range(9))) for b in range(8)) for a in range(8))
INVERSE = tuple(COMPOSE[a].index(0) for a in range(8))


def mask_of(squares):
    return sum(1 << v for v in squares)


def map_mask(m, k):
    return sum(1 << CELLS[k][v] for v in range(9) if m >> v & 1)


def replay_qstructs(live_moves):
    """Board.update_qstructs (board.py:27-69) of moves that close no cycle, in the order given: the list of sets."""
    q = []
    for lo, hi in live_moves:
        m0 = next((i for i, s in enumerate(q) if lo in s), -1)
        m1 = next((i for i, s in enumerate(q) if hi in s), -2)
        assert m0 != m1, "a live move closes no cycle"
        if m0 >= 0 and m1 >= 0:
            q[m0] = q[m0] | q[m1]
            q.pop(m1)
        else:
            i = max(m0, m1)
            if i < 0:
                q.append(set())
                i = len(q) - 1
            q[i] |= {lo, hi}
    return q


def live_rounds(board, moves, n_moves):
    """Rounds of the moves that have not collapsed: those that stand on no square (an autofill move names one square
    twice and stands on it)."""
    on_board = {int(r) for r in board if r >= 0}
    return [t for t in range(int(n_moves)) if t not in on_board and moves[t][0] != moves[t][1]]


def image(board, moves, n_moves, k):
    """The mirrored game's (board[9], moves[9][2] padded with 255, qmask[4], n_q) from a position's attributes."""
    s = CELLS[k]
    n = int(n_moves)
    out_board = [-1] * 9
    for v in range(9):
        out_board[s[v]] = int(board[v])
    out_moves = [[255, 255] for _ in range(9)]
    for t in range(n):
        out_moves[t] = sorted((s[int(moves[t][0])], s[int(moves[t][1])]))
    q = replay_qstructs([tuple(out_moves[t]) for t in live_rounds(board, moves, n)])
    qmask = [mask_of(c) for c in q] + [0] * (4 - len(q))
    return out_board, out_moves, qmask, len(q)


def mirrored_bit(lo, hi, bit, k):
    """The collapse bit of the mirrored game: 1 iff sigma of the landing square is the higher of the mapped pair."""
    s = CELLS[k]
    land = max(lo, hi) if bit else min(lo, hi)
    return 1 if s[land] == max(s[lo], s[hi]) else 0

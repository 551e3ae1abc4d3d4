"""The definition of include/qttt_selfplay_exact.h in numpy / float64 over tests/solve_model.py's Solver: which rows of a
self-play batch are relabelled, and with what.  Test infrastructure.  Also the inputs the CPU floor and the GPU tests
share: the recorded plain batches of tests/golden/selfplay_exact_plain.npz and a staging batch made of fixture boards."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle  # noqa: E402
import solve_model  # noqa: E402

ROWS = 10
MIN_PLY, MAX_PLY = 6, 9
ARRAYS = ("board", "moves", "n_moves", "qmask", "n_q")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLAIN = os.path.join(GOLDEN, "selfplay_exact_plain.npz")
# the recorded batches: SelfPlay(G, n_rollouts=8, net=golden f32, leaf_eval="value", value_targets=(1, -1)).play(SEED)
SEED, ROLLOUTS, PLAIN_GAMES = 2026, 8, (1, 3, 65)
# rows the model relabels in them, by (G, min_ply): what the floor asserts of the model and the GPU tests of the device
RELABELLED = {(1, 7): 1, (1, 8): 0, (3, 6): 6, (3, 7): 3, (3, 8): 0, (65, 6): 155, (65, 7): 94, (65, 8): 37}

_SOLVER = []


def solver():
    """One Solver for the whole session: its memo is what keeps the model's enumeration short."""
    if not _SOLVER:
        _SOLVER.append(solve_model.Solver())
    return _SOLVER[0]


def relabel(boards_per_row, length_or_rows, done, mask, pi, v, min_ply, policy):
    """(pi f64[10, G, 36], v f32[10, G], exact u8[10, G]) after qttt_selfplay_exact_targets.  boards_per_row: ten dicts of
    export_boards() arrays (board, moves, n_moves, qmask, n_q), row t's G boards; length_or_rows u8[G] is L.  `mask` is
    part of the staging set and not consulted: the legal actions are the position's own."""
    assert MIN_PLY <= int(min_ply) <= MAX_PLY and len(boards_per_row) == ROWS
    L = np.asarray(length_or_rows).astype(np.int64)
    G = len(L)
    done = np.asarray(done).reshape(ROWS, G)
    pi = np.array(pi, dtype=np.float64, copy=True).reshape(ROWS, G, 36)
    v = np.array(v, dtype=np.float32, copy=True).reshape(ROWS, G)
    assert np.asarray(mask).shape == (ROWS, G, 36)
    exact = np.zeros((ROWS, G), dtype=np.uint8)
    s = solver()
    for t in range(ROWS):
        live = [g for g in range(G) if t < L[g] and not done[t, g]]
        if not live:
            continue
        b = boards_per_row[t]
        ob = oracle.boards_from_arrays(*[np.asarray(b[k]) for k in ARRAYS])
        for g in live:
            key = ob.b[g].tobytes()
            if solve_model.played(key) < min_ply:
                continue
            r = s.solve(key)
            q16 = r["q"] * 16.0
            legal = np.isfinite(q16)
            if r["leaf"] or not legal.any():
                continue
            assert (q16[legal] == np.round(q16[legal])).all() and np.abs(q16[legal]).max() <= 16
            V = r["value"]
            best = legal & (r["q"] == V)                        # exact: sixteenths
            v[t, g] = np.float32(0.0 + V)
            if policy:
                pi[t, g] = np.where(best, 1.0 / float(best.sum()), 0.0)
            exact[t, g] = 1
    return pi, v, exact


def played_per_row(boards_per_row):
    """i64[10, G]: moves played of every staged board (0 for the empty board of a row past a game's length)."""
    out = []
    for b in boards_per_row:
        ob = oracle.boards_from_arrays(*[np.asarray(b[k]) for k in ARRAYS])
        out.append([solve_model.played(ob.b[g].tobytes()) for g in range(ob.n)])
    return np.array(out, dtype=np.int64)


# ---------------------------------------------------------------- the recorded plain batches
def plain(G):
    """The recorded play(SEED) batch of G games: dict(rows = ten dicts of board arrays, length, done, mask, pi, v, winner)."""
    with np.load(PLAIN) as z:
        out = {k: z["g%d_%s" % (G, k)] for k in ("length", "done", "mask", "pi", "v", "winner")}
        out["rows"] = [{k: z["g%d_%s" % (G, k)][t] for k in ARRAYS} for t in range(ROWS)]
    return out


# ---------------------------------------------------------------- a staging batch of fixture boards
def fixture_batch(G=65):
    """A staging batch that no game wrote, from tests/golden/solve_deep.npz: game g's row t holds a
    fixture board with t moves played for t = 4..8 (the rows below are empty boards, which is all a row with fewer moves
    needs to be), length 9 and no done row, except: game 1 is short (length 7), game 2 has done = 1 at row 7, games
    16..63 have length 0.  So at G = 65 the 64-record workgroups that cover rows 6..8 list the boards of games 0..15 (but
    the exceptions) and of game 64, those of rows 0..5 and of row 9 list none, and the sixteenths and eighths of
    solve_deep.npz are among the values.  pi and v hold recognisable garbage that a relabelled row must lose and every other
    row must keep.  Returns dict(rows, length, done, mask, pi, v)."""
    pools = {}
    with np.load(os.path.join(GOLDEN, "solve_deep.npz")) as z:
        deep = {k: z[k] for k in ARRAYS + ("played", "value", "q")}
    frac = np.abs(deep["value"] * 16) % 16 != 0                 # |V| not in {0, 1}
    for t in range(4, 9):
        idx = np.flatnonzero(deep["played"] == t)
        idx = np.concatenate([idx[frac[idx]], idx[~frac[idx]]])  # fractional values first
        pools[t] = idx
    rows = []
    for t in range(ROWS):
        if t in pools:
            pick = pools[t][np.arange(G) % len(pools[t])]
            rows.append({k: deep[k][pick].copy() for k in ARRAYS})
        else:
            rows.append({"board": np.zeros((G, 9), np.int8), "moves": np.full((G, 9, 2), 255, np.uint8),
                         "n_moves": np.zeros(G, np.uint8), "qmask": np.zeros((G, 4), np.uint16), "n_q": np.zeros(G, np.uint8)})
    length = np.full(G, 9, np.uint8)
    length[16:64] = 0
    if G > 1:
        length[1] = 7
    done = np.zeros((ROWS, G), np.uint8)
    if G > 2:
        done[7, 2] = 1
    rng = np.random.default_rng(7)
    pi = rng.random((ROWS, G, 36))
    v = rng.choice(np.array([-1.0, 0.0, 1.0, 0.3125], np.float32), (ROWS, G))
    mask = np.zeros((ROWS, G, 36), np.uint8)
    for t in pools:
        ob = oracle.boards_from_arrays(*[rows[t][k] for k in ARRAYS])
        L = oracle.lib()
        for g in range(G):
            m = int(L.qo_legal_mask(ob.b[g].tobytes()))
            mask[t, g] = [(m >> a) & 1 for a in range(36)]
    return {"rows": rows, "length": length, "done": done, "mask": mask, "pi": pi, "v": v}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view("u%d" % a.dtype.itemsize) if a.dtype.kind == "f" else a

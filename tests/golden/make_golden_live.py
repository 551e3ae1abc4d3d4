#!/usr/bin/env python3
"""Generates tests/golden/reference_live.npz from the UNMODIFIED reference (loaded through ref_shim.py): what the
reference returned for the inputs of tests/test_oracle_vs_reference.py, so that those tests hold the C oracle against
the reference without the reference being present.  Build container only; the .npz is data (inputs + expected outputs).

  fuzz{0,1}_*   3000 random episodes x 12 steps (fuzz1: 40 % of the actions arbitrary squares in 0..11): actions,
                collapse bits and every state field, reward, terminated, check_win after each step
  draw_*        300 episodes x up to 10 legal steps (bit 0): actions, random.choice calls per step, collapsed or not
  disp_*        200 random boards: Board.moves / .board and what displayBoard printed for them
  reward_*      Env._reward for every check_win pair (p1, p2) in -1..9
  ind2move, move2ind_fwd, move2ind_rev   mcts.py's action tables
  exp_*         every child MCTS._step made from every position to depth 2 (generation order), and the children count
                per (position, action)
  step2_*       every position reachable in <= 2 plies; per (action, bit) of {0..9}^2 + (255, 0), (3, 255) x {0, 1} the
                SHA-256 of what Env.step left (step2_digest, see digest_step2)
"""
import copy
import hashlib
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_shim import load_reference, REFERENCE_ROOT  # noqa: E402

OUT = os.path.join(HERE, "reference_live.npz")
STEP2_ACTIONS = [(a, b) for a in range(10) for b in range(10)] + [(255, 0), (3, 255)]


def digest_step2(board, n_moves, moves, qmask, n_q, reward, term, p1, p2):
    """One SHA-256 over the canonical arrays of one (action, bit) pass: board i8[n,9], n_moves u8[n], moves u8[n,9,2]
    (255 beyond n_moves), qmask u16[n,4] (0 beyond n_q), n_q u8[n], reward bits u32[n], terminated u8[n], check_win
    i8[n] x 2.  The test computes the same from the oracle."""
    h = hashlib.sha256()
    for a, dt in ((board, np.int8), (n_moves, np.uint8), (moves, np.uint8), (qmask, np.uint16), (n_q, np.uint8),
                  (reward, np.uint32), (term, np.uint8), (p1, np.int8), (p2, np.int8)):
        h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
    return h.hexdigest()


def fuzz(qtttgym, src, seed, n_eps, T, adversarial):
    rng = random.Random(seed)
    acts = np.zeros((n_eps, T, 2), dtype=np.uint8)
    bits = np.zeros((n_eps, T), dtype=np.uint8)
    exp = {k: [] for k in ("board", "n_moves", "moves", "qmask", "n_q", "reward", "term", "p1", "p2")}
    for e in range(n_eps):
        env = qtttgym.Env()
        env.reset()
        rows = {k: [] for k in exp}
        for t in range(T):
            board = env._gameboard.board
            empty = [i for i in range(9) if board[i] == -1]
            if adversarial and rng.random() < 0.4 or len(empty) < 2:
                a, b = rng.randrange(0, 12), rng.randrange(0, 12)
            else:
                a, b = rng.sample(empty, 2)
            bit = rng.getrandbits(1)
            src.bit = bit
            obs, r, term, trunc, info = env.step((a, b))
            acts[e, t] = (a, b)
            bits[e, t] = bit
            gb = env._gameboard
            rows["board"].append(list(gb.board))
            rows["n_moves"].append(len(gb.moves))
            mv = [[255, 255]] * 9
            for i, m in enumerate(gb.moves):
                mv[i] = [m[0], m[1]]
            rows["moves"].append(mv)
            qm = [0] * 4
            for i, s in enumerate(gb.qstructs):
                qm[i] = sum(1 << x for x in s)
            rows["qmask"].append(qm)
            rows["n_q"].append(len(gb.qstructs))
            rows["reward"].append(r)
            rows["term"].append(bool(term))
            p1, p2 = gb.check_win()
            rows["p1"].append(p1)
            rows["p2"].append(p2)
        for k in exp:
            exp[k].append(rows[k])
    dt = {"board": np.int8, "n_moves": np.uint8, "moves": np.uint8, "qmask": np.uint16, "n_q": np.uint8,
          "reward": np.float32, "term": np.uint8, "p1": np.int8, "p2": np.int8}
    out = {"acts": acts, "bits": bits}
    out.update((k, np.array(v).astype(dt[k])) for k, v in exp.items())
    return out


def draws(qtttgym, src):
    rng = random.Random(5)
    n_eps, T = 300, 10
    acts = np.full((n_eps, T, 2), 255, dtype=np.uint8)
    n_steps = np.zeros(n_eps, dtype=np.uint8)
    calls = np.zeros((n_eps, T), dtype=np.uint8)
    collapsed = np.zeros((n_eps, T), dtype=np.uint8)
    src.bit = 0
    for e in range(n_eps):
        env = qtttgym.Env()
        env.reset()
        for t in range(T):
            board = env._gameboard.board
            empty = [i for i in range(9) if board[i] == -1]
            if len(empty) < 2:
                break
            before = list(board)
            c0 = src.calls
            a = tuple(rng.sample(empty, 2))
            env.step(a)
            acts[e, t] = a
            calls[e, t] = src.calls - c0
            collapsed[e, t] = before != env._gameboard.board
            n_steps[e] = t + 1
    return {"acts": acts, "n_steps": n_steps, "calls": calls, "collapsed": collapsed}


def display(qtttgym, src):
    import contextlib
    import io
    rng = random.Random(77)
    n = 200
    moves = np.full((n, 9, 3), -1, dtype=np.int8)
    n_moves = np.zeros(n, dtype=np.uint8)
    board = np.zeros((n, 9), dtype=np.int8)
    text = []
    for k in range(n):
        gb = qtttgym.Board(qtttgym.QEvalClassic())
        for _ in range(rng.randrange(0, 10)):
            empty = [i for i in range(9) if gb.board[i] == -1]
            if len(empty) < 2:
                break
            src.bit = rng.getrandbits(1)
            gb.make_move(tuple(rng.sample(empty, 2)))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            qtttgym.displayBoard(gb)
        text.append(buf.getvalue())
        for i, m in enumerate(gb.moves):
            moves[k, i] = m
        n_moves[k], board[k] = len(gb.moves), gb.board
    return {"moves": moves, "n_moves": n_moves, "board": board, "text": np.array(text)}


def rewards(qtttgym):
    class FixedBoard:
        def __init__(self, pair):
            self.pair = pair

        def check_win(self):
            return self.pair
    env = qtttgym.Env()
    value = np.zeros((11, 11), dtype=np.float64)
    kind = np.zeros((11, 11), dtype="<U8")
    for p1 in range(-1, 10):
        for p2 in range(-1, 10):
            env._gameboard = FixedBoard((p1, p2))
            r = env._reward()
            value[p1 + 1, p2 + 1], kind[p1 + 1, p2 + 1] = r, type(r).__name__
    return {"value": value, "type": kind, "map_keys": np.array(list(env._reward_map)),
            "map_values": np.array(list(env._reward_map.values()), dtype=np.float64)}


def expand_depth3(qtttgym, ref_mcts):
    class Toggle:
        def __init__(self):
            self.bit = 0

        def choice(self, seq):
            out = seq[self.bit]
            self.bit ^= 1
            return out
    tog = Toggle()
    saved = qtttgym.qeval.random
    qtttgym.qeval.random = tog
    try:
        strat = ref_mcts.MCTS(rollouts=1, num_simulations=1)
        GS = ref_mcts.MCTS.GameState
        frontier = [GS([-1] * 9, [], True, None, False)]
        nch_all, kids = [], []
        wcode = {True: 1, False: 0, None: -1}
        for depth in range(3):
            nxt = []
            for gs in frontier:
                for a in range(36):
                    lo, hi = ref_mcts.ind2move(a)
                    tog.bit = 0
                    try:
                        ch = strat._step(gs, a)
                    except Exception:
                        ch = []
                    nch_all.append(len(ch))
                    if len(ch) == 2:
                        r = len(gs.moves)
                        ch.sort(key=lambda k: 0 if k.board[lo] == r else 1)
                    for k in ch:
                        mv = [[255, 255]] * 3
                        for j, m in enumerate(k.moves):
                            mv[j] = [m[0], m[1]]
                        kids.append((list(k.board), mv, len(k.moves), wcode[k.winner], bool(k.terminal), hash(k),
                                     sum(1 << x for x in k.actions)))
                        nxt.append(k)
            frontier = nxt
    finally:
        qtttgym.qeval.random = saved
    return {"nch": np.array(nch_all, dtype=np.uint8),
            "board": np.array([k[0] for k in kids], dtype=np.int8),
            "moves": np.array([k[1] for k in kids], dtype=np.uint8),
            "n_moves": np.array([k[2] for k in kids], dtype=np.uint8),
            "winner": np.array([k[3] for k in kids], dtype=np.int8),
            "terminal": np.array([k[4] for k in kids], dtype=np.uint8),
            "hash": np.array([k[5] for k in kids], dtype=np.int64),
            "legal": np.array([k[6] for k in kids], dtype=np.uint64)}


def step_depth2(qtttgym, src):
    positions = []

    def grow(gb, depth):
        positions.append(gb)
        if depth == 2:
            return
        for a in range(9):
            for b in range(a + 1, 9):
                if gb.board[a] != -1 or gb.board[b] != -1:
                    continue
                for bit in (0, 1):
                    src.bit = bit
                    calls = src.calls
                    k = copy.deepcopy(gb)
                    k.make_move((a, b))
                    if src.calls == calls and bit == 1:
                        continue                          # no collapse: the bit was not consumed, one child only
                    grow(k, depth + 1)
    grow(qtttgym.Board(qtttgym.QEvalClassic()), 0)
    n = len(positions)
    mv = np.full((n, 9, 2), 255, dtype=np.uint8)
    bd = np.zeros((n, 9), dtype=np.int8)
    qm = np.zeros((n, 4), dtype=np.uint16)
    nm = np.zeros(n, dtype=np.uint8)
    nq = np.zeros(n, dtype=np.uint8)
    for i, gb in enumerate(positions):
        for t, m in enumerate(gb.moves):
            mv[i, t] = m[:2]
        bd[i], nm[i], nq[i] = gb.board, len(gb.moves), len(gb.qstructs)
        for k, s in enumerate(gb.qstructs):
            qm[i, k] = sum(1 << x for x in s)
    env = qtttgym.Env()
    digests, truncated = [], []
    for a, b in STEP2_ACTIONS:
        for bit in (0, 1):
            rows = {k: [] for k in ("board", "n_moves", "moves", "qmask", "n_q", "reward", "term", "p1", "p2")}
            for gb in positions:
                g = qtttgym.Board(gb.qeval)
                g.board, g.moves, g.qstructs = list(gb.board), list(gb.moves), [set(q) for q in gb.qstructs]
                env._gameboard = g
                src.bit = bit
                _, r, term, trunc, _ = env.step((a, b))
                truncated.append(trunc is False)
                g = env._gameboard
                m = [[255, 255]] * 9
                for j, x in enumerate(g.moves):
                    m[j] = list(x[:2])
                q = [0] * 4
                for j, s in enumerate(g.qstructs):
                    q[j] = sum(1 << x for x in s)
                p1, p2 = g.check_win()
                for k, v in (("board", g.board), ("n_moves", len(g.moves)), ("moves", m), ("qmask", q),
                             ("n_q", len(g.qstructs)), ("reward", np.float32(r).view(np.uint32)), ("term", bool(term)),
                             ("p1", p1), ("p2", p2)):
                    rows[k].append(v)
            digests.append(digest_step2(*(np.array(rows[k]) for k in ("board", "n_moves", "moves", "qmask", "n_q",
                                                                       "reward", "term", "p1", "p2"))))
    assert all(truncated)
    return {"board": bd, "moves": mv, "n_moves": nm, "qmask": qm, "n_q": nq, "actions": np.array(STEP2_ACTIONS),
            "digest": np.array(digests)}


def main():
    qtttgym, src = load_reference()
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    import mcts as ref_mcts                      # the reference's mcts.py, unmodified
    data = {}
    for adversarial in (0, 1):
        data.update(("fuzz%d_%s" % (adversarial, k), v) for k, v in fuzz(qtttgym, src, 9001 + adversarial, 3000, 12,
                                                                           bool(adversarial)).items())
    data.update(("draw_" + k, v) for k, v in draws(qtttgym, src).items())
    data.update(("disp_" + k, v) for k, v in display(qtttgym, src).items())
    data.update(("reward_" + k, v) for k, v in rewards(qtttgym).items())
    data["ind2move"] = np.array([ref_mcts.ind2move(a) for a in range(36)], dtype=np.int64)
    data["move2ind_fwd"] = np.array([ref_mcts.move2ind(*ref_mcts.ind2move(a)) for a in range(36)], dtype=np.int64)
    data["move2ind_rev"] = np.array([ref_mcts.move2ind(*ref_mcts.ind2move(a)[::-1]) for a in range(36)], dtype=np.int64)
    data.update(("exp_" + k, v) for k, v in expand_depth3(qtttgym, ref_mcts).items())
    data.update(("step2_" + k, v) for k, v in step_depth2(qtttgym, src).items())
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()

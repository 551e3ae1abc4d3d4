"""The definition of include/qttt_solve.h in Python over the C oracle (qo_expand, qo_update_winner, qo_legal_mask), in
float64: the expectimax value of a position, the value of each of its actions, the lowest best action and the number of
positions the plain recursion visits.  Test infrastructure; practical for positions with five or more moves played.

The recursion is memoised on the 48 bytes of the oracle's board, and every entry keeps its own `nodes`, so the count
that comes out is the un-merged one: a transposition is looked up once and counted every time."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle  # noqa: E402

DENOMINATOR = 16            # QTTT_SOLVE_DENOMINATOR: every value times this is an integer
NEG_INF = float("-inf")


def played(rec_bytes):
    """Moves played: len(moves) without the autofill move (lo == hi), which nobody plays."""
    b = np.frombuffer(rec_bytes, dtype=oracle.BOARD_DTYPE)[0]
    n = int(b["n_moves"])
    return n - 1 if n and b["moves"][n - 1][0] == b["moves"][n - 1][1] else n


class Solver:
    def __init__(self):
        self.L = oracle.lib()
        self.memo = {}              # board bytes -> (value, nodes)
        self._w, self._t = ctypes.c_int(), ctypes.c_int()

    def _info(self, key):
        self.L.qo_update_winner(key, ctypes.byref(self._w), ctypes.byref(self._t))
        return self._w.value, self._t.value, int(self.L.qo_legal_mask(key))

    def _leaf_value(self, key, winner):
        if winner < 0:
            return 0.0
        first_to_move = played(key) % 2 == 0
        return 1.0 if (winner == 1) == first_to_move else -1.0

    def _children(self, key, a):
        child = ctypes.create_string_buffer(96)
        w, t, lm = (ctypes.c_int * 2)(), (ctypes.c_int * 2)(), (ctypes.c_uint64 * 2)()
        k = self.L.qo_expand(key, a, child, w, t, lm)
        return [child.raw[48 * c:48 * c + 48] for c in range(k)]

    def _q(self, key, a):
        """(Q(a), nodes below) or None where the expansion has no child."""
        kids = self._children(key, a)
        if not kids:
            return None
        vals = [self.value(k) for k in kids]
        total = sum(v for v, _ in vals)
        q = 0.0 - total if len(kids) == 1 else 0.0 - total / 2.0
        return q, sum(n for _, n in vals)

    def value(self, key):
        """(V, nodes) of the position with the oracle bytes `key`."""
        hit = self.memo.get(key)
        if hit is not None:
            return hit
        winner, terminal, legal = self._info(key)
        if terminal or legal == 0:
            out = (self._leaf_value(key, winner), 1)
        else:
            best, nodes = NEG_INF, 1
            for a in range(36):
                if legal >> a & 1:
                    r = self._q(key, a)
                    if r is not None:
                        best = max(best, r[0])
                        nodes += r[1]
            out = (best, nodes)
        self.memo[key] = out
        return out

    def solve(self, rec):
        """One board (a BOARD_DTYPE record or its 48 bytes) -> dict(value f64, q f64[36], best int, nodes int, leaf bool)."""
        key = rec if isinstance(rec, bytes) else np.asarray(rec, dtype=oracle.BOARD_DTYPE).tobytes()
        winner, terminal, legal = self._info(key)
        q = np.full(36, NEG_INF)
        if terminal or legal == 0:
            return {"value": self._leaf_value(key, winner), "q": q, "best": 255, "nodes": 1, "leaf": True}
        nodes = 1
        for a in range(36):
            if legal >> a & 1:
                r = self._q(key, a)
                if r is not None:
                    q[a] = r[0]
                    nodes += r[1]
        best = int(np.argmax(q))                    # the lowest action that attains the max
        return {"value": float(q[best]), "q": q, "best": best, "nodes": nodes, "leaf": False}


def solve_boards(ob, solver=None):
    """Every board of an oracle.OracleBoards -> dict of arrays: value f32, q f32[n, 36], best u8, nodes i64 (the casts of
    the float64 results: what the device must equal bit for bit)."""
    s = solver or Solver()
    res = [s.solve(ob.b[i]) for i in range(ob.n)]
    return {"value": np.array([r["value"] for r in res], dtype=np.float64).astype(np.float32),
            "q": np.array([r["q"] for r in res], dtype=np.float64).reshape(ob.n, 36).astype(np.float32),
            "best": np.array([r["best"] for r in res], dtype=np.uint8),
            "nodes": np.array([r["nodes"] for r in res], dtype=np.int64),
            "value64": np.array([r["value"] for r in res], dtype=np.float64),
            "q64": np.array([r["q"] for r in res], dtype=np.float64).reshape(ob.n, 36)}

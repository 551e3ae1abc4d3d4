"""The rooted forest of un-collapsed moves and the length of the re-root walk, in plain Python, for the tests: a helper
module that reads nothing from the package or the oracle.  Input is a fixture's `actions` and `bits` alone.

The state the step keeps (csrc/qttt_step_core.h): every square of a component but its tree's root has a parent edge.  A
legal move (lo, hi) picks its child end

    x = lo   if lo is in no component, or the move closes a cycle and the collapse bit is 0
    x = hi   otherwise

re-roots x's tree at x by reversing the parent edges from x up to the old root, and hangs x under the move's other end.
The walk length of a step is the number of edges from x to its root BEFORE the move: 0 for an isolated square, at most 8
(a nine-square path re-rooted from its far end).  On a cycle the whole component goes classical; a last empty square is
filled (board.py:22-25).  This is the only place the rule is restated."""
import numpy as np

NOOP, GROW, UNION, CYCLE = 0, 1, 2, 3
KIND_NAMES = ("noop", "grow", "union", "cycle")


class Forest:
    """One board: parent[v] = the other end of v's parent edge (None: a root or an isolated square), comps = the
    components as sets (their order is not modelled), classical = the collapsed squares."""

    def __init__(self):
        self.parent = [None] * 9
        self.comps = []
        self.classical = set()

    def _comp(self, v):
        return next((c for c in self.comps if v in c), None)

    def depth(self, v):
        d = 0
        while self.parent[v] is not None:
            v = self.parent[v]
            d += 1
            assert d <= 8, "a parent chain longer than nine squares"
        return d

    def step(self, a, b, bit):
        """Plays (a, b) with the offered collapse bit: (kind, size, walk).  size = squares of the component the move
        leaves (grow, union) or collapses (cycle); 0 for a noop."""
        if a > 8 or b > 8 or a == b or a in self.classical or b in self.classical:
            return NOOP, 0, 0
        lo, hi = min(a, b), max(a, b)
        c_lo, c_hi = self._comp(lo), self._comp(hi)
        cycle = c_lo is not None and c_lo is c_hi
        x = lo if (c_lo is None or (cycle and not (bit & 1))) else hi
        walk = self.depth(x)
        if cycle:
            for v in c_lo:
                self.parent[v] = None
            self.classical |= c_lo
            self.comps.remove(c_lo)
            if len(self.classical) == 8:                               # the autofill: it stands in no component
                self.classical = set(range(9))
            return CYCLE, len(c_lo), walk
        # reverse the path x -> old root, then x hangs under the move's other end
        v, prev = x, (hi if x == lo else lo)
        while v is not None:
            nxt = self.parent[v]
            self.parent[v] = prev
            v, prev = nxt, v
        if c_lo is not None and c_hi is not None:
            c_lo |= c_hi
            self.comps.remove(c_hi)
            return UNION, len(c_lo), walk
        c = c_lo if c_lo is not None else c_hi
        if c is None:
            c = set()
            self.comps.append(c)
        c |= {lo, hi}
        return GROW, len(c), walk


def walks(fx):
    """kind, size, walk and n_q (components after the step), each uint8[E, T], of a fixture's episodes."""
    acts, bits = fx["actions"], fx["bits"]
    E, T = bits.shape
    out = {k: np.zeros((E, T), dtype=np.uint8) for k in ("kind", "size", "walk", "n_q")}
    for e in range(E):
        f = Forest()
        for t in range(T):
            k, s, w = f.step(int(acts[e, t, 0]), int(acts[e, t, 1]), int(bits[e, t]))
            out["kind"][e, t], out["size"][e, t], out["walk"][e, t], out["n_q"][e, t] = k, s, w, len(f.comps)
    return out


def closing_steps(fx):
    """For each row that has a twin (twin[e] != e): the step at which the two rows' bits differ, the closing move;
    -1 for a row without a twin."""
    bits, twin = fx["bits"], fx["twin"]
    E = bits.shape[0]
    out = np.full(E, -1, dtype=np.int64)
    for e in range(E):
        if int(twin[e]) != e:
            d = np.nonzero(bits[e] != bits[int(twin[e])])[0]
            assert len(d) == 1, (e, d)
            out[e] = int(d[0])
    return out


def histogram(fx, w=None):
    """{(family, kind name): [count of walk length 0..8]} over the legal steps of a fixture."""
    w = w or walks(fx)
    fams = [str(k) for k in fx["kind"]]
    out = {}
    for fam in sorted(set(fams)):
        rows = np.array([f == fam for f in fams])
        for k in (GROW, UNION, CYCLE):
            sel = w["walk"][rows][w["kind"][rows] == k]
            out[(fam, KIND_NAMES[k])] = np.bincount(sel, minlength=9).tolist()
    return out

"""A float64 numpy restatement of include/qttt_selfplay_value.h: the searched value of a root from its W and N
(search_value, record_value) and the value targets made of it (value_targets, modes MIX and TD).  Python loops in
ascending order, IEEE doubles one operation at a time, np.float32 at the single rounding of a row.  No tolerance: the tests
compare bits."""
import numpy as np

ROWS = 10
MIX, TD = 0, 1
MODES = {"mix": MIX, "td": TD}


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def round_row(x):
    """The one rounding of a row: f64 -> f32, a zero (an underflow included) stored as +0.0."""
    y = np.float32(x)
    return np.float32(0.0) if y == 0 else y


def search_value(W, N, v_row):
    """q of one root: W f64[36], N int[36] as qttt_tree_root returns them; v_row the f32 the row holds."""
    sw, sn = np.float64(0.0), np.float64(0.0)
    for a in range(36):
        sw = sw + np.float64(W[a])
        sn = sn + np.float64(N[a])
    if sn > 0:
        return round_row(sw / sn)
    return np.float32(v_row)


def record_value(W, N, ply, length, q, v):
    """qttt_selfplay_record_value on numpy arrays: W f64[G, 36], N int[G, 36], ply an int or None (the stream form),
    length u8[G], q and v f32[10, G].  Returns the new q."""
    q = np.array(q, dtype=np.float32, copy=True)
    for g in range(len(length)):
        r = int(length[g]) if ply is None or ply < 0 else int(ply)
        if r >= ROWS or int(length[g]) != r:
            continue
        q[r, g] = search_value(W[g], N[g], v[r, g])
    return q


def blend(lam, a, b):
    x = (np.float64(1.0) - lam) * np.float64(a)
    y = lam * np.float64(b)
    return x + y


def value_targets(mode, lam, rows, length, done, exact, q, v):
    """qttt_selfplay_value_targets on numpy arrays; rows and exact may be None.  Returns the new v f32[10, G]."""
    mode = MODES.get(mode, mode)
    assert mode in (MIX, TD)
    lam = np.float64(lam)
    v = np.array(v, dtype=np.float32, copy=True)
    G = v.shape[1]
    for g in range(G):
        L = min(int(rows[g] if rows is not None else length[g]), ROWS)
        ex = [exact is not None and int(exact[t, g]) == 1 for t in range(ROWS)]
        if mode == MIX:
            for t in range(L):
                if int(done[t, g]) != 0 or ex[t]:
                    continue
                v[t, g] = round_row(blend(lam, v[t, g], q[t, g]))
            continue
        if L < 2:
            continue
        ret = np.float64(v[L - 1, g])
        for t in range(L - 2, -1, -1):
            keep = ex[t + 1] or int(done[t + 1, g]) != 0
            b = np.float64(v[t + 1, g]) if keep else np.float64(q[t + 1, g])
            ret = np.float64(0.0) - blend(lam, b, ret)
            if ex[t]:
                ret = np.float64(v[t, g])
            else:
                v[t, g] = round_row(ret)
    return v


def outcome_game(L, v0):
    """The record's value column of a finished game of L rows: v0 * (-1)^i, a zero as +0.0, and its done column."""
    v = np.zeros(ROWS, np.float32)
    done = np.zeros(ROWS, np.uint8)
    for i in range(L):
        x = np.float32(-v0 if i & 1 else v0)
        v[i] = np.float32(0.0) if x == 0 else x
    if L > 0:
        done[L - 1] = 1
    return v, done


def _random_f32(rng, shape, sixteenths):
    if sixteenths:
        x = (rng.integers(-16, 17, shape) / 16.0).astype(np.float32)
    else:
        x = (rng.standard_normal(shape) * np.exp(rng.uniform(-60.0, 3.0, shape))).astype(np.float32)
    return x + np.float32(0.0)                                                     # no -0.0


def hand_batch(G, seed, sixteenths, exact_kind="none", short_rows=False, random_v=False):
    """A hand-filled batch for the target kernel: every length 1..10 present (G permitting), finished games with the
    record's alternating outcome (random_v: random values in the rows below the terminal one instead), q random
    (multiples of 1/16, or finite f32 values from 1e-26 to 20 in magnitude).
    exact_kind: "none" (None), "zero" (all 0) or "late" (random on rows >= 5, with random v in sixteenths there).
    short_rows: also a rows vector with rows[g] = 0 for some games and rows[g] < length[g] for others."""
    rng = np.random.default_rng(seed)
    length = ((np.arange(G) % ROWS) + 1).astype(np.uint8)
    rng.shuffle(length)
    if G < ROWS:
        length = rng.permutation(np.arange(1, ROWS + 1))[:G].astype(np.uint8)
        length[0] = ROWS if G == 1 else length[0]
    v = np.zeros((ROWS, G), np.float32)
    done = np.zeros((ROWS, G), np.uint8)
    for g in range(G):
        v[:, g], done[:, g] = outcome_game(int(length[g]), float(rng.choice([1.0, -1.0, 0.0])))
    q = _random_f32(rng, (ROWS, G), sixteenths)
    if random_v:
        live = (np.arange(ROWS)[:, None] < length[None, :]) & (done == 0)
        v = np.where(live, _random_f32(rng, (ROWS, G), sixteenths), v)
    exact = None
    if exact_kind == "zero":
        exact = np.zeros((ROWS, G), np.uint8)
    elif exact_kind == "late":
        t = np.arange(ROWS)[:, None]
        exact = ((rng.random((ROWS, G)) < 0.5) & (t >= 5) & (t < length[None, :]) & (done == 0)).astype(np.uint8)
        truth = (rng.integers(-16, 17, (ROWS, G)) / 16.0).astype(np.float32) + np.float32(0.0)
        v = np.where(exact == 1, truth, v)
    rows = None
    if short_rows:
        rows = length.copy()
        rows[::3] = 0
        cut = np.flatnonzero((np.arange(G) % 3 == 1) & (length > 1))
        rows[cut] = (length[cut] * rng.random(len(cut))).astype(np.uint8)          # 0 <= rows < length
    return {"length": length, "done": done, "v": v, "q": q, "exact": exact, "rows": rows}

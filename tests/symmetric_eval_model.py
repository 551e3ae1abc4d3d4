"""The definition of include/qttt_nn_symmetric.h in numpy: the map back of an image's rows to the board's own actions
(l'[a] = l[tau_k[a]]), and the mean of 1, 2, 4 or 8 f32 terms as a balanced binary tree, scaled by the exact 1 / n.  A
plain helper module: the tests hand it the outputs of transformed(k).evaluate(net) and compare the fused entry with
what it returns."""
import numpy as np

ROWS = ("value", "logits", "probs")
SIZES = (1, 2, 4, 8)


def map_back(rows, tau_k):
    """rows f32[..., 36] of an image under k -> the same values indexed by the board's actions: out[..., a] =
    rows[..., tau_k[a]].  tau_k = ACTIONS[k] (qttt_symmetry_tables)."""
    return np.asarray(rows)[..., np.asarray(tau_k, dtype=np.int64)]


def pairwise_mean(terms):
    """terms f32[n, ...], n in SIZES, list position first: ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)) in f32,
    then times float32(1 / n); a single term is returned as it is."""
    x = np.asarray(terms)
    assert x.dtype == np.float32 and len(x) in SIZES
    n = len(x)
    with np.errstate(invalid="ignore", over="ignore"):
        while len(x) > 1:
            x = x[0::2] + x[1::2]
        return x[0] if n == 1 else x[0] * np.float32(1.0 / n)


def mapped_terms(images, symmetries, actions):
    """{row: f32[n_sym, N, ...]}: for list position j, image symmetries[j]'s rows mapped back.  images[k] = the dict of
    numpy rows that evaluate gives for the boards' images under k (only the k in `symmetries` are looked at)."""
    out = {}
    for row in ROWS:
        if row in images[symmetries[0]]:
            out[row] = np.stack([images[k][row] if row == "value" else map_back(images[k][row], actions[k])
                                 for k in symmetries]).astype(np.float32, copy=False)
    return out


def symmetric_mean(images, symmetries, actions):
    """The entry's outputs for the list `symmetries`: {row: f32[N, ...]}."""
    return {row: pairwise_mean(t) for row, t in mapped_terms(images, symmetries, actions).items()}


def per_board(images, sym, actions):
    """The per-board form: board i's rows are image sym[i]'s rows mapped back (an entry past 7 is the identity)."""
    sym = np.asarray(sym)
    k = np.where(sym < 8, sym, 0).astype(np.int64)
    i = np.arange(len(k))
    tau = np.asarray(actions, dtype=np.int64)[k]                       # [N, 36]
    out = {}
    for row in ROWS:
        if row in images[0]:
            stack = np.stack([images[j][row] for j in range(8)])      # [8, N, ...]
            out[row] = stack[k, i] if row == "value" else stack[k, i][i[:, None], tau]
    return out


def same_bits(a, b):
    """Equal bit for bit, NaNs matched with NaNs (whatever their payload)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))

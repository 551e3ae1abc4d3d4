"""The eight symmetries of the board (include/qttt_symmetry.h): k = 0..7, a mirror first if k & 4, then
k & 3 quarter turns clockwise.  The tables are the library's own (qttt_symmetry_tables), read once and never restated
here: CELLS[k][v] = sigma_k(v), ACTIONS[k][a] = tau_k(a) on the 36-action indexing, INVERSE[k], and COMPOSE[a][b] = the
k of "a first, then b".  States are mapped by VecEnv.transformed, a whole self-play batch by SelfPlayBatch.augment."""
import ctypes

import torch

from . import _native

N_SYMMETRIES = _native.SYMMETRIES
_NAMES = ("CELLS", "ACTIONS", "INVERSE", "COMPOSE")
_host = None
_device = {}


def tables():
    """(CELLS 8 x 9, ACTIONS 8 x 36, INVERSE 8, COMPOSE 8 x 8) as tuples of ints, from the library."""
    global _host
    if _host is None:
        K = N_SYMMETRIES
        bufs = [(ctypes.c_uint8 * n)() for n in (K * 9, K * 36, K, K * K)]
        _native.check(_native.lib().qttt_symmetry_tables(*bufs), "qttt_symmetry_tables")
        rows = lambda b, w: tuple(tuple(b[k * w:(k + 1) * w]) for k in range(K))
        _host = (rows(bufs[0], 9), rows(bufs[1], 36), tuple(bufs[2]), rows(bufs[3], K))
    return _host


def __getattr__(name):
    if name in _NAMES:
        return tables()[_NAMES.index(name)]
    raise AttributeError(name)


def _k(k):
    k = int(k)
    if not 0 <= k < N_SYMMETRIES:
        raise ValueError("a symmetry is 0..%d, got %d" % (N_SYMMETRIES - 1, k))
    return k


def inverse(k):
    return tables()[2][_k(k)]


def compose(a, b):
    """The symmetry that is `a` first, then `b`."""
    return tables()[3][_k(a)][_k(b)]


def check_symmetries(symmetries):
    """`symmetries` (None: all eight, in order) as a tuple of 1..8 ints in 0..7."""
    sym = tuple(range(N_SYMMETRIES)) if symmetries is None else tuple(_k(k) for k in symmetries)
    if not 1 <= len(sym) <= N_SYMMETRIES:
        raise ValueError("1..%d symmetries, got %d" % (N_SYMMETRIES, len(sym)))
    return sym


def check_eval_symmetries(symmetries):
    """The list a symmetry-averaged evaluation takes the mean over (include/qttt_nn_symmetric.h), as a tuple: "all" or a
    sequence of 1, 2, 4 or 8 ints in 0..7."""
    sym = tuple(range(N_SYMMETRIES)) if isinstance(symmetries, str) and symmetries == "all" else tuple(_k(k) for k in symmetries)
    if len(sym) not in _native.NN_SYMMETRIC_SIZES:
        raise ValueError("the mean is taken over %s symmetries, got %d" % (" | ".join(map(str, _native.NN_SYMMETRIC_SIZES)), len(sym)))
    return sym


def device_tables(device):
    """(cells u8[8, 9], actions u8[8, 36]) as tensors on `device`, the action table with 220 more columns that map
    36..255 to themselves (255: no action)."""
    device = torch.device(device)
    t = _device.get(device)
    if t is None:
        cells, actions = tables()[:2]
        wide = [list(row) + list(range(36, 256)) for row in actions]
        t = _device[device] = (torch.tensor(cells, dtype=torch.uint8, device=device),
                               torch.tensor(wide, dtype=torch.uint8, device=device))
    return t


def transform_action36(a, k):
    """tau_k of a u8 tensor of action indices; k an int or an integer tensor that broadcasts against `a`.  An index
    past 35 (255: none) stays."""
    if a.dtype != torch.uint8:
        raise ValueError("action36 must be a uint8 tensor")
    wide = device_tables(a.device)[1]
    if torch.is_tensor(k):
        k = k.to(device=a.device, dtype=torch.int64)
        if bool(((k < 0) | (k >= N_SYMMETRIES)).any()):
            raise ValueError("a symmetry is 0..%d" % (N_SYMMETRIES - 1))
    else:
        k = _k(k)
    return wide[k, a.to(torch.int64)]

"""CPU tests of the board's symmetries (include/qttt_symmetry.h, qtttgym_amd.symmetry): the group's tables, from the
definition and from the library; the Python model of a state's image (tests/symmetry_model.py) and the repository's
oracle, played in pairs, against games of the reference recorded beside their mirrored games
(tests/golden/symmetry_traces.npz); the header, the binding table and the argument errors.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qttt_symmetry.h")

import symmetry_model as M  # noqa: E402
from qtttgym_amd import _native, ind2move, move2ind, symmetry  # noqa: E402

ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3
SIDE_KEYS = ("board", "moves", "n_moves", "qmask", "n_q")


@pytest.fixture(scope="module")
def traces():
    with np.load(os.path.join(ROOT, "tests", "golden", "symmetry_traces.npz")) as z:
        return {k: z[k] for k in z.files}


def positions(tr):
    """(game, ply) of every recorded position."""
    return [(g, t) for g in range(len(tr["k"])) for t in range(int(tr["n_plies"][g]))]


# ---------------------------------------------------------------- the tables
def test_the_eight_symmetries_are_the_dihedral_group():
    assert M.CELLS[0] == tuple(range(9)) and len(set(M.CELLS)) == 8
    assert M.CELLS[1] == (2, 5, 8, 1, 4, 7, 0, 3, 6)          # a quarter turn clockwise: the top row becomes the right column
    assert M.CELLS[4] == (2, 1, 0, 5, 4, 3, 8, 7, 6)          # the mirror: columns swapped
    for k in range(8):
        assert sorted(M.CELLS[k]) == list(range(9)) and M.CELLS[k][4] == 4
        assert {frozenset(M.CELLS[k][v] for v in line) for line in M.LINES} == {frozenset(line) for line in M.LINES}
    for a in range(8):
        for b in range(8):
            k = M.COMPOSE[a][b]                               # closed: a first, then b is one of the eight
            assert all(M.CELLS[k][v] == M.CELLS[b][M.CELLS[a][v]] for v in range(9))
        assert M.COMPOSE[a][M.INVERSE[a]] == 0 == M.COMPOSE[M.INVERSE[a]][a]
        assert M.COMPOSE[a][0] == a == M.COMPOSE[0][a]
    assert M.COMPOSE[1][1] == 2 and M.COMPOSE[1][3] == 0 and M.COMPOSE[4][4] == 0 and M.INVERSE[1] == 3
    assert any(M.COMPOSE[a][b] != M.COMPOSE[b][a] for a in range(8) for b in range(8))      # not abelian


def test_every_action_table_is_a_bijection_consistent_with_the_pair_indexing():
    for k in range(8):
        assert sorted(M.ACTIONS[k]) == list(range(36))
        for a in range(36):
            i, j = ind2move(a)
            assert M.ACTIONS[k][a] == move2ind(M.CELLS[k][i], M.CELLS[k][j])
    for a in range(8):
        for b in range(8):
            assert all(M.ACTIONS[M.COMPOSE[a][b]][x] == M.ACTIONS[b][M.ACTIONS[a][x]] for x in range(36))


def test_the_library_tables_are_the_model_tables():
    assert symmetry.CELLS == M.CELLS and symmetry.ACTIONS == M.ACTIONS
    assert symmetry.INVERSE == M.INVERSE and symmetry.COMPOSE == M.COMPOSE
    assert [symmetry.inverse(k) for k in range(8)] == list(M.INVERSE)
    assert all(symmetry.compose(a, b) == M.COMPOSE[a][b] for a in range(8) for b in range(8))
    L = _native.lib()
    cells = (ctypes.c_uint8 * 72)()
    assert L.qttt_symmetry_tables(cells, None, None, None) == 0 and tuple(cells[9:18]) == M.CELLS[1]    # each is nullable
    assert L.qttt_symmetry_tables(None, None, None, None) == 0
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            symmetry.inverse(bad)
        with pytest.raises(ValueError):
            symmetry.compose(0, bad)
    for bad in ([], [0] * 9, [8], [0, -1]):
        with pytest.raises(ValueError):
            symmetry.check_symmetries(bad)
    assert symmetry.check_symmetries(None) == tuple(range(8)) and symmetry.check_symmetries([3, 3]) == (3, 3)


def test_transform_action36_on_host_tensors():
    import torch
    a = torch.tensor([0, 7, 35, 36, 255], dtype=torch.uint8)
    for k in range(8):
        assert symmetry.transform_action36(a, k).tolist() == [M.ACTIONS[k][0], M.ACTIONS[k][7], M.ACTIONS[k][35], 36, 255]
    ks = torch.tensor([0, 1, 2, 3, 4])
    assert symmetry.transform_action36(a, ks).tolist() == [0, M.ACTIONS[1][7], M.ACTIONS[2][35], 36, 255]
    grid = symmetry.transform_action36(torch.arange(36, dtype=torch.uint8)[None, :], torch.arange(8)[:, None])
    assert grid.dtype == torch.uint8 and grid.tolist() == [list(r) for r in M.ACTIONS]
    with pytest.raises(ValueError):
        symmetry.transform_action36(a, 8)
    with pytest.raises(ValueError):
        symmetry.transform_action36(a, torch.tensor([0, 1, 2, 3, 8]))
    with pytest.raises(ValueError):
        symmetry.transform_action36(a.to(torch.int64), 0)


# ---------------------------------------------------------------- the fixture, the model, the oracle
def _permuted_order(tr, g, t):
    k = int(tr["k"][g])
    return [M.map_mask(int(m), k) for m in tr["a_qmask"][g, t]]


def test_the_fixture_holds_the_order_cases(traces):
    tr = traces
    assert len(tr["k"]) == 512 and set(tr["k"].tolist()) == set(range(8))
    pos = positions(tr)
    assert len(pos) == int(tr["n_plies"].sum()) >= 4000
    order = 0
    for g, t in pos:
        k = int(tr["k"][g])
        s = M.CELLS[k]
        # board, moves (each pair re-sorted) and the SET of qstructs are the permuted attributes of the original ...
        assert [int(tr["b_board"][g, t][s[v]]) for v in range(9)] == tr["a_board"][g, t].tolist()
        n = int(tr["a_n_moves"][g, t])
        assert n == int(tr["b_n_moves"][g, t]) and int(tr["a_n_q"][g, t]) == int(tr["b_n_q"][g, t])
        assert [sorted((s[i], s[j])) for i, j in tr["a_moves"][g, t, :n].tolist()] == tr["b_moves"][g, t, :n].tolist()
        perm = _permuted_order(tr, g, t)
        assert sorted(perm) == sorted(tr["b_qmask"][g, t].tolist())
        order += perm != tr["b_qmask"][g, t].tolist()          # ... the LIST ORDER is not
    assert order >= 20, order


def test_the_model_reproduces_the_mirrored_game_at_every_ply(traces):
    tr = traces
    order = 0
    for g, t in positions(tr):
        k = int(tr["k"][g])
        board, moves, qmask, n_q = M.image(tr["a_board"][g, t], tr["a_moves"][g, t], tr["a_n_moves"][g, t], k)
        assert board == tr["b_board"][g, t].tolist() and moves == tr["b_moves"][g, t].tolist(), (g, t)
        assert qmask == tr["b_qmask"][g, t].tolist() and n_q == int(tr["b_n_q"][g, t]), (g, t)
        order += _permuted_order(tr, g, t) != qmask
        # and of each game on its own: the list order IS the replay of its un-collapsed moves (k = 0)
        for side in "ab":
            same = M.image(tr[side + "_board"][g, t], tr[side + "_moves"][g, t], tr[side + "_n_moves"][g, t], 0)
            assert same[2] == tr[side + "_qmask"][g, t].tolist(), (side, g, t)
    assert order >= 20


def test_the_oracle_played_in_pairs_reproduces_both_games(traces):
    import oracle
    tr = traces
    G = len(tr["k"])
    a, b = oracle.OracleBoards(G), oracle.OracleBoards(G)
    ks = tr["k"].astype(int)
    cells = np.array(M.CELLS)
    for t in range(9):
        live = tr["n_plies"] > t
        mv = tr["move"][:, t].astype(int)
        lo, hi, L = np.where(live, mv[:, 0], 0), np.where(live, mv[:, 1], 0), np.where(live, tr["landing"][:, t], 0)
        bit_a = (L == hi).astype(np.uint8)
        slo, shi = cells[ks, lo], cells[ks, hi]
        bit_b = (cells[ks, L] == np.maximum(slo, shi)).astype(np.uint8)
        assert bit_b.tolist() == [M.mirrored_bit(int(x), int(y), int(z), int(k)) for x, y, z, k in zip(lo, hi, bit_a, ks)]
        act_a = np.where(live[:, None], np.stack([lo, hi], 1), 255).astype(np.uint8)        # (255, 255): a noop
        act_b = np.where(live[:, None], np.stack([slo, shi], 1), 255).astype(np.uint8)
        a.step(act_a, bit_a)
        b.step(act_b, bit_b)
        for side, ob in (("a", a), ("b", b)):
            for key in SIDE_KEYS:
                got = getattr(ob, key)[live]
                assert np.array_equal(got, tr[side + "_" + key][live, t].astype(got.dtype)), (side, key, t)


# ---------------------------------------------------------------- header, binding table
def test_header_is_plain_c99_and_included_by_qttt_h_after_selfplay():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_selfplay.h"') < src.index('#include "qttt_symmetry.h"')
    vp18 = ", ".join(["const void *", "const double *", "const uint8_t *", "const uint8_t *", "const float *",
                      "const uint8_t *", "const uint8_t *", "const int8_t *", "const uint8_t *", "void *", "double *",
                      "uint8_t *", "uint8_t *", "float *", "uint8_t *", "uint8_t *", "int8_t *", "uint8_t *"])
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                          "-I" + os.path.join(ROOT, "include"), "-"],
                         input='#include "qttt.h"\nint main(void){'
                               'int (*t)(uint8_t *, uint8_t *, uint8_t *, uint8_t *) = qttt_symmetry_tables;\n'
                               'int (*f)(const void *, void *, const uint8_t *, int, int64_t, void *) = qttt_transform;\n'
                               'int (*a)(int64_t, const uint8_t *, int, %s, void *) = qttt_selfplay_augment;\n'
                               'return t == 0 || f == 0 || a == 0 || QTTT_SYMMETRIES != 8 || QTTT_ABI_VERSION != 6;}\n' % vp18,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_binding_header_exports_and_build_list_agree():
    import __graft_entry__ as entry
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.SYMMETRY_SIGNATURES) == {"qttt_symmetry_tables", "qttt_transform", "qttt_selfplay_augment"}
    assert not names & (set(_native.SIGNATURES) | set(_native.TREE_SIGNATURES) | set(_native.SELFPLAY_SIGNATURES))
    assert HEADER in entry.HEADERS
    L = _native.lib()                                        # resolves every table, this one included
    for name in names:
        assert getattr(ctypes.CDLL(_native.LIB_PATH), name)
        assert getattr(L, name).argtypes == _native.SYMMETRY_SIGNATURES[name][1]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # additive entries: the ABI number stays
    assert _native.SYMMETRIES == 8 and re.search(r"#define QTTT_SYMMETRIES 8\b", src)
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "qttt_transform" in text and "qttt_selfplay_augment" in text, doc


# ---------------------------------------------------------------- argument errors
def _transform(L, state_in=0x1000, state_out=0x2000, sym=None, k=0, n=1):
    """The entry with fake addresses (never dereferenced: every call of this file fails its checks first)."""
    return L.qttt_transform(state_in, state_out, sym, k, n, None)


def test_transform_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    for kw in (dict(n=-1), dict(k=-1), dict(k=8), dict(k=8, sym=0x3000)):
        assert _transform(L, **kw) == ERR_SIZE, kw
        assert _transform(L, state_in=None, state_out=None, **kw) == ERR_SIZE, kw
        assert _transform(L, state_in=0x1001, state_out=0x2001, **kw) == ERR_SIZE, kw
    assert _transform(L, n=0, state_in=None, state_out=None) == 0          # nothing to do, no pointer looked at
    assert _transform(L, n=0, state_in=0x1001, state_out=0x2001, k=7) == 0
    assert _transform(L, n=0, k=8) == ERR_SIZE                              # (but the sizes still come first)
    assert _transform(L, state_in=None) == ERR_NULL and _transform(L, state_out=None) == ERR_NULL
    assert _transform(L, state_in=None, state_out=0x2001) == ERR_NULL      # nulls before alignment
    assert _transform(L, state_in=0x1001, state_out=None) == ERR_NULL
    for off in (1, 8):
        assert _transform(L, state_in=0x1000 + off) == ERR_ACTION and _transform(L, state_out=0x2000 + off) == ERR_ACTION
    assert _transform(L, state_in=0x1008, state_out=0x1008, sym=0x3001) == ERR_ACTION


def _augment(L, games=1, sym=(0,), n_sym=None, bufs=None):
    arr = None if sym is None else (ctypes.c_uint8 * max(len(sym), 1))(*sym)
    bufs = [0x10000 + 0x100 * k for k in range(18)] if bufs is None else bufs
    return L.qttt_selfplay_augment(games, arr, len(sym) if n_sym is None else n_sym, *bufs, None)


def test_augment_return_codes_in_documented_order_without_device_work():
    L = _native.lib()
    nothing, odd = [None] * 18, [0x10001 + 0x100 * k for k in range(18)]
    for kw in (dict(games=-1), dict(sym=(), n_sym=0), dict(sym=(0,) * 9), dict(sym=(0,), n_sym=-1), dict(sym=(8,)),
               dict(sym=(0, 1, 255)), dict(sym=tuple(range(8)), n_sym=9)):
        assert _augment(L, **kw) == ERR_SIZE, kw
        assert _augment(L, bufs=nothing, **kw) == ERR_SIZE, kw
        assert _augment(L, bufs=odd, **kw) == ERR_SIZE, kw
    assert _augment(L, games=0, bufs=nothing) == 0                          # nothing to do, no buffer looked at
    assert _augment(L, games=0, bufs=odd, sym=tuple(range(8))) == 0
    assert _augment(L, games=0, sym=None, n_sym=3, bufs=nothing) == 0
    assert _augment(L, games=0, sym=(9,)) == ERR_SIZE                       # (but the sizes still come first)
    assert _augment(L, sym=None, n_sym=1) == ERR_NULL                       # then nulls, before any alignment
    for k in range(18):
        bufs = list(odd)
        bufs[k] = None
        assert _augment(L, bufs=bufs) == ERR_NULL, k
    # then alignment: states 16 bytes, pi 8, v 4, of either side; the byte buffers take any address
    # (`good` itself is never passed: it would pass every check and launch)
    good = [0x10000 + 0x100 * k + (0 if k % 9 in (0, 1, 4) else 1) for k in range(18)]
    for k, off in ((0, 8), (0, 1), (1, 4), (1, 1), (4, 2), (4, 1), (9, 8), (10, 4), (13, 2)):
        bufs = list(good)
        bufs[k] += off
        assert _augment(L, bufs=bufs) == ERR_ACTION, (k, off)


def test_python_checks_its_arguments_before_it_asks_for_a_device():
    from qtttgym_amd import SelfPlayBatch, VecEnv
    assert callable(VecEnv.transformed) and callable(SelfPlayBatch.augment)
    batch = SelfPlayBatch.__new__(SelfPlayBatch)             # no device: the symmetries are checked first
    for bad in ([], [8], [0] * 9):
        with pytest.raises(ValueError):
            batch.augment(bad)

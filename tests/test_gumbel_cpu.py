"""CPU tests of the Gumbel root (include/qttt_tree_gumbel.h, TreeSearch(root_policy="gumbel")): the library's host-only
visit sequence against hand-written expectations and its invariants; tests/gumbel_model.py's rules on synthetic
statistics; the model alone on the searches tests/test_gumbel_gpu.py runs (how many root decisions are too close to
call); the header and the binding table; the constructors' checks.  No GPU."""
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
HEADER = os.path.join(ROOT, "include", "qttt_tree_gumbel.h")

import gumbel_model as GM  # noqa: E402
from qtttgym_amd import _native  # noqa: E402

ERR_NULL, ERR_SIZE = -1, -2


def _sequence(m, n):
    out = np.full(n, -7, dtype=np.int32)
    assert _native.lib().qttt_gumbel_visit_sequence(m, n, out.ctypes.data) == 0
    return out.tolist()


# ---------------------------------------------------------------- the visit sequence
HAND = {(1, 5): [0, 1, 2, 3, 4],
        (2, 4): [0, 0, 1, 1],
        (4, 8): [0, 0, 0, 0, 1, 1, 2, 2],
        (16, 32): [0] * 16 + [1] * 8 + [2] * 4 + [3] * 4,
        (3, 7): [0, 0, 0, 1, 1, 2, 2],
        (36, 16): [0] * 16}


@pytest.mark.parametrize("m,n", sorted(HAND))
def test_visit_sequence_by_hand(m, n):
    assert _sequence(m, n) == HAND[m, n] == GM.visit_sequence(m, n)


@pytest.mark.parametrize("n", [1, 2, 16, 50, 200])
def test_visit_sequence_invariants(n):
    for m in range(1, 37):
        seq = _sequence(m, n)
        assert len(seq) == n and seq == GM.visit_sequence(m, n) and seq[0] == 0
        if m == 1:
            assert seq == list(range(n))
            continue
        # a phase visits its c actions once each, all at the same count: c halves from m down to 2 and stays there
        widths, i, c, L = [], 0, m, int(np.ceil(np.log2(m)))
        while i < n:
            for _ in range(max(1, n // (L * c))):
                row = seq[i:i + c]
                assert len(set(row)) <= 1, (m, n, i)               # one count per sweep over the survivors
                if row:
                    widths.append(c)
                i += c
            c = max(2, c // 2)
        assert widths[0] == m and all(b in (a, max(2, a // 2)) for a, b in zip(widths, widths[1:]))
        assert n < 2 * m * L or widths[-1] == 2                    # a budget that reaches the end halves down to 2
        for ph in GM.phases(seq):
            assert all(a <= b for a, b in zip(ph, ph[1:]))


def test_visit_sequence_errors():
    L = _native.lib()
    buf = np.zeros(4, dtype=np.int32)
    for m, n in ((-1, 4), (37, 4), (2, 0), (2, -1), (2, (1 << 24) + 1)):
        assert L.qttt_gumbel_visit_sequence(m, n, buf.ctypes.data) == ERR_SIZE
        assert L.qttt_gumbel_visit_sequence(m, n, None) == ERR_SIZE
    assert L.qttt_gumbel_visit_sequence(2, 4, None) == ERR_NULL
    assert L.qttt_tree_gumbel_bytes(5) == 5 * 880 and L.qttt_tree_gumbel_bytes(0) == 0
    assert L.qttt_tree_gumbel_bytes(-1) == ERR_SIZE


# ---------------------------------------------------------------- the model on synthetic statistics
def _synthetic(seed):
    rng = np.random.default_rng(seed)
    legal = sorted(rng.choice(36, size=int(rng.integers(1, 37)), replace=False).tolist())
    logits = np.full(36, -np.inf, dtype=np.float32)
    logits[legal] = rng.normal(size=len(legal)).astype(np.float32) * 3
    N = np.zeros(36, dtype=np.int64)
    N[legal] = rng.integers(0, 6, size=len(legal)) * (rng.random(len(legal)) < 0.6)
    W = np.zeros(36)
    W[legal] = rng.uniform(-1, 1, len(legal)) * N[legal]
    gumbel = np.zeros(36)
    gumbel[legal] = GM.gumbel_of(rng.random(len(legal)) * 0.999 + 0.0005)
    return legal, logits, N, W, gumbel, np.float32(rng.uniform(-1, 1))


def _rec(legal, logits, gumbel, root_value, m, n0=None):
    considered, m_eff = GM.top_considered(gumbel, logits, legal, m)
    prior = GM.softmax_legal(logits.astype(np.float64), legal)
    return GM.make_rec(gumbel, prior, logits, np.zeros(36, np.int64) if n0 is None else n0, considered, root_value, m_eff)


@pytest.mark.parametrize("seed", range(40))
def test_model_properties_on_synthetic_statistics(seed):
    legal, logits, N, W, gumbel, rv = _synthetic(seed)
    rec = _rec(legal, logits, gumbel, rv, 1 + seed % 36)
    assert rec["m_eff"] == min(1 + seed % 36, len(legal)) == bin(rec["considered"]).count("1")
    cons = [a for a in range(36) if (rec["considered"] >> a) & 1]
    assert set(cons) <= set(legal)
    assert all(rec["s0"][a] >= rec["s0"][b] for a in cons for b in legal if b not in cons)
    choose, pi, q_hat, _ = GM.final(rec, N, W, legal, 50.0, 1.0)
    assert abs(pi.sum() - 1.0) <= 36 * 2.0 ** -52 and (pi[[a for a in range(36) if a not in legal]] == 0).all()
    assert choose in cons
    # no visits: v_mix is the root's value, for every action
    q0, s0, v0 = GM.completed_q(np.zeros(36, np.int64), np.zeros(36), legal, rec["prior"], rv, 50.0, 1.0)
    assert v0 == np.float64(rv) and (q0[legal] == np.float64(rv)).all()
    # visited actions keep their own mean, unvisited ones get v_mix, which lies within the values it mixes
    q1, _, v1 = GM.completed_q(N, W, legal, rec["prior"], rv, 50.0, 1.0)
    seen = [a for a in legal if N[a]]
    assert all(q1[a] == W[a] / N[a] for a in seen) and all(q1[a] == v1 for a in legal if not N[a])
    if seen:
        lo, hi = min([float(rv)] + [q1[a] for a in seen]), max([float(rv)] + [q1[a] for a in seen])
        assert lo - 1e-12 <= v1 <= hi + 1e-12
    # a constant added to all logits (exactly representable, so s0's order and gaps stay) changes no decision
    shifted = logits.copy()
    shifted[legal] = (logits[legal].astype(np.float64) + 4.0).astype(np.float32)
    if (shifted[legal].astype(np.float64) - 4.0 == logits[legal].astype(np.float64)).all():
        rec2 = _rec(legal, shifted, gumbel, rv, 1 + seed % 36)
        # gumbel + logit may round differently after the shift: only decisions with a margin above that count
        choose2, pi2, _, margin2 = GM.final(rec2, N, W, legal, 50.0, 1.0)
        _, _, _, margin = GM.final(rec, N, W, legal, 50.0, 1.0)
        if min(margin, margin2) > 1e-9 and rec2["considered"] == rec["considered"]:
            assert choose2 == choose
        assert np.allclose(pi2, pi, rtol=1e-12, atol=0)
        for c in range(3):
            a1, g1 = GM.root_action(rec, N, np.zeros(36, int), W, legal, c, 50.0, 1.0)
            a2, g2 = GM.root_action(rec2, N, np.zeros(36, int), W, legal, c, 50.0, 1.0)
            if min(g1, g2) > 1e-9 and rec2["considered"] == rec["considered"]:
                assert a1 == a2


def test_root_rule_by_hand():
    legal = [0, 3, 7, 9]
    logits = np.full(36, -np.inf, dtype=np.float32)
    logits[legal] = [1.0, 0.0, 2.0, -1.0]
    gumbel = np.zeros(36)
    gumbel[legal] = [0.5, 3.0, 0.0, 0.25]                          # s0 = 1.5, 3.0, 2.0, -0.75
    rec = _rec(legal, logits, gumbel, 0.25, 3)
    assert rec["considered"] == (1 << 0) | (1 << 3) | (1 << 7) and rec["m_eff"] == 3
    N, W, F = np.zeros(36, np.int64), np.zeros(36), np.zeros(36, np.int64)
    # nothing visited: sigma is one constant, the largest s0 with 0 visits wins; an in-flight visit counts as a visit
    assert GM.root_action(rec, N, F, W, legal, 0, 50.0, 1.0)[0] == 3
    F[3] = 1
    assert GM.root_action(rec, N, F, W, legal, 0, 50.0, 1.0)[0] == 7
    F[7] = 1
    assert GM.root_action(rec, N, F, W, legal, 0, 50.0, 1.0)[0] == 0
    F[0] = 1
    assert GM.root_action(rec, N, F, W, legal, 0, 50.0, 1.0)[0] == 3          # nobody matches: all considered
    assert GM.root_action(rec, N, F, W, legal, 1, 50.0, 1.0)[0] == 3
    # completed Q: action 3 lost its visit, action 7 won: sigma = (50 + 1) * q
    N[[3, 7]], W[[3, 7]], F[:] = 1, [-1.0, 1.0], 0
    q, sigma, v_mix = GM.completed_q(N, W, legal, rec["prior"], 0.25, 50.0, 1.0)
    p = rec["prior"]
    assert v_mix == (0.25 + (2.0 * GM.wave_sum(np.where(N > 0, p * q, 0))) / GM.wave_sum(np.where(N > 0, p, 0))) / 3.0
    assert q[3] == -1.0 and q[7] == 1.0 and q[0] == q[9] == v_mix and sigma[7] == 51.0
    assert GM.root_action(rec, N, F, W, legal, 1, 50.0, 1.0)[0] == 7
    choose, pi, _, _ = GM.final(rec, N, W, legal, 50.0, 1.0)
    assert choose == 7 and pi.argmax() == 7
    rec["n0"][7] = 1                                               # a reused subtree: that visit was there before begin
    assert GM.final(rec, N, W, legal, 50.0, 1.0)[0] == 3 and GM.root_action(rec, N, F, W, legal, 0, 50.0, 1.0)[0] == 7
    dead = GM.make_rec(np.zeros(36), np.zeros(36), logits, np.zeros(36, int), 0, 0.0, 0)
    assert GM.root_action(dead, N, F, W, legal, 0, 50.0, 1.0)[0] is None and GM.final(dead, N, W, [], 50.0, 1.0)[0] == 255


# ---------------------------------------------------------------- the model alone, on the GPU tests' searches
def test_the_model_alone_leaves_out_at_most_two_percent_of_the_random_network_cases():
    import gumbel_cases as C
    left_out = total = 0
    for case in C.RANDOM_CASES:
        m = C.model_search(case, net=C.net_state_dict("random"))
        close = C.close_calls(m)
        left_out += int(close.sum())
        total += len(close)
    assert total >= 100 and left_out <= C.LEFT_OUT_CAP * total, (left_out, total)


# ---------------------------------------------------------------- header, binding table
def test_header_is_plain_c99_and_included_by_qttt_h_after_the_leaves_header():
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_tree_leaves.h"') < src.index('#include "qttt_tree_gumbel.h"')
    prog = ('#include "qttt.h"\nint main(void){\n'
            'int (*b)(const void *, int64_t, int64_t, uint64_t, uint32_t, int64_t, int, const float *, const float *, void *,'
            ' void *) = qttt_tree_gumbel_begin;\n'
            'int (*s)(void *, int64_t, int64_t, uint64_t, uint32_t, int, int64_t, double, double, void *, void *, const void *,'
            ' const int32_t *, int, int, double, double, void *) = qttt_tree_select_batch_gumbel;\n'
            'int (*r)(const void *, const void *, int64_t, int64_t, double, double, uint8_t *, double *, double *, void *)'
            ' = qttt_tree_gumbel_root;\nint (*q)(int, int, int32_t *) = qttt_gumbel_visit_sequence;\n'
            'return b == 0 || s == 0 || r == 0 || q == 0 || QTTT_ABI_VERSION != 6 || QTTT_TREE_GUMBEL_BYTES != 880;}\n')
    for text in (prog, prog.replace('"qttt.h"', '"qttt_tree_gumbel.h"').replace("QTTT_ABI_VERSION", "6")):
        out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c",
                              "-I" + os.path.join(ROOT, "include"), "-"], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr


def test_binding_header_exports_and_build_list_agree():
    import __graft_entry__ as entry
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"^(?:int|int64_t)\s+(qttt_\w+)\s*\(", src, flags=re.M))
    assert names == set(_native.TREE_GUMBEL_SIGNATURES) and len(names) == 7
    assert HEADER in entry.HEADERS
    assert os.path.join(ROOT, "qtttgym_amd", "csrc", "qttt_tree_gumbel_kernels.h") in entry.HEADERS
    L = _native.lib()
    for name in names:
        assert getattr(ctypes.CDLL(_native.LIB_PATH), name)
        assert getattr(L, name).argtypes == _native.TREE_GUMBEL_SIGNATURES[name][1]
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6             # additive entries: the ABI number stays
    assert _native.TREE_GUMBEL_BYTES == GM.REC_DTYPE.itemsize == 880 and _native.TREE_GUMBEL_BASE == GM.GUMBEL_BASE
    assert _native.TREE_MAX_GUMBEL == GM.MAX_GUMBEL and GM.GUMBEL_BASE + 36 * GM.MAX_GUMBEL <= 1 << 32
    assert GM.GUMBEL_BASE > _native.SELFPLAY_MOVE_BASE + _native.SELFPLAY_ROWS
    for doc in ("DESIGN.md", "README.md"):
        assert "qttt_tree_select_batch_gumbel" in open(os.path.join(ROOT, doc)).read(), doc
    assert re.search(r"^## 19\. ", open(os.path.join(ROOT, "DESIGN.md")).read(), flags=re.M)


# ---------------------------------------------------------------- the constructors' checks
def test_python_checks_the_root_policy_before_it_asks_for_a_device():
    from qtttgym_amd import SelfPlay, TreeSearch
    net = object()                    # never looked at: every call fails before
    for cls, kw in ((TreeSearch, dict(capacity=8)), (SelfPlay, dict(n_rollouts=2))):
        with pytest.raises(ValueError, match="root_policy"):
            cls(4, net=net, leaf_eval="value", root_policy="ucb", **kw)
        with pytest.raises(ValueError, match="gumbel"):
            cls(4, net=net, leaf_eval="playouts", root_policy="gumbel", **kw)
        with pytest.raises(ValueError, match="gumbel"):
            cls(4, net=None, root_policy="gumbel", **kw)
        for m in (0, 37, -1):
            with pytest.raises(ValueError, match="max_considered"):
                cls(4, net=net, leaf_eval="value", root_policy="gumbel", max_considered=m, **kw)
        for c in (-1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="c_visit"):
                cls(4, net=net, leaf_eval="value", root_policy="gumbel", c_visit=c, **kw)
        for c in (float("inf"), float("nan")):
            with pytest.raises(ValueError, match="c_scale"):
                cls(4, net=net, leaf_eval="value", root_policy="gumbel", c_scale=c, **kw)
    with pytest.raises(ValueError, match="root_noise"):
        SelfPlay(4, n_rollouts=2, net=net, leaf_eval="value", root_policy="gumbel", root_noise=(0.25, 0.3))
    with pytest.raises(ValueError, match="sample_plies"):
        SelfPlay(4, n_rollouts=2, net=net, leaf_eval="value", root_policy="gumbel", sample_plies=2)
    assert TreeSearch.root_policy == "puct" and TreeSearch.ROOT_POLICIES == ("puct", "gumbel")

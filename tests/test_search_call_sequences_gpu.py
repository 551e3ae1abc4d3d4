"""The order of the library calls of one searched, recorded ply, pinned as literal lists: what TreeSearch.contemplate,
SelfPlay.record, SelfPlay.stream and Reanalyser.run hand to LibCaller._call, entry by entry, for every way to search a root
or to record it.  The lists were taken from the commit before the host-side record / round refactor with this file's own
wrapper; a list that stops matching means that the code changed the launches, never that the list is out of date.

Every configuration is G = 3 games, n_rollouts = 5 and leaves = 2: one single rollout on the fresh roots, two rounds of two,
then the record, which is the smallest shape with all three.  (a) is the exception in one respect: playouts have no
leaf-parallel rounds (TreeSearch rejects leaves > 1 without value leaves), so its five rollouts are five single ones.
(a)-(g) log ply 0 as play() runs it: the new environment and trees, the search, the record, the step, the sync.  (f) is
forced playouts with pruned targets as the keyword alone gives them; f_forced_pruned_noised adds what they are meant for,
root noise and a sampled move.  (h) and (i) log one whole stream() ply of (c) and of (f), both forms, into a ring of 64
samples, (j) one Reanalyser.run() of (f) over a ring that holds one play().
(k)-(n) are the playout cap, the resident search and the TD(lambda) record_value, taken from the commit before the host search
got one plan, one round and one ply, where play_ply spelled the ply out: the search (or _search_capped), record_value, the
record (or record_capped), the step, the sync.  The cap's draw for these values, cap_full_mask(2 * 11 + 1, 0, 3, 0, 0.5), is [0, 1, 0]:
both groups hold a game, which every capped case asserts before it compares, for an empty group launches nothing.
Every case also pins the trees' counters after the ply: (rollout_idx, noise_idx, gumbel_idx, _bound, _fresh)."""
import pytest

import gumbel_cases as C
from tree_harness import DEV

from qtttgym_amd import PolicyValueNet, Reanalyser, ReplayBuffer, SelfPlay
from qtttgym_amd._host import LibCaller, cap_full_mask

pytestmark = pytest.mark.gpu
G, R, K, SEED = 3, 5, 2, 11
_NET = []


def _net():
    if not _NET:
        _NET.append(PolicyValueNet(C.net_state_dict("random"), device=DEV))
    return _NET[0]


class _Log:
    """Every LibCaller._call between __enter__ and __exit__, by entry name, in order."""

    def __enter__(self):
        self.names, self._orig = [], LibCaller._call
        names, orig = self.names, self._orig

        def logged(caller, name, *args):
            names.append(name)
            return orig(caller, name, *args)

        LibCaller._call = logged
        return self.names

    def __exit__(self, *exc):
        LibCaller._call = self._orig


def _value(**kw):
    return dict(net=_net(), leaf_eval="value", leaves=K, **kw)


NOISED = dict(root_noise=(0.25, 0.3), sample_plies=1)
CONFIGS = {
    "a_playouts": lambda: dict(net=None),
    "b_value": lambda: _value(),
    "c_noise_sampled": lambda: _value(**NOISED),
    "d_gumbel": lambda: _value(root_policy="gumbel"),
    "e_exact_prove": lambda: _value(exact_from=6, prove=True),
    "f_forced_pruned": lambda: _value(forced_playouts=2.0),
    "f_forced_pruned_noised": lambda: _value(forced_playouts=2.0, **NOISED),
    "g_eval_symmetries": lambda: _value(eval_symmetries="all"),
    "k_cap": lambda: _value(playout_cap=(0.5, 2), **NOISED),
    "k_cap_forced": lambda: _value(playout_cap=(0.5, 2), forced_playouts=2.0, **NOISED),
    "l_resident": lambda: _value(resident=True, rounds_per_launch=1),
    "m_resident_forced": lambda: _value(resident=True, forced_playouts=2.0, **NOISED),
    "n_td_lambda": lambda: _value(td_lambda=0.5, value_targets=(1.0, -1.0)),
}


def _selfplay(name):
    return SelfPlay(G, n_rollouts=R, seed=SEED, device=DEV, **CONFIGS[name]())


def _counters(tree):
    return (tree.rollout_idx, tree.noise_idx, tree.gumbel_idx, tree._bound, tree._fresh)


def _both_groups(sp):
    """A capped case logs both groups' launches: the draw of ply 0 must put a game in each."""
    if sp.playout_cap is not None:
        full = cap_full_mask(2 * SEED + 1, 0, G, 0, sp.playout_cap[0])
        assert full.tolist() == [0, 1, 0] and 0 < full.sum() < G


def play_ply(name):
    sp = _selfplay(name)
    _both_groups(sp)
    with _Log() as names:
        env, tree = sp._new_game_objects(SEED)
        batch = sp.new_batch()
        sp._ply(env, tree, batch, 0, 0)
    return names, _counters(tree)


def stream_ply(name):
    sp, ring = _selfplay(name), ReplayBuffer(64, device=DEV)
    _both_groups(sp)
    with _Log() as names:
        sp.stream(ring, 1)
    return names, _counters(sp.tree)


def reanalyse_run(name):
    sp, ring = _selfplay(name), ReplayBuffer(64, device=DEV)
    ring.add(sp.play())
    ra = Reanalyser(sp, ring, G)
    with _Log() as names:
        ra.run()
    return names, _counters(ra.tree)


RUNS = {
    "play:a_playouts": (play_ply, "a_playouts", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_rollout_many", "qttt_tree_backup",
        "qttt_tree_select", "qttt_rollout_many", "qttt_tree_backup", "qttt_tree_select", "qttt_rollout_many",
        "qttt_tree_backup", "qttt_tree_select", "qttt_rollout_many", "qttt_tree_backup", "qttt_tree_select",
        "qttt_rollout_many", "qttt_tree_backup", "qttt_selfplay_record", "qttt_env_step", "qttt_tree_sync"], (5, 0, 0, 12, True)),
    "play:b_value": (play_ply, "b_value", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_select_batch",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch", "qttt_evaluate",
        "qttt_tree_backup_batch", "qttt_selfplay_record", "qttt_env_step", "qttt_tree_sync"], (5, 0, 0, 12, True)),
    "play:c_noise_sampled": (play_ply, "c_noise_sampled", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_root_noise",
        "qttt_tree_select_batch", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_sampled", "qttt_env_step", "qttt_tree_sync"], (5, 1, 0, 12, True)),
    "play:d_gumbel": (play_ply, "d_gumbel", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_root_states",
        "qttt_evaluate", "qttt_tree_gumbel_begin", "qttt_tree_select_batch_gumbel", "qttt_evaluate",
        "qttt_tree_backup_batch", "qttt_tree_select_batch_gumbel", "qttt_evaluate", "qttt_tree_backup_batch",
        "qttt_selfplay_record_gumbel", "qttt_env_step", "qttt_tree_sync"], (5, 0, 1, 12, True)),
    "play:e_exact_prove": (play_ply, "e_exact_prove", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select_batch", "qttt_evaluate", "qttt_tree_solve_leaves",
        "qttt_tree_backup_batch_exact", "qttt_tree_prove", "qttt_tree_select_batch", "qttt_evaluate",
        "qttt_tree_solve_leaves", "qttt_tree_backup_batch_exact", "qttt_tree_prove", "qttt_tree_select_batch",
        "qttt_evaluate", "qttt_tree_solve_leaves", "qttt_tree_backup_batch_exact", "qttt_tree_prove",
        "qttt_selfplay_record", "qttt_env_step", "qttt_tree_sync"], (5, 0, 0, 12, True)),
    "play:f_forced_pruned": (play_ply, "f_forced_pruned", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout",
        "qttt_tree_select_batch_forced", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch_forced",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_pruned", "qttt_env_step", "qttt_tree_sync"], (5, 0, 0, 12, True)),
    "play:f_forced_pruned_noised": (play_ply, "f_forced_pruned_noised", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_root_noise",
        "qttt_tree_select_batch_forced", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch_forced",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_pruned", "qttt_env_step", "qttt_tree_sync"], (5, 1, 0, 12, True)),
    "play:g_eval_symmetries": (play_ply, "g_eval_symmetries", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select_batch", "qttt_evaluate_symmetric",
        "qttt_tree_backup_batch", "qttt_tree_select_batch", "qttt_evaluate_symmetric", "qttt_tree_backup_batch",
        "qttt_tree_select_batch", "qttt_evaluate_symmetric", "qttt_tree_backup_batch", "qttt_selfplay_record",
        "qttt_env_step", "qttt_tree_sync"], (5, 0, 0, 12, True)),
    "play:k_cap": (play_ply, "k_cap", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout",
        "qttt_tree_root_noise_subset", "qttt_tree_select_batch_subset", "qttt_evaluate",
        "qttt_tree_backup_batch_subset", "qttt_tree_select_batch_subset", "qttt_evaluate",
        "qttt_tree_backup_batch_subset", "qttt_tree_select_batch_subset", "qttt_evaluate",
        "qttt_tree_backup_batch_subset", "qttt_selfplay_record_capped", "qttt_env_step", "qttt_tree_sync"], (5, 1, 0, 12, True)),
    "play:k_cap_forced": (play_ply, "k_cap_forced", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout",
        "qttt_tree_root_noise_subset", "qttt_tree_select_batch_subset", "qttt_evaluate",
        "qttt_tree_backup_batch_subset", "qttt_tree_select_batch_subset", "qttt_evaluate",
        "qttt_tree_backup_batch_subset", "qttt_tree_select_batch_subset", "qttt_evaluate",
        "qttt_tree_backup_batch_subset", "qttt_selfplay_record_capped", "qttt_env_step", "qttt_tree_sync"], (5, 1, 0, 12, True)),
    "play:l_resident": (play_ply, "l_resident", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_search_resident",
        "qttt_tree_search_resident", "qttt_selfplay_record", "qttt_env_step", "qttt_tree_sync"], (5, 0, 0, 12, True)),
    "play:m_resident_forced": (play_ply, "m_resident_forced", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_root_noise",
        "qttt_tree_search_resident", "qttt_selfplay_record_pruned", "qttt_env_step", "qttt_tree_sync"], (5, 1, 0, 12, True)),
    "play:n_td_lambda": (play_ply, "n_td_lambda", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_select_batch",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch", "qttt_evaluate",
        "qttt_tree_backup_batch", "qttt_selfplay_record_value", "qttt_selfplay_record", "qttt_env_step",
        "qttt_tree_sync"], (5, 0, 0, 12, True)),
    "stream:c_noise_sampled": (stream_ply, "c_noise_sampled", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_root_noise",
        "qttt_tree_select_batch", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_stream_sampled", "qttt_env_step",
        "qttt_tree_sync", "qttt_selfplay_harvest", "qttt_replay_append", "qttt_selfplay_restart"], (5, 1, 0, 100, True)),
    "stream:f_forced_pruned": (stream_ply, "f_forced_pruned", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout",
        "qttt_tree_select_batch_forced", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch_forced",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_stream_pruned", "qttt_env_step",
        "qttt_tree_sync", "qttt_selfplay_harvest", "qttt_replay_append", "qttt_selfplay_restart"], (5, 0, 0, 100, True)),
    "stream:f_forced_pruned_noised": (stream_ply, "f_forced_pruned_noised", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_root_noise",
        "qttt_tree_select_batch_forced", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch_forced",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_stream_pruned", "qttt_env_step",
        "qttt_tree_sync", "qttt_selfplay_harvest", "qttt_replay_append", "qttt_selfplay_restart"], (5, 1, 0, 100, True)),
    "stream:k_cap": (stream_ply, "k_cap", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout",
        "qttt_tree_root_noise_subset", "qttt_tree_select_batch_subset", "qttt_evaluate",
        "qttt_tree_backup_batch_subset", "qttt_tree_select_batch_subset", "qttt_evaluate",
        "qttt_tree_backup_batch_subset", "qttt_tree_select_batch_subset", "qttt_evaluate",
        "qttt_tree_backup_batch_subset", "qttt_selfplay_record_capped", "qttt_env_step", "qttt_tree_sync",
        "qttt_selfplay_harvest_capped", "qttt_replay_append", "qttt_selfplay_restart"], (5, 1, 0, 100, True)),
    "stream:k_cap_forced": (stream_ply, "k_cap_forced", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout",
        "qttt_tree_root_noise_subset", "qttt_tree_select_batch_subset", "qttt_evaluate",
        "qttt_tree_backup_batch_subset", "qttt_tree_select_batch_subset", "qttt_evaluate",
        "qttt_tree_backup_batch_subset", "qttt_tree_select_batch_subset", "qttt_evaluate",
        "qttt_tree_backup_batch_subset", "qttt_selfplay_record_capped", "qttt_env_step", "qttt_tree_sync",
        "qttt_selfplay_harvest_capped", "qttt_replay_append", "qttt_selfplay_restart"], (5, 1, 0, 100, True)),
    "reanalyse:f_forced_pruned": (reanalyse_run, "f_forced_pruned", [
        "qttt_replay_gather", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout",
        "qttt_tree_select_batch_forced", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch_forced",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_pruned", "qttt_replay_update"], (5, 0, 0, 11, False)),
}


@pytest.mark.parametrize("case", sorted(RUNS))
def test_call_sequence_is_the_parents(case):
    run, name, want, counters = RUNS[case]
    got = run(name)
    print(case, got)
    assert got == (want, counters), (case, got)

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
samples, (j) one Reanalyser.run() of (f) over a ring that holds one play()."""
import pytest

import gumbel_cases as C
from tree_harness import DEV

from qtttgym_amd import PolicyValueNet, Reanalyser, ReplayBuffer, SelfPlay
from qtttgym_amd._host import LibCaller

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
}


def _selfplay(name):
    return SelfPlay(G, n_rollouts=R, seed=SEED, device=DEV, **CONFIGS[name]())


def play_ply(name):
    sp = _selfplay(name)
    with _Log() as names:
        env, tree = sp._new_game_objects(SEED)
        batch = sp.new_batch()
        sp._search(tree)
        env.step_raw(sp.record(tree, 0, batch))
        tree.sync(env)
    return names


def stream_ply(name):
    sp, ring = _selfplay(name), ReplayBuffer(64, device=DEV)
    with _Log() as names:
        sp.stream(ring, 1)
    return names


def reanalyse_run(name):
    sp, ring = _selfplay(name), ReplayBuffer(64, device=DEV)
    ring.add(sp.play())
    ra = Reanalyser(sp, ring, G)
    with _Log() as names:
        ra.run()
    return names


RUNS = {
    "play:a_playouts": (play_ply, "a_playouts", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_rollout_many", "qttt_tree_backup",
        "qttt_tree_select", "qttt_rollout_many", "qttt_tree_backup", "qttt_tree_select", "qttt_rollout_many",
        "qttt_tree_backup", "qttt_tree_select", "qttt_rollout_many", "qttt_tree_backup", "qttt_tree_select",
        "qttt_rollout_many", "qttt_tree_backup", "qttt_selfplay_record", "qttt_env_step", "qttt_tree_sync"]),
    "play:b_value": (play_ply, "b_value", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_select_batch",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch", "qttt_evaluate",
        "qttt_tree_backup_batch", "qttt_selfplay_record", "qttt_env_step", "qttt_tree_sync"]),
    "play:c_noise_sampled": (play_ply, "c_noise_sampled", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_root_noise",
        "qttt_tree_select_batch", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_sampled", "qttt_env_step", "qttt_tree_sync"]),
    "play:d_gumbel": (play_ply, "d_gumbel", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_root_states",
        "qttt_evaluate", "qttt_tree_gumbel_begin", "qttt_tree_select_batch_gumbel", "qttt_evaluate",
        "qttt_tree_backup_batch", "qttt_tree_select_batch_gumbel", "qttt_evaluate", "qttt_tree_backup_batch",
        "qttt_selfplay_record_gumbel", "qttt_env_step", "qttt_tree_sync"]),
    "play:e_exact_prove": (play_ply, "e_exact_prove", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select_batch", "qttt_evaluate", "qttt_tree_solve_leaves",
        "qttt_tree_backup_batch_exact", "qttt_tree_prove", "qttt_tree_select_batch", "qttt_evaluate",
        "qttt_tree_solve_leaves", "qttt_tree_backup_batch_exact", "qttt_tree_prove", "qttt_tree_select_batch",
        "qttt_evaluate", "qttt_tree_solve_leaves", "qttt_tree_backup_batch_exact", "qttt_tree_prove",
        "qttt_selfplay_record", "qttt_env_step", "qttt_tree_sync"]),
    "play:f_forced_pruned": (play_ply, "f_forced_pruned", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout",
        "qttt_tree_select_batch_forced", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch_forced",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_pruned", "qttt_env_step", "qttt_tree_sync"]),
    "play:f_forced_pruned_noised": (play_ply, "f_forced_pruned_noised", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_root_noise",
        "qttt_tree_select_batch_forced", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch_forced",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_pruned", "qttt_env_step", "qttt_tree_sync"]),
    "play:g_eval_symmetries": (play_ply, "g_eval_symmetries", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select_batch", "qttt_evaluate_symmetric",
        "qttt_tree_backup_batch", "qttt_tree_select_batch", "qttt_evaluate_symmetric", "qttt_tree_backup_batch",
        "qttt_tree_select_batch", "qttt_evaluate_symmetric", "qttt_tree_backup_batch", "qttt_selfplay_record",
        "qttt_env_step", "qttt_tree_sync"]),
    "stream:c_noise_sampled": (stream_ply, "c_noise_sampled", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_root_noise",
        "qttt_tree_select_batch", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_stream_sampled", "qttt_env_step",
        "qttt_tree_sync", "qttt_selfplay_harvest", "qttt_replay_append", "qttt_selfplay_restart"]),
    "stream:f_forced_pruned": (stream_ply, "f_forced_pruned", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout",
        "qttt_tree_select_batch_forced", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch_forced",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_stream_pruned", "qttt_env_step",
        "qttt_tree_sync", "qttt_selfplay_harvest", "qttt_replay_append", "qttt_selfplay_restart"]),
    "stream:f_forced_pruned_noised": (stream_ply, "f_forced_pruned_noised", [
        "qttt_reset", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout", "qttt_tree_root_noise",
        "qttt_tree_select_batch_forced", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch_forced",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_stream_pruned", "qttt_env_step",
        "qttt_tree_sync", "qttt_selfplay_harvest", "qttt_replay_append", "qttt_selfplay_restart"]),
    "reanalyse:f_forced_pruned": (reanalyse_run, "f_forced_pruned", [
        "qttt_replay_gather", "qttt_tree_reset", "qttt_tree_select", "qttt_tree_value_rollout",
        "qttt_tree_select_batch_forced", "qttt_evaluate", "qttt_tree_backup_batch", "qttt_tree_select_batch_forced",
        "qttt_evaluate", "qttt_tree_backup_batch", "qttt_selfplay_record_pruned", "qttt_replay_update"]),
}


@pytest.mark.parametrize("case", sorted(RUNS))
def test_call_sequence_is_the_parents(case):
    run, name, want = RUNS[case]
    got = run(name)
    assert got == want, (case, got)

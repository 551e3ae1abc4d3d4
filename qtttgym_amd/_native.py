"""ctypes binding of libqttt_hip.so (include/qttt.h).  There is no CPU fallback: if the HIP
library is missing or a call fails, this raises."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# QTTT_LIB_PATH: load another build of the same ABI (A/B diagnostics); default = the in-tree build
LIB_PATH = os.environ.get("QTTT_LIB_PATH") or os.path.join(_HERE, "libqttt_hip.so")

ABI_VERSION = 6
FLAG_AUTO_RESET = 1
FLAG_FUSED = 2
BOARD_RECORD_BYTES = 64
SIM_STRIDE = 16
EXPAND_ROLLOUT_MAX_SIMS = 128
OP_MAKE_MOVE, OP_UPDATE_QSTRUCTS, OP_CHECK_WIN = 0, 1, 2
NN_F32, NN_BF16 = 0, 1
POLICY_ROLLOUT_MAX_SIMS = 128
TREE_GAME_BYTES, TREE_NODE_BYTES, TREE_PRIOR_BYTES = 128, 608, 144
TREE_MAX_DEPTH = 10
TREE_MAX_CAPACITY = 1 << 30
TREE_MAX_SIMS = 128
TREE_MAX_ROLLOUTS = 1 << 24
TREE_SELECT_BASE = 1 << 31

class EnvRecord(ctypes.Structure):
    """include/qttt.h: struct qttt_env."""
    _fields_ = [("state", ctypes.c_void_p), ("n", ctypes.c_int64), ("board_offset", ctypes.c_int64),
                ("seed", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("reward", ctypes.c_void_p), ("terminated", ctypes.c_void_p), ("classical", ctypes.c_void_p),
                ("q_p1", ctypes.c_void_p), ("q_p1_len", ctypes.c_void_p), ("q_p2", ctypes.c_void_p),
                ("q_p2_len", ctypes.c_void_p), ("turn", ctypes.c_void_p), ("step_counter", ctypes.c_void_p)]


ENV_STEP, ENV_STEP_OBSERVE, ENV_STEP_RANDOM, ENV_SAMPLE = 0, 1, 2, 3

# every symbol include/qttt.h declares: name -> (restype, argtypes)
_vp, _i32, _i64, _u64, _u32 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64,
                               ctypes.c_uint32)
SIGNATURES = {
    "qttt_abi_version": (_i32, []),
    "qttt_state_bytes": (_i64, [_i64]),
    "qttt_reset": (_i32, [_vp, _i64, _vp]),
    "qttt_reset_observe": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "qttt_step": (_i32, [_vp, _vp, _vp, _u64, _u32, _i64, _u32, _vp, _vp, _i64, _vp]),
    "qttt_step_observe": (_i32, [_vp, _vp, _vp, _u64, _u32, _i64, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _i64, _vp]),
    "qttt_step_many": (_i32, [_vp, _vp, _vp, _u64, _u32, _i64, _u32, _vp, _vp, _i64, _i64, _i32, _vp]),
    "qttt_step_random_many": (_i32, [_vp, _u64, _u32, _i64, _u32, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp]),
    "qttt_observe": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "qttt_check_win": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "qttt_export": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "qttt_import": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "qttt_board_op": (_i32, [_vp, _vp, _i64, _vp]),
    "qttt_board_op_sync": (_i32, [_vp, _vp, _i64, _vp]),
    "qttt_board_op_host": (_i32, [_vp, _vp, _i64, _vp]),
    "qttt_board_mailbox_retire": (_i32, [_i32]),
    "qttt_sample_actions": (_i32, [_vp, _u64, _u32, _i64, _u32, _vp, _i64, _vp]),
    "qttt_node_info": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "qttt_state_key": (_u64, [_u64, _u64]),
    "qttt_expand": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "qttt_expand_rollout": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u32, _i64, _i32, _vp, _vp,
                                   _i64, _vp]),
    "qttt_rollout": (_i32, [_vp, _u64, _u32, _i64, _vp, _vp, _vp, _i64, _vp]),
    "qttt_rollout_many": (_i32, [_vp, _u64, _u32, _i64, _i32, _vp, _vp, _i64, _vp]),
    "qttt_encode": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "qttt_set_tuning": (_i32, [_i32, _i32]),
    "qttt_step_launch_shape": (_i32, [_i64, _u32, _i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "qttt_env_step": (_i32, [ctypes.POINTER(EnvRecord), _vp, _vp, _u32, _i32, _vp]),
    "qttt_counter_add": (_i32, [_vp, _u32, _vp]),
    "qttt_step_random": (_i32, [_vp, _u64, _u32, _i64, _u32, _vp, _vp, _vp, _i64, _vp]),
    "qttt_hash": (_u64, [_u64, _u64, _u32]),
}
# every symbol include/qttt_nn.h declares (the policy/value network, ABI 6; qttt.h includes it)
NN_SIGNATURES = {
    "qttt_nn_weights_bytes": (_i64, [_i32]),
    "qttt_evaluate": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp]),
}
# every symbol include/qttt_policy_rollout.h declares (network-guided playouts; qttt.h includes it)
POLICY_ROLLOUT_SIGNATURES = {
    "qttt_rollout_policy": (_i32, [_vp, _vp, _i32, _u64, _u32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
}

# every symbol include/qttt_tree.h declares (the batched search trees; qttt.h includes it)
_f64 = ctypes.c_double
TREE_SIGNATURES = {
    "qttt_tree_bytes": (_i64, [_i64, _i64]),
    "qttt_tree_reset": (_i32, [_vp, _i64, _i64, _vp, _vp]),
    "qttt_tree_select": (_i32, [_vp, _i64, _i64, _u64, _u32, _i64, _f64, _vp, _vp]),
    "qttt_tree_backup": (_i32, [_vp, _i64, _i64, _vp, _i32, _vp, _vp]),
    "qttt_tree_sync": (_i32, [_vp, _i64, _i64, _vp, _vp]),
    "qttt_tree_root": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qttt_tree_sqrt": (_i32, [_u32, _i64, _vp, _vp]),
    "qttt_tree_score": (_i32, [_vp, _vp, _vp, _vp, _f64, _i64, _vp, _vp]),
}
# every symbol include/qttt_tree_compact.h declares (compaction of the search trees; qttt.h includes it)
TREE_COMPACT_SIGNATURES = {
    "qttt_tree_compact_bytes": (_i64, [_i64, _i64]),
    "qttt_tree_compact": (_i32, [_vp, _i64, _i64, _vp, _vp]),
}
# every symbol include/qttt_selfplay.h declares (the self-play record; qttt.h includes it)
SELFPLAY_ROWS = 10
SELFPLAY_SIGNATURES = {
    "qttt_selfplay_record": (_i32, [_vp, _i64, _i64, _i32, _u32, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp]),
}
# every symbol include/qttt_symmetry.h declares (the board's symmetries; qttt.h includes it)
SYMMETRIES = 8
_u8p = ctypes.POINTER(ctypes.c_uint8)
SYMMETRY_SIGNATURES = {
    "qttt_symmetry_tables": (_i32, [_u8p, _u8p, _u8p, _u8p]),
    "qttt_transform": (_i32, [_vp, _vp, _vp, _i32, _i64, _vp]),
    "qttt_selfplay_augment": (_i32, [_i64, _u8p, _i32] + [_vp] * 18 + [_vp]),
}
# every symbol include/qttt_tree_value.h declares (the value rollout of the search trees; qttt.h includes it)
TREE_VALUE_SIGNATURES = {
    "qttt_tree_value_rollout": (_i32, [_vp, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _vp]),
}
# every symbol include/qttt_tree_leaves.h declares (leaf-parallel rounds of the search trees; qttt.h includes it)
TREE_MAX_LEAVES = 64
TREE_PATH_BYTES = 64
TREE_LEAVES_SIGNATURES = {
    "qttt_tree_paths_bytes": (_i64, [_i64, _i32]),
    "qttt_tree_select_batch": (_i32, [_vp, _i64, _i64, _u64, _u32, _i32, _i64, _f64, _f64, _vp, _vp, _vp]),
    "qttt_tree_backup_batch": (_i32, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
}
# every symbol include/qttt_tree_explore.h declares (root exploration: Dirichlet noise, the sampled move; qttt.h
# includes it)
TREE_NOISE_BASE = 0xC0000000
TREE_NOISE_TRIES = 16
TREE_NOISE_DRAWS = 2 * TREE_NOISE_TRIES + 1
SELFPLAY_MOVE_BASE = 0xE0000000
TREE_MAX_NOISE = (SELFPLAY_MOVE_BASE - TREE_NOISE_BASE) // (36 * TREE_NOISE_DRAWS)
TREE_EXPLORE_SIGNATURES = {
    "qttt_tree_root_noise": (_i32, [_vp, _i64, _i64, _u64, _u32, _i64, _f64, _f64, _vp, _vp, _vp]),
    "qttt_selfplay_record_sampled": (_i32, SELFPLAY_SIGNATURES["qttt_selfplay_record"][1][:-1]
                                     + [_u64, _i64, _f64, _i32, _vp]),
}
# every symbol include/qttt_nn_symmetric.h declares (the network averaged over a position's symmetries; qttt.h
# includes it)
NN_SYMMETRIC_SIZES = (1, 2, 4, 8)
NN_SYMMETRIC_SIGNATURES = {
    "qttt_evaluate_symmetric": (_i32, [_vp, _vp, _i32, _u8p, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
}
# every symbol include/qttt_tree_gumbel.h declares (the Gumbel root of the search trees; qttt.h includes it)
TREE_GUMBEL_BYTES = 880
TREE_GUMBEL_BASE = 0xF0000000
TREE_MAX_GUMBEL = 0x10000000 // 36
TREE_GUMBEL_SIGNATURES = {
    "qttt_tree_gumbel_bytes": (_i64, [_i64]),
    "qttt_gumbel_visit_sequence": (_i32, [_i32, _i32, _vp]),
    "qttt_tree_root_states": (_i32, [_vp, _i64, _i64, _vp, _vp]),
    "qttt_tree_gumbel_begin": (_i32, [_vp, _i64, _i64, _u64, _u32, _i64, _i32, _vp, _vp, _vp, _vp]),
    "qttt_tree_select_batch_gumbel": (_i32, TREE_LEAVES_SIGNATURES["qttt_tree_select_batch"][1][:-1]
                                      + [_vp, _vp, _i32, _i32, _f64, _f64, _vp]),
    "qttt_tree_gumbel_root": (_i32, [_vp, _vp, _i64, _i64, _f64, _f64, _vp, _vp, _vp, _vp]),
    "qttt_selfplay_record_gumbel": (_i32, SELFPLAY_SIGNATURES["qttt_selfplay_record"][1][:-1] + [_vp, _f64, _f64, _vp]),
}
# every symbol include/qttt_replay.h declares (the replay ring: append self-play, sample minibatches; qttt.h includes it)
REPLAY_MAX_CAPACITY = 1 << 30
REPLAY_MAX_GAMES = 1 << 30
REPLAY_SCAN_BLOCK = 256
REPLAY_ARRAYS = ("P", "Q", "pi", "mask", "v", "done")          # the order of qttt_replay_layout's offsets
REPLAY_SIGNATURES = {
    "qttt_replay_bytes": (_i64, [_i64]),
    "qttt_replay_layout": (_i32, [_i64, ctypes.POINTER(ctypes.c_int64)]),
    "qttt_replay_append_scratch_bytes": (_i64, [_i64]),
    "qttt_replay_append": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qttt_replay_sample": (_i32, [_vp, _i64, _i64, _u64, _u32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# every symbol include/qttt_train.h declares (the training step: loss, gradients, AMSGrad on the f32 blob; qttt.h includes it)
TRAIN_CHUNK = 256
TRAIN_MAX_SAMPLES = 1 << 24
_f32 = ctypes.c_float
TRAIN_SIGNATURES = {
    "qttt_train_workspace_bytes": (_i64, [_i64]),
    "qttt_train_gradients": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qttt_train_adam": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _vp, _vp]),
}
# every symbol include/qttt_selfplay_stream.h declares (continuous self-play: the per-game record, harvest, restart; qttt.h
# includes it)
SELFPLAY_MAX_MOVE_DRAWS = 1 << 28
SELFPLAY_TALLIES = 4
_RECORD_STREAM = [a for i, a in enumerate(SELFPLAY_SIGNATURES["qttt_selfplay_record"][1][:-1]) if i != 3]    # no ply
SELFPLAY_STREAM_SIGNATURES = {
    "qttt_selfplay_record_stream": (_i32, _RECORD_STREAM + [_vp]),
    "qttt_selfplay_record_stream_sampled": (_i32, _RECORD_STREAM + [_u64, _i64, _f64, _i32, _u32, _vp]),
    "qttt_selfplay_record_stream_gumbel": (_i32, _RECORD_STREAM + [_vp, _f64, _f64, _vp]),
    "qttt_selfplay_harvest": (_i32, [_vp, _i64, _i64, _f64, _f64] + [_vp] * 13 + [_vp]),
    "qttt_selfplay_restart": (_i32, [_vp, _i64, _i64, _vp, _vp] + [_vp] * 7 + [_vp]),
}
# every symbol include/qttt_solve.h declares (the exact endgame solver; qttt.h includes it)
SOLVE_MIN_PLY, SOLVE_MAX_PLY = 4, 9
SOLVE_DENOMINATOR = 16
SOLVE_SIGNATURES = {
    "qttt_solve": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# every symbol include/qttt_tree_exact.h declares (exact leaves in the search trees; qttt.h includes it)
TREE_EXACT_MIN_PLY = 6
TREE_NODE_SOLVED = 1 << 4
TREE_NODE_VALUE_SHIFT = 16
TREE_NODE_VALUE_MASK = 63 << TREE_NODE_VALUE_SHIFT
TREE_EXACT_SIGNATURES = {
    "qttt_tree_solve_leaves": (_i32, [_vp, _i64, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "qttt_tree_backup_batch_exact": TREE_LEAVES_SIGNATURES["qttt_tree_backup_batch"],
}
# every symbol include/qttt_tree_prove.h declares (proven interior nodes of the search trees; qttt.h includes it)
TREE_PROVE_SIGNATURES = {
    "qttt_tree_prove": (_i32, [_vp, _i64, _i64, _i32, _vp, _vp, _vp]),
    "qttt_tree_root_exact": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
}
# every symbol include/qttt_selfplay_exact.h declares (exact targets for the late rows of a self-play batch; qttt.h includes it)
SELFPLAY_EXACT_MIN_PLY, SELFPLAY_EXACT_MAX_PLY = 6, 9
SELFPLAY_EXACT_SIGNATURES = {
    "qttt_selfplay_exact_targets": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# every symbol include/qttt_replay_reanalyse.h declares (reanalysis: a window of the ring as a state buffer, the guarded
# write-back of refreshed targets; qttt.h includes it)
REPLAY_WINDOW_ID = 1 << 32
REPLAY_REANALYSE_SIGNATURES = {
    "qttt_replay_gather": (_i32, [_vp, _i64, _i64, _u64, _u32, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qttt_replay_update": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# every symbol include/qttt_replay_priority.h declares (prioritised replay: the priority table beside the ring, its sync,
# the guarded write-back, the proportional draw; qttt.h includes it)
PRIORITY_ONE = 1 << 16
PRIORITY_HEADER_BYTES = 64
PRIORITY_MAX_LEVELS = 4
REPLAY_PRIORITY_SIGNATURES = {
    "qttt_replay_priority_bytes": (_i64, [_i64]),
    "qttt_replay_priority_layout": (_i32, [_i64, ctypes.POINTER(ctypes.c_int64)]),
    "qttt_replay_priority_sync": (_i32, [_vp, _vp, _i64, _vp]),
    "qttt_replay_priority_update": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "qttt_replay_sample_prioritized": (_i32, [_vp, _vp, _i64, _i64, _u64, _u32, _vp, _i32] + [_vp] * 10 + [_vp]),
}
# every symbol include/qttt_train_weighted.h declares (importance weights in the training step's loss; qttt.h includes it)
TRAIN_WEIGHTED_SIGNATURES = {
    "qttt_train_gradients_weighted": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# every symbol include/qttt_selfplay_value.h declares (search-value targets for self-play: the roots' searched value and the
# value targets made of it; qttt.h includes it)
VALUE_MIX, VALUE_TD = 0, 1
SELFPLAY_VALUE_SIGNATURES = {
    "qttt_selfplay_record_value": (_i32, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "qttt_selfplay_value_targets": (_i32, [_i64, _i32, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# every symbol include/qttt_tree_forced.h declares (forced playouts at the root and policy target pruning; qttt.h includes it)
TREE_FORCED_SIGNATURES = {
    "qttt_tree_select_batch_forced": (_i32, TREE_LEAVES_SIGNATURES["qttt_tree_select_batch"][1][:-1] + [_f64, _vp]),
    "qttt_tree_root_forced": (_i32, [_vp, _i64, _i64, _f64, _f64, _vp, _vp, _vp]),
    "qttt_selfplay_record_pruned": (_i32, TREE_EXPLORE_SIGNATURES["qttt_selfplay_record_sampled"][1][:-1] + [_f64, _f64, _vp]),
    "qttt_selfplay_record_stream_pruned": (_i32, SELFPLAY_STREAM_SIGNATURES["qttt_selfplay_record_stream_sampled"][1][:-1]
                                           + [_f64, _f64, _vp]),
}
# every symbol include/qttt_tree_subset.h declares (rounds and root noise for a listed subset of the games; qttt.h includes it)
_i32p = ctypes.c_void_p                 # const int32_t *ids: a device address
TREE_SUBSET_SIGNATURES = {
    "qttt_tree_select_batch_subset": (_i32, [_vp, _i64, _i64, _u64, _u32, _i32, _i64, _f64, _f64, _f64, _i32p, _i64, _vp, _vp,
                                             _vp]),
    "qttt_tree_backup_batch_subset": (_i32, [_vp, _i64, _i64, _i32, _i32p, _i64, _vp, _vp, _vp, _vp]),
    "qttt_tree_root_noise_subset": (_i32, [_vp, _i64, _i64, _u64, _u32, _i64, _f64, _f64, _i32p, _i64, _vp, _vp, _vp]),
}
# every symbol include/qttt_selfplay_cap.h declares (the record and harvest of playout cap randomisation; qttt.h includes it)
SELFPLAY_CAP_BASE = 0xA0000000
SELFPLAY_MAX_CAP_DRAWS = 1 << 28
SELFPLAY_CAP_SIGNATURES = {
    "qttt_selfplay_record_capped": (_i32, TREE_FORCED_SIGNATURES["qttt_selfplay_record_stream_pruned"][1][:-1] + [_vp, _vp]),
    "qttt_selfplay_harvest_capped": SELFPLAY_STREAM_SIGNATURES["qttt_selfplay_harvest"],
}
# every symbol include/qttt_tree_resident.h declares (the resident search: every round of a move in one launch; qttt.h
# includes it)
TREE_RESIDENT_SIGNATURES = {
    "qttt_tree_search_resident": (_i32, [_vp, _i64, _i64, _u64, _u32, _i32, _u32, _i64, _f64, _f64, _f64, _vp, _i32, _vp]),
    "qttt_tree_resident_games_per_group": (_i32, [_i32, _i32]),
    "qttt_tree_resident_plan": (_i32, [_i32, _u32, _vp, _i32]),
}

_lib = None

# Process settings the measurements of this repo were made with.  Importing the package does NOT touch os.environ
# (an embedding host owns its environment): a launcher calls recommended_env(apply=True) before anything initialises
# HIP, or exports the variables itself.  INTEGRATION.md §3.
RECOMMENDED_ENV = {
    # kernel arguments placed in device memory: ROCm 7.2's default on MI355X, read when the HIP runtime starts.  Worth
    # 1.2 us per launch (tools/stepbench, profiles/r04/kernarg_placement.txt: 7.13 us with it, 8.32 without at 1 M
    # boards; 3.80 / 4.77 at 262 144)
    "HIP_FORCE_DEV_KERNARG": "1",
    # multi-process RCCL / tensor sharing on this pool needs dmabuf IPC
    "HSA_ENABLE_IPC_MODE_LEGACY": "0",
}


def recommended_env(apply=False):
    """The environment variables bench.py / the examples run with, as a dict.  apply=True sets those that the process
    has not set itself (os.environ.setdefault) — call it before the first HIP call (torch.cuda.*, lib()): the HIP
    runtime reads them once, when it starts."""
    if apply:
        for k, v in RECOMMENDED_ENV.items():
            os.environ.setdefault(k, v)
    return dict(RECOMMENDED_ENV)


def flag_shape(boards_per_lane=0, workgroup_size=0):
    """include/qttt.h QTTT_FLAG_SHAPE: the launch shape carried by one call's flags (0 = the library's choice)."""
    if boards_per_lane not in (0, 1, 2, 4) or workgroup_size not in (0, 256, 512, 1024):
        raise ValueError("boards per lane 0|1|2|4 and workgroup size 0|256|512|1024")
    return (boards_per_lane << 8) | ({0: 0, 256: 1, 512: 2, 1024: 3}[workgroup_size] << 12)


def step_launch_shape(n, flags=0, observe=False):
    """(boards per lane, workgroup size) a step call with these flags uses for a batch of n boards."""
    bpl, blk = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().qttt_step_launch_shape(int(n), int(flags), int(bool(observe)), ctypes.byref(bpl), ctypes.byref(blk)),
          "qttt_step_launch_shape")
    return bpl.value, blk.value


class QtttNativeError(RuntimeError):
    pass


def retire_mailbox(wait=True):
    """include/qttt.h qttt_board_mailbox_retire: asks the resident wave behind the single-board façades (Board.make_move,
    Env.step) to leave now — before a device-wide synchronise, or before handing the GPU to something else.  A no-op when
    none is resident; the next Board / Env call launches it again."""
    check(lib().qttt_board_mailbox_retire(1 if wait else 0), "qttt_board_mailbox_retire")


def lib():
    """Loads the HIP library (once).  Raises QtttNativeError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QtttNativeError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in (list(SIGNATURES.items()) + list(NN_SIGNATURES.items())
                                  + list(POLICY_ROLLOUT_SIGNATURES.items()) + list(TREE_SIGNATURES.items())
                                  + list(TREE_COMPACT_SIGNATURES.items()) + list(SELFPLAY_SIGNATURES.items())
                                  + list(SYMMETRY_SIGNATURES.items()) + list(TREE_VALUE_SIGNATURES.items())
                                  + list(TREE_EXPLORE_SIGNATURES.items()) + list(TREE_LEAVES_SIGNATURES.items())
                                  + list(NN_SYMMETRIC_SIGNATURES.items()) + list(TREE_GUMBEL_SIGNATURES.items())
                                  + list(REPLAY_SIGNATURES.items()) + list(TRAIN_SIGNATURES.items())
                                  + list(SELFPLAY_STREAM_SIGNATURES.items()) + list(SOLVE_SIGNATURES.items())
                                  + list(TREE_EXACT_SIGNATURES.items()) + list(SELFPLAY_EXACT_SIGNATURES.items())
                                  + list(TREE_PROVE_SIGNATURES.items()) + list(REPLAY_REANALYSE_SIGNATURES.items())
                                  + list(REPLAY_PRIORITY_SIGNATURES.items()) + list(TRAIN_WEIGHTED_SIGNATURES.items())
                                  + list(SELFPLAY_VALUE_SIGNATURES.items()) + list(TREE_FORCED_SIGNATURES.items())
                                  + list(TREE_SUBSET_SIGNATURES.items()) + list(SELFPLAY_CAP_SIGNATURES.items())
                                  + list(TREE_RESIDENT_SIGNATURES.items())):
            try:
                fn = getattr(L, name)
            except AttributeError:
                raise QtttNativeError("%s does not export %s (stale build?)" % (LIB_PATH, name)) from None
            fn.restype = res
            fn.argtypes = args
        if L.qttt_abi_version() != ABI_VERSION:
            raise QtttNativeError("libqttt_hip.so ABI %d != expected %d (stale build?)"
                                  % (L.qttt_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


_ARG_ERRORS = {-1: "null pointer", -2: "bad size / offset", -3: "misaligned actions"}


def check(rc, what):
    if rc != 0:
        if rc < 0:
            raise QtttNativeError("%s: argument error %d (%s)" % (what, rc, _ARG_ERRORS.get(rc, "?")))
        raise QtttNativeError("%s: hipError_t %d" % (what, rc))

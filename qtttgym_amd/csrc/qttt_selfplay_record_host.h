// qttt_selfplay_record_host.h — plain C++ without HIP: the argument checks of the eight self-play record entries and of the
// three leaf-parallel selects (include/qttt_selfplay.h, qttt_selfplay_stream.h, qttt_tree_leaves.h, qttt_tree_explore.h,
// qttt_tree_gumbel.h, qttt_tree_forced.h), one function each, in the order include/qttt.h promises: a mode or a root rule adds
// its own tests to the common ones.  tools/forced_host_check.cpp calls both with every class of bad argument.
#ifndef QTTT_SELFPLAY_RECORD_HOST_H
#define QTTT_SELFPLAY_RECORD_HOST_H
#include "qttt_checks.h"
#include "qttt_tree_forced_host.h"

namespace {

constexpr int RECORD_PLAIN = 0, RECORD_SAMPLED = 1, RECORD_GUMBEL = 2, RECORD_PRUNED = 3;      // selfplay_record_kernel's MODE
constexpr int SELECT_PUCT = 0, SELECT_GUMBEL = 1, SELECT_FORCED = 2;                           // the root rule of a select

// the scales of sigma (include/qttt_tree_gumbel.h): c_visit finite and >= 0, c_scale finite
inline bool gumbel_scale_bad(double c_visit, double c_scale) { return !is_finite(c_visit) || c_visit < 0.0 || !is_finite(c_scale); }

// the tree and the nine outputs of a record, every one required
struct RecordArgs {
    const void *tree, *states, *pi, *mask, *done, *v, *action36, *length, *winner, *actions;
};
// what a mode takes besides; a mode looks at its own fields only
struct RecordExtra {
    int64_t board_offset;              // the sampled and the pruned record: these three
    double temperature;
    int sample_plies;
    double forced_k, c_puct;           // the pruned record
    const void *rec;                   // the Gumbel record: rec (required, 16-byte aligned) and the scales
    double c_visit, c_scale;
    bool capped;                       // the capped record (include/qttt_selfplay_cap.h): full is required
    const void *full;
};

// The lockstep record (stream = false) tests ply in 0..9; the stream record has no ply, and tests draw_index below its bound
// in the modes that draw a move (sampled, pruned).  The Gumbel record uses neither n_rollouts nor alpha and tests neither.
// `work`: the call has something to launch (games > 0).
inline int record_check(int mode, bool stream, const RecordArgs &p, int64_t games, int64_t capacity, int ply, uint32_t draw_index,
                        uint32_t n_rollouts, double alpha, double v_first, double v_second, const RecordExtra &x, bool &work) {
    const bool draws = mode == RECORD_SAMPLED || mode == RECORD_PRUNED, gumbel = mode == RECORD_GUMBEL;
    work = false;
    if (tree_size_bad(games, capacity) || !is_finite(v_first) || !is_finite(v_second) ||
        (!stream && (ply < 0 || ply >= QTTT_SELFPLAY_ROWS)) || (stream && draws && draw_index >= QTTT_SELFPLAY_MAX_MOVE_DRAWS) ||
        (!gumbel && (n_rollouts == 0u || !is_finite(alpha) || alpha <= 0.0)) ||
        (draws && (x.board_offset < 0 || !is_finite(x.temperature) || x.temperature <= 0.0 || x.sample_plies < 0 ||
                   x.sample_plies > QTTT_SELFPLAY_ROWS)) ||
        (mode == RECORD_PRUNED && (forced_k_bad(x.forced_k) || !is_finite(x.c_puct))) || (gumbel && gumbel_scale_bad(x.c_visit, x.c_scale)))
        return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(p.tree, p.states, p.pi, p.mask, p.done, p.v, p.action36, p.length, p.winner, p.actions) || (gumbel && !x.rec) ||
        (x.capped && !x.full))
        return QTTT_ERR_NULL;
    if (misaligned(p.tree, 16) || misaligned(p.states, 16) || misaligned(p.pi, 8) || misaligned(p.v, 4) ||
        (gumbel && misaligned(x.rec, 16)))
        return QTTT_ERR_ACTION;
    work = true;
    return 0;
}

// what a root rule takes besides
struct SelectExtra {
    double forced_k;                   // the forced select
    const void *rec, *visit_table;     // the Gumbel select: both required, 16- and 4-byte aligned
    int n_sims, sim_idx0;
    double c_visit, c_scale;
};

inline int select_batch_check(int rule, const void *tree, int64_t games, int64_t capacity, uint32_t rollout_idx0, int leaves,
                              int64_t board_offset, double virtual_loss, const void *paths, const void *leaf_state,
                              const SelectExtra &x, bool &work) {
    const bool gumbel = rule == SELECT_GUMBEL;
    work = false;
    if (tree_size_bad(games, capacity) || board_offset < 0 || tree_leaves_bad(games, leaves) ||
        (uint64_t)rollout_idx0 + (uint64_t)leaves > QTTT_TREE_MAX_ROLLOUTS || !is_finite(virtual_loss) || virtual_loss < 0.0 ||
        (gumbel && (x.n_sims < 1 || x.n_sims > QTTT_TREE_MAX_ROLLOUTS || x.sim_idx0 < 0 || (int64_t)x.sim_idx0 + leaves > x.n_sims ||
                    gumbel_scale_bad(x.c_visit, x.c_scale))) ||
        (rule == SELECT_FORCED && forced_k_bad(x.forced_k)))
        return QTTT_ERR_SIZE;
    if (games == 0) return 0;
    if (any_null(tree, paths, leaf_state) || (gumbel && any_null(x.rec, x.visit_table))) return QTTT_ERR_NULL;
    if (misaligned(tree, 16) || misaligned(paths, 16) || (gumbel && (misaligned(x.rec, 16) || misaligned(x.visit_table, 4))))
        return QTTT_ERR_ACTION;
    work = true;
    return 0;
}

}  // namespace

#endif  // QTTT_SELFPLAY_RECORD_HOST_H

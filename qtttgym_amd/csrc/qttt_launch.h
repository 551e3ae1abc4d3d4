// qttt_launch.h — host only: what every C ABI entry of qttt_kernels.hip is written with.  The step's launch-shape
// table, the compile-time dispatch of runtime flags (with_bools / with_int), the one launch form and its chunked loop, and the observation
// buffers' check (the predicates of every argument check are qttt_checks.h's).
#ifndef QTTT_LAUNCH_H
#define QTTT_LAUNCH_H
#include <atomic>
#include <type_traits>
#include "qttt_step_kernels.h"
#include "qttt_checks.h"

namespace {

// Boards per lane and workgroup size of the step kernel, by batch size.  Measured on MI355X with
// tools/stepbench (interleaved A/B, profiles/r02/stepbench_block_sweep.txt), us per launch:
//   boards      (1,256) (1,1024) (2,256) (2,512) (2,1024)
//   131 072      3.11    3.41     3.36    3.46    4.25
//   262 144      3.63    3.66     3.90    3.86    4.62
//   393 216      4.38    4.74     4.61    4.92    4.83
//   524 288      5.16    4.93     5.30    5.23    5.08
//   786 432      7.29    6.75     6.59    6.27    6.95
//   1 048 576    8.84    8.72     7.68    7.37    7.25
//   1 572 864   12.05   12.75    11.56   11.78   11.39
//   2 097 152   14.38   16.10    13.53   13.64   14.08
//   4 194 304   28.40   30.52    27.51   27.78   29.12
//   16 777 216  103.2   109.0    105.0   107.4   108.5
// Below ~450 K boards the launch is latency-bound and one board per lane in small workgroups puts the
// most waves in flight; 1024-thread workgroups win where they fill the chip exactly once (512 K lanes =
// 2 workgroups on each of the 256 CUs); past that, small workgroups backfill best.
inline void auto_tuning(int64_t n, int &bpl, int &blk) {
    if (n <= 448 * 1024) { bpl = 1; blk = 256; }
    else if (n <= 512 * 1024) { bpl = 1; blk = 1024; }
    else if (n < 896 * 1024) { bpl = 2; blk = 512; }
    else if (n <= 1536 * 1024) { bpl = 2; blk = 1024; }
    else { bpl = 2; blk = 256; }
}
// qttt_step_many's register-resident route: the rows of the table above where a batch is ONE occupancy round of the step
// kernel — (1, 1024), (2, 512), (2, 1024): every board of the batch is on the chip at once and the whole working set sits in
// the Infinity Cache.  There a run of steps whose per-step outputs nobody keeps (out_stride == 0) goes through
// step_fused_kernel, one launch per RESIDENT_MAX_PLIES steps with the boards in registers, instead of one launch per step:
// only the state after the last step and that step's reward / terminated can ever be read.  Not below and not above these
// rows: there qttt_step_many is one launch per step, which is what bench.py's 4 096-, 262 144- and 16 M-board replay legs
// are defined and accounted as.  Not for a caller who names a launch shape (the call's QTTT_FLAG_SHAPE bits
// or the process tuning word): they are asking for the per-step kernel.  Not for runs shorter than RESIDENT_MIN_STEPS: a
// short run at a chip-filling size is the form launch-level measurements are taken in (the mailbox's "launches 2 .. 9 after
// a Board call"), and it stays what they measure; from 16 plies on the launch's own state round trip is under a tenth of
// the run.  QTTT_FLAG_FUSED asks for the same kernel at any size and any length.
constexpr int32_t RESIDENT_MIN_STEPS = 16;
inline bool one_round_rows(int64_t n) { return n > 448 * 1024 && n <= 1536 * 1024; }
inline bool shape_named(uint32_t flags);
inline bool resident_route(int64_t n, uint32_t flags, int64_t out_stride, int32_t n_steps) {
    return one_round_rows(n) && out_stride == 0 && n_steps >= RESIDENT_MIN_STEPS && !shape_named(flags);
}
// Process-wide DEFAULT launch shape (bench / profiling): boards per lane 1|2|4 and workgroup size
// 256|512|1024, 0 = by batch size.  Initialised from QTTT_STEP_BPL / QTTT_STEP_BLOCK, changeable through
// qttt_set_tuning(); one relaxed atomic word (bpl | block << 8), so concurrent callers never race on it.
// A call that carries QTTT_FLAG_SHAPE(...) in its flags does not look at it at all.
inline std::atomic<int> &tuning_word() {
    static std::atomic<int> v([] {
        int bpl = 0, blk = 0;
        if (const char *e = getenv("QTTT_STEP_BPL")) { int q = atoi(e); if (q == 1 || q == 2 || q == 4) bpl = q; }
        if (const char *e = getenv("QTTT_STEP_BLOCK")) { int q = atoi(e); if (q == 256 || q == 512 || q == 1024) blk = q; }
        return bpl | (blk << 8);
    }());
    return v;
}
inline bool shape_named(uint32_t flags) {
    return (flags & ((7u << 8) | (3u << 12))) != 0 || tuning_word().load(std::memory_order_relaxed) != 0;
}
// the shape one call is launched with: the call's own QTTT_FLAG_SHAPE bits, else the process default,
// else the table; `observe`: the observation tiles are sized for <= 2 boards per lane
inline void resolve_shape(int64_t n, uint32_t flags, bool observe, int &bpl, int &blk) {
    int f_bpl = (int)((flags >> 8) & 7u), f_blk = 0;
    switch ((flags >> 12) & 3u) { case 1: f_blk = 256; break; case 2: f_blk = 512; break; case 3: f_blk = 1024; break; default: break; }
    if (f_bpl != 1 && f_bpl != 2 && f_bpl != 4) f_bpl = 0;
    if (!f_bpl && !f_blk) {
        const int w = tuning_word().load(std::memory_order_relaxed);
        f_bpl = w & 0xFF;
        f_blk = w >> 8;
    }
    auto_tuning(n, bpl, blk);
    if (f_bpl) bpl = f_bpl;
    if (f_blk) blk = f_blk;
    if (observe && bpl > 2) bpl = 2;
    if (bpl == 4) blk = QTTT_BLOCK;                      // four boards per lane exist with 512 threads only
}

// Kernel selection: f(std::integral_constant<bool, b>...) for the runtime flags b..., and f(std::integral_constant<int,
// V>) for the V of Vs that equals v (the last one when none does); both return what f returns.  Every combination is one
// instantiation of f, reached through a tree of plain branches, so a launch inside f is a direct launch of one kernel
// instance.
template <typename F>
inline auto with_bools(F &&f) { return f(); }
template <typename F, typename... B>
inline auto with_bools(F &&f, bool b, B... rest) {
    if (b) return with_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...);
    return with_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}
template <int V, int... Vs, typename F>
inline auto with_int(int v, F &&f) {
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V>{});
    else if (v == V) return f(std::integral_constant<int, V>{});
    else return with_int<Vs...>(v, f);
}

// The one launch form: `groups` workgroups of `block` threads of one kernel instance on `stream`; 0 or the HIP error.
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
template <typename... P, typename... A>
inline int launch(void (*kernel)(P...), int64_t groups, int block, void *stream, const A &...args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3((unsigned)block), 0, (hipStream_t)stream, args...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
// `blocks` workgroups in grids of at most 2^30: launch_chunk(first block, grid) per chunk, in order, up to the first failure.
template <typename F>
inline int chunked_launch(int64_t blocks, F &&launch_chunk) {
    constexpr int64_t GRID_MAX = (int64_t)1 << 30;
    for (int64_t b0 = 0; b0 < blocks; b0 += GRID_MAX)
        if (const int rc = launch_chunk(b0, blocks - b0 < GRID_MAX ? blocks - b0 : GRID_MAX)) return rc;
    return 0;
}

// Runs of at most CAP plies from step_idx0 on, one launch each (the plies' launch keys travel as a kernel argument, KEYS:
// FusedKeys with FUSED_MAX_PLIES, ResidentKeys<CAP> for the output-free kernel): launch_run(done, plies, keys) for every
// run, in order; stops at the first launch that fails.  A slot past the run's last ply holds the first ply's key.
template <int CAP, typename KEYS, typename F>
inline int fused_runs(uint64_t seed, uint32_t step_idx0, int32_t n_steps, F &&launch_run) {
    static_assert(sizeof(KEYS) == CAP * sizeof(u64), "one key per ply");
    for (int64_t done = 0; done < n_steps; done += CAP) {
        const int32_t plies = (int32_t)(n_steps - done < CAP ? n_steps - done : CAP);
        KEYS keys;
        for (int32_t t = 0; t < CAP; ++t) keys.k[t] = launch_key(seed, step_idx0 + (u32)done + (u32)(t < plies ? t : 0));
        if (const int rc = launch_run(done, plies, keys)) return rc;
    }
    return 0;
}

// The observation buffers (qttt_observe's outputs) of a batch of n boards: all given when n > 0, q_p1 2-byte and q_p2
// 8-byte aligned (the kernels store whole rows from LDS, 2 / 8 bytes at a time).
inline bool obs_missing(const ObsOut &o) { return any_null(o.classical, o.q_p1, o.q_p1_len, o.q_p2, o.q_p2_len, o.turn); }
inline int obs_check(const ObsOut &o, int64_t n) {
    if (n > 0 && obs_missing(o)) return QTTT_ERR_NULL;
    return (misaligned(o.q_p1, 2) || misaligned(o.q_p2, 8)) ? QTTT_ERR_ACTION : 0;
}

}  // namespace

#endif  // QTTT_LAUNCH_H

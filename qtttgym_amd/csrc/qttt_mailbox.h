// qttt_mailbox.h — host only: the host half of the bounded mailbox for SINGLE Board records (board_mailbox_kernel,
// qttt_aux_kernels.h), which qttt_board_op_host serves one-record calls through.
// One resident wave on a private non-blocking stream serves a pinned request slot; a call is: copy the record into the
// slot (four 16-byte pieces of 12 data bytes + the request number each; the numbers are written last), poll the
// answer's number.  The wave leaves by itself after QTTT_BOARD_MAILBOX_US microseconds without a request (default 20,
// at most 200; 0 = no mailbox: every call is a launch, as before round 5), QTTT_BOARD_MAILBOX_MAX_US after it started
// whatever the traffic (default 1000, at most 10000), or when qttt_board_mailbox_retire() asks it to, and says so in
// `exited`; the next call then launches it again.  A request that meets a wave which has just left is answered by the
// relaunch (the host watches `exited` while it polls), and a call that gets no answer within 20 ms turns the mailbox
// off for the rest of the process and goes through the launch path — the call always returns.
// What a resident wave costs others: a DEVICE-wide synchronise (hipDeviceSynchronize, torch.cuda.synchronize()) issued
// within the idle window after a Board call waits for the wave to leave (<= the window; <= the residency bound when
// another thread keeps calling); stream-level synchronisation and the legacy default stream do not (the stream is
// non-blocking).  A step launch that fills the chip (>= 512 K boards) retires it first (retire_mailbox_for, below), so
// that the wave's CU slot does not cost that launch a second partial round.  The `stream` argument of the call is not
// used on this path: host records have no device-side producer to be ordered after.
#ifndef QTTT_MAILBOX_H
#define QTTT_MAILBOX_H
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include "qttt_aux_kernels.h"
#include "qttt_launch.h"

namespace {

// A hint: the single-record mailbox wave (BoardMailbox, below) MAY be resident.  It holds one wave slot of one CU, so a
// launch that fills the chip exactly runs a second partial round beside it (+1.4 us at 1 M boards,
// profiles/r05/keepwarm_probe.txt): such launches ask it to leave first (it is gone within one poll).  One relaxed load
// per launch when no wave is resident.  (What is NOT done from here: querying the mailbox's stream so that the runtime
// retires the finished kernel.  A finished mailbox kernel nobody has queried leaves the launches of other streams
// 0.05 - 0.4 us longer for a while — tools/probes/mailbox_rest_delta_probe.py — and one hipStreamQuery after the wave has
// said it left removes most of that, which qttt_board_mailbox_retire(1) does; but the query returns "not ready" for a few
// microseconds after the wave's last store, and repeating it from the launch path cost the launches 0.4 - 1.0 us each:
// measured, profiles/r06/mailbox_rest_delta_probe_query_from_the_launch_path.txt, not adopted.)
std::atomic<bool> g_mailbox_resident{false};
constexpr int64_t CHIP_FILLING_BOARDS = 512 * 1024;

struct BoardMailbox {
    std::mutex mu;
    bool tried = false, on = false, alive = false, leaving = false;
    int device = -1;
    uint8_t *slot_in = nullptr, *slot_out = nullptr;     // 64 bytes each, pinned, system-coherent
    u32 *exited = nullptr;
    hipStream_t stream = nullptr;
    u32 ring = 0, generation = 0;
    u64 idle_ticks = 0, resident_ticks = 0;

    bool start() {                                       // once per process
        tried = true;
        long us = 20, max_us = 1000;
        if (const char *e = getenv("QTTT_BOARD_MAILBOX_US")) us = atol(e);
        if (const char *e = getenv("QTTT_BOARD_MAILBOX_MAX_US")) max_us = atol(e);
        if (us <= 0) return false;
        if (us > 200) us = 200;
        if (max_us < us) max_us = us;
        if (max_us > 10000) max_us = 10000;
        idle_ticks = (u64)us * 100u;                     // s_memrealtime: 100 MHz
        resident_ticks = (u64)max_us * 100u;
        uint8_t *mem = nullptr;
        if (hipGetDevice(&device) != hipSuccess) return false;
        if (hipHostMalloc(reinterpret_cast<void **>(&mem), 256, hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); return false; }
        memset(mem, 0, 256);
        slot_in = mem; slot_out = mem + 64; exited = reinterpret_cast<u32 *>(mem + 128);
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(mem); return false; }
        on = true;
        return true;
    }
    bool launch_wave() {
        ++generation;
        alive = launch(board_mailbox_kernel, 1, 64, stream, reinterpret_cast<const mbox_u32x4 *>(slot_in),
                       reinterpret_cast<mbox_u32x4 *>(slot_out), exited, generation, ring, 1u << 20, idle_ticks, 1u << 20,
                       resident_ticks) == 0;
        leaving = false;
        g_mailbox_resident.store(alive, std::memory_order_relaxed);
        return alive;
    }
    void write_numbers(u32 v) {
        volatile u32 *w = reinterpret_cast<volatile u32 *>(slot_in);
        w[3] = v; w[7] = v; w[11] = v; w[15] = v;
    }
    bool has_left() { return *static_cast<volatile u32 *>(exited) == generation; }
    // the wave was asked to leave: wait until it has said so (its next poll: a few us; bounded), then give the runtime ONE
    // chance to retire the finished kernel here rather than beside the caller's next launches (see g_mailbox_resident)
    void await_exit() {
        const auto give_up = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
        bool gone = has_left();
        for (unsigned spin = 1; !gone; ++spin, gone = has_left())
            if ((spin & 1023u) == 0u && std::chrono::steady_clock::now() > give_up) break;   // (it then leaves by its idle exit)
        alive = leaving = false;
        g_mailbox_resident.store(false, std::memory_order_relaxed);
        if (gone) { (void)hipStreamQuery(stream); (void)hipGetLastError(); }
    }
    // 0 = a resident wave was asked to leave (or none was resident); it is gone within a poll (a few us)
    int retire(bool wait) {
        std::lock_guard<std::mutex> g(mu);
        if (!on || !alive) { g_mailbox_resident.store(false, std::memory_order_relaxed); return 0; }
        if (has_left()) { alive = leaving = false; g_mailbox_resident.store(false, std::memory_order_relaxed); return 0; }
        if (!leaving) {
            write_numbers(MBOX_LEAVE);
            leaving = true;
        }
        if (wait) await_exit();
        return 0;
    }
    // From the step entries, in front of a launch that fills the chip (never blocks, never calls into the runtime): ask a
    // resident wave to leave.
    void housekeeping() {
        std::unique_lock<std::mutex> g(mu, std::try_to_lock);
        if (!g.owns_lock()) return;                              // a Board call is in flight on another thread: its business
        if (!on || !alive) { g_mailbox_resident.store(false, std::memory_order_relaxed); return; }
        if (has_left()) { alive = leaving = false; g_mailbox_resident.store(false, std::memory_order_relaxed); return; }
        if (!leaving) {
            static const bool keep = [] { const char *e = getenv("QTTT_BOARD_MAILBOX_KEEP"); return e && atoi(e) != 0; }();
            if (keep) return;                                    // (QTTT_BOARD_MAILBOX_KEEP=1: A/B diagnostics of this very rule)
            write_numbers(MBOX_LEAVE);
            leaving = true;
        }
        g_mailbox_resident.store(false, std::memory_order_relaxed);   // asked once: the later launches have nothing to do here
    }
    // 0 = answered (out filled), 1 = not served: use the launch path
    int call(const void *rec_in, void *rec_out) {
        std::lock_guard<std::mutex> g(mu);
        if (!tried) start();
        int dev = -1;
        if (!on || hipGetDevice(&dev) != hipSuccess || dev != device) return 1;
        if (leaving) await_exit();
        ring = mbox_next(ring);
        volatile u32 *answer = reinterpret_cast<volatile u32 *>(slot_out) + 15;
        volatile u32 *gone = exited;
        if (alive && *gone == generation) alive = false;
        const uint8_t *src = static_cast<const uint8_t *>(rec_in);
        for (int k = 0; k < 4; ++k) memcpy(slot_in + 16 * k, src + 12 * k, 12);   // record bytes 0..47 (41 are read)
        std::atomic_thread_fence(std::memory_order_release);
        write_numbers(ring);
        if (!alive && !launch_wave()) { on = false; return 1; }
        const auto give_up = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
        for (unsigned spin = 1; *answer != ring; ++spin) {
            if (*gone == generation && *answer != ring) {          // the wave left before it saw this request
                if (!launch_wave()) { on = false; return 1; }
            }
            if ((spin & 4095u) == 0u && std::chrono::steady_clock::now() > give_up) {
                on = false;                                        // something is wrong with this path on this host: stop using it
                return 1;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        memcpy(rec_out, slot_out, 60);
        static_cast<uint8_t *>(rec_out)[60] = static_cast<uint8_t *>(rec_out)[61] = static_cast<uint8_t *>(rec_out)[62] = 0;
        static_cast<uint8_t *>(rec_out)[63] = 1;                   // the completion stamp of the contract
        return 0;
    }
};
BoardMailbox &board_mailbox() {
    static BoardMailbox m;
    return m;
}
inline void retire_mailbox_for(int64_t n) {
    if (n >= CHIP_FILLING_BOARDS && g_mailbox_resident.load(std::memory_order_relaxed)) board_mailbox().housekeeping();
}

}  // namespace

#endif  // QTTT_MAILBOX_H

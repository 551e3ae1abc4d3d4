// qttt_checks.h — plain C++17 without HIP: the predicates that the argument checks of every C ABI entry are made of, once.
// qttt_launch.h includes it for qttt_kernels.hip, the host-check headers (csrc/*_host.h) for their stand-alone programs under
// tools/.  Every entry asks in the order include/qttt.h promises: a bad size -> QTTT_ERR_SIZE, an empty batch -> 0, a required
// pointer missing -> QTTT_ERR_NULL, a pointer the kernel's vector accesses cannot take -> QTTT_ERR_ACTION; then the launch.
#ifndef QTTT_CHECKS_H
#define QTTT_CHECKS_H
#include <stdint.h>
#include "qttt.h"

namespace {

template <typename... P>
inline bool any_null(const P *...p) { return (... || !p); }
inline bool misaligned(const void *p, unsigned bytes) { return ((uintptr_t)p & (bytes - 1u)) != 0; }   // bytes: 2^k; null passes
inline bool is_finite(double x) { return x - x == 0.0; }     // false for NaN and the infinities (libm owns the name finite)

inline bool tree_size_bad(int64_t games, int64_t capacity) { return games < 0 || capacity < 1 || capacity > QTTT_TREE_MAX_CAPACITY; }
// the sizes of a leaf-parallel round: K in range, and games * K boards, records and priors rows addressable
inline bool tree_leaves_bad(int64_t games, int leaves) {
    return games < 0 || leaves < 1 || leaves > QTTT_TREE_MAX_LEAVES || games > INT64_MAX / (256 * (int64_t)QTTT_TREE_MAX_LEAVES);
}

}  // namespace

#endif  // QTTT_CHECKS_H

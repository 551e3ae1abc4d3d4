/* qttt_tree_compact.h — compaction of the device search trees of qttt_tree.h, part of the C ABI of libqttt_hip.so (an
 * additive entry of QTTT_ABI_VERSION 6; included by qttt.h after qttt_tree.h, whose buffer layout, conventions and
 * error order hold here; the algorithm is described in qttt_tree.h's header comment).
 *
 * Errors, in this order, before any device work: QTTT_ERR_SIZE for games < 0 or capacity outside
 * 1..QTTT_TREE_MAX_CAPACITY (qttt_tree_compact_bytes returns it too); 0 with no device work for games == 0;
 * QTTT_ERR_NULL for a null tree or scratch; QTTT_ERR_ACTION for a tree not 16-byte or a scratch not 4-byte aligned. */
#ifndef QTTT_TREE_COMPACT_H
#define QTTT_TREE_COMPACT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the scratch buffer qttt_tree_compact needs (host-only): one i32 per node, 4 games capacity;
 * QTTT_ERR_SIZE for bad sizes. */
int64_t qttt_tree_compact_bytes(int64_t games, int64_t capacity);

/* MCTS._prune as done by sync (mcts.py:222-231, 330-337): keeps the nodes reachable from each game's root, in their
 * old order, root at index 0; used = their number; the recorded path is cleared as by qttt_tree_reset (depth = leaf =
 * 0, the leaf flags those of the root); the overflow flag keeps its value.  Node records and priors at or beyond the
 * new `used` are unspecified afterwards, as is `scratch`.  A game that is compact already (root 0, every node
 * reachable) is left as it is, byte for byte. */
int qttt_tree_compact(void *tree, int64_t games, int64_t capacity, void *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif

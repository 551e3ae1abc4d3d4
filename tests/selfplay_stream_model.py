"""A numpy model of the bookkeeping of continuous self-play (include/qttt_selfplay_stream.h): the per-game record row, the
harvest of the slots whose new root is terminal, the masked lengths the append takes, and the restart.  The search and the
moves are not modelled: a test hands the model, ply by ply, the roots it would have seen.  Nothing runs on a device."""
import numpy as np

import replay_model

ROWS = replay_model.ROWS


class Stream:
    """G slots.  ply(roots, after) is one stream ply: `roots` = per slot (P, Q, pi[36], mask[36], action36) of the live
    root that is recorded, `after` = per slot None (the game goes on) or (P, Q, winner) of the terminal root the move led
    to.  The staging arrays are SelfPlayBatch's; `ring` (replay_model.Ring, optional) receives the appends."""

    def __init__(self, G, ring=None, v_first=1.0, v_second=0.0):
        self.G, self.ring, self.v_first, self.v_second = G, ring, np.float32(v_first), np.float32(v_second)
        self.stride = (G + 63) // 64 * 64
        self.states = np.zeros((ROWS, 2, self.stride), np.uint64)
        self.pi = np.zeros((ROWS, G, 36))
        self.mask = np.zeros((ROWS, G, 36), np.uint8)
        self.done = np.zeros((ROWS, G), np.uint8)
        self.v = np.zeros((ROWS, G), np.float32)
        self.action36 = np.zeros((ROWS, G), np.uint8)
        self.length = np.zeros(G, np.uint8)
        self.winner = np.zeros(G, np.int8)
        self.harvest_len = np.zeros(G, np.uint8)
        self.finished = np.zeros(G, np.uint8)
        self.games_done = np.zeros(G, np.int64)
        self.tally = np.zeros((G, 4), np.int64)
        self.plies = 0
        self.log = []                                   # (ply, slot, rows) of every harvested game, in ring order

    # the three device steps
    def record(self, roots):
        for g in range(self.G):
            t = int(self.length[g])
            # a slot is never at a terminal root when a ply begins, and a live game has a row left for its terminal one
            assert t < ROWS - 1 and (t == 0 or self.done[t - 1, g] == 0), (g, t)
        for g, (P, Q, pi, mask, a) in enumerate(roots):
            t = int(self.length[g])
            self.states[t, 0, g], self.states[t, 1, g] = P, Q
            self.pi[t, g], self.mask[t, g], self.done[t, g], self.action36[t, g] = pi, mask, 0, a
            self.length[g] = t + 1

    def harvest(self, after):
        for g, end in enumerate(after):
            if end is None:
                self.harvest_len[g] = self.finished[g] = 0
                continue
            P, Q, w = end
            t = int(self.length[g])
            assert t < ROWS
            self.states[t, 0, g], self.states[t, 1, g] = P, Q
            self.pi[t, g], self.mask[t, g], self.done[t, g], self.action36[t, g] = 1.0 / 36.0, 1, 1, 255
            v0 = self.v_first if w > 0 else (self.v_second if w == 0 else np.float32(0.0))
            for i in range(t + 1):
                x = -v0 if i & 1 else v0
                self.v[i, g] = np.float32(0.0) if x == 0 else x
            self.winner[g] = w
            self.length[g] = self.harvest_len[g] = t + 1
            self.finished[g] = 1
            self.games_done[g] += 1
            self.tally[g, 0 if w > 0 else (1 if w == 0 else 2)] += 1
            self.tally[g, 3] += t + 1
            self.log.append((self.plies, g, t + 1))

    def restart(self):
        for g in np.nonzero(self.finished)[0]:
            self.states[:, :, g] = 0
            self.pi[:, g], self.mask[:, g], self.done[:, g], self.v[:, g], self.action36[:, g] = 0, 0, 0, 0, 0
            self.length[g] = 0

    def ply(self, roots, after):
        self.record(roots)
        self.harvest(after)
        n = 0
        if self.ring is not None:
            n = self.ring.append(self.states.reshape(ROWS, -1).view(np.uint8), self.pi, self.mask, self.done, self.v,
                                 self.harvest_len)
            assert n == int(self.harvest_len.sum())
        self.restart()
        self.plies += 1
        return n

    # the returned statistics
    @property
    def samples(self):
        return int(self.tally[:, 3].sum())

    @property
    def winners(self):
        return self.tally[:, :3].sum(0).tolist()

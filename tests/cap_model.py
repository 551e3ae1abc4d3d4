"""The model of playout cap randomisation (include/qttt_tree_subset.h, include/qttt_selfplay_cap.h) that
tests/test_cap_cpu.py and tests/test_cap_gpu.py sit over.  "Model" means: the composition of the entries the library had
before the feature, plus the host's draw.  A capped ply is replayed by searching WHOLE copies of the trees one group at a
time with the existing full-batch calls (TreeSearch.contemplate, add_root_noise), taking every game's bytes from the copy
of its own group, recording with the existing stream record into a scratch batch and keeping only what the capped record
may write; the back-fill's signs are redone from the recorded states.  The draw is restated with the library's
host-callable qttt_hash, one Python integer at a time.  A plain helper module."""
import numpy as np
import torch

from qtttgym_amd import _native

GAME_BYTES, NODE_BYTES, PRIOR_BYTES = _native.TREE_GAME_BYTES, _native.TREE_NODE_BYTES, _native.TREE_PRIOR_BYTES
FIELDS = ("states", "pi", "mask", "done", "v", "action36", "length", "winner", "actions")
ROWS = _native.SELFPLAY_ROWS


# ---------------------------------------------------------------- the draw
def is_full(seed, board_id, ply_index, p):
    h = int(_native.lib().qttt_hash(int(seed), int(board_id), (_native.SELFPLAY_CAP_BASE + int(ply_index)) & 0xFFFFFFFF))
    return float(h >> 11) * 2.0 ** -53 < p


def full_mask(seed, board_offset, G, ply_index, p):
    return np.array([is_full(seed, board_offset + g, ply_index, p) for g in range(G)], dtype=np.uint8)


# ---------------------------------------------------------------- the rows' signs
def moves_played(P):
    """The moves played of packed P words (include/qttt.h: bits 8..11 of the high word)."""
    return (np.asarray(P, dtype=np.uint64) >> np.uint64(40)) & np.uint64(0xF)


def backfill(P_rows, v0):
    """v of a finished game's rows from their states' P words: +v0 where the first player is to move, a zero is +0.0."""
    odd = (moves_played(P_rows) & np.uint64(1)).astype(bool)
    v = np.where(odd, -np.float32(v0), np.float32(v0)).astype(np.float32)
    return np.where(v == 0, np.float32(0.0), v)


def state_words(states, G):
    """The staging states u8[ROWS, bytes] as (P, Q) int64 [ROWS, G] views' copies."""
    w = states.view(torch.int64).view(ROWS, 2, -1)
    return w[:, 0, :G], w[:, 1, :G]


# ---------------------------------------------------------------- subsets of the games
def subsets(G):
    """name -> ids of the issue's subsets: none, all, the last game only, every other game, one game per workgroup (a
    workgroup holds four games)."""
    return {"none": [], "all": list(range(G)), "last": [G - 1], "every other": list(range(0, G, 2)),
            "one per workgroup": list(range(min(1, G - 1), G, 4))}


def game_views(buf, G, capacity):
    """A tree buffer (torch u8) as three [G, bytes] views: game headers, node records, priors."""
    o1 = G * GAME_BYTES
    o2 = o1 + G * capacity * NODE_BYTES
    o3 = o2 + G * capacity * PRIOR_BYTES
    return buf[:o1].view(G, -1), buf[o1:o2].view(G, -1), buf[o2:o3].view(G, -1)


def copy_games(dst, src, mask, G, capacity):
    for d, s in zip(game_views(dst, G, capacity), game_views(src, G, capacity)):
        d[mask] = s[mask]


def clone_batch(sp, batch):
    out = sp.new_batch()
    for f in FIELDS:
        getattr(out, f).copy_(getattr(batch, f))
    if getattr(batch, "q", None) is not None:
        out.alloc_q().copy_(batch.q)
    return out


# ---------------------------------------------------------------- capped self-play out of the existing entries
class CapModel:
    """SelfPlay(playout_cap=(p, n_fast), **kw) replayed with SelfPlay(**kw) and three TreeSearch objects."""

    def __init__(self, G, game_seed, playout_cap, **kw):
        from qtttgym_amd import SelfPlay, TreeSearch
        self.p, self.n_fast = playout_cap
        self.G, seed = G, int(game_seed)
        sp = self.sp = SelfPlay(G, **kw)
        self.st = sp._stream_begin(seed)
        self.env, self.tree, self.batch = self.st["env"], self.st["tree"], self.st["batch"]
        make = lambda **over: TreeSearch(G, capacity=sp.capacity, seed=2 * seed + 1, device=sp.device,      # noqa: E731
                                         **dict(sp.search_kwargs(), **over))
        self.fast_tree, self.full_tree = make(forced_playouts=None), make()

    def _group_copy(self, t):
        """A whole copy of the trees as they stand after the first rollout, their counters included."""
        src = self.tree
        t.tree.copy_(src.tree)
        t.rollout_idx, t._bound, t._fresh, t.noise_idx = src.rollout_idx, src._bound, src._fresh, src.noise_idx
        return t

    def search(self, ply_index):
        sp, t, G = self.sp, self.tree, self.G
        full = full_mask(t.seed, t.board_offset, G, ply_index, self.p)
        t.contemplate(1)
        fast_t = self._group_copy(self.fast_tree)
        fast_t.contemplate(self.n_fast - 1)
        full_t = self._group_copy(self.full_tree)
        if sp.root_noise is not None:
            full_t.add_root_noise(*sp.root_noise)
            t.noise_idx += 1
        full_t.contemplate(sp.n_rollouts - 1)
        m = torch.as_tensor(full.astype(bool), device=sp.device)
        copy_games(t.tree, full_t.tree, m, G, t.capacity)
        copy_games(t.tree, fast_t.tree, ~m, G, t.capacity)
        t.rollout_idx, t._bound, t._fresh = full_t.rollout_idx, full_t._bound, full_t._fresh   # the copy that ran them all
        return m

    def _resign(self, games):
        """The back-fill of the finished games `games` (bool[G]) by their rows' states."""
        b, G = self.batch, self.G
        P = state_words(b.states, G)[0].cpu().numpy().view(np.uint64)
        v, length = b.v.cpu().numpy(), b.length.cpu().numpy()
        for g in np.nonzero(games.cpu().numpy())[0]:
            n = int(length[g])
            v[:n, g] = backfill(P[:n, g], v[0, g])               # the existing kernels give row 0 +v0
        b.v.copy_(torch.as_tensor(v))

    def record(self, full, draw_index):
        """The capped record out of the existing stream record: returns the actions to step with."""
        sp, b, G = self.sp, self.batch, self.G
        tmp = clone_batch(sp, b)
        sp.record(self.tree, None, tmp, draw_index=draw_index)
        row = b.length.to(torch.int64)
        live = tmp.length != b.length
        g = torch.arange(G, device=sp.device)
        term = live & (tmp.done[row.clamp(max=ROWS - 1), g] != 0)
        take = live & (full | term)
        for f, (_, shp) in b._ROWS.items():
            getattr(b, f)[:, take] = getattr(tmp, f)[:, take]
        for src, dst in zip(state_words(tmp.states, G), state_words(b.states, G)):
            dst[:, take] = src[:, take]
        b.length[take] = tmp.length[take]
        b.winner[term] = tmp.winner[term]
        b.actions.copy_(tmp.actions)
        self._resign(term)
        return b.actions

    def play_ply(self, ply):
        sp = self.sp
        if ply < ROWS - 1:
            full = self.search(ply)
            if sp.value_mode is not None:
                sp.record_value(self.tree, None, self.batch)
        else:
            full = torch.zeros(self.G, dtype=torch.bool, device=sp.device)
        self.env.step_raw(self.record(full, ply))
        self.tree.sync(self.env)
        if sp.compact:
            self.tree.compact()

    def play(self):
        for ply in range(ROWS):
            self.play_ply(ply)
        return self.batch

    def stream_ply(self, ring):
        sp, st = self.sp, self.st
        if not sp.compact:
            self.tree._bound = 1 + (ROWS - 2) * (2 * sp.n_rollouts + 1)
        full = self.search(st["ply"])
        self.env.step_raw(self.record(full, st["ply"]))
        self.tree.sync(self.env)
        if sp.compact:
            self.tree.compact()
        sp._stream_harvest(st)
        self._resign(st["finished"] != 0)
        ring.add(self.batch, length=st["harvest_len"])
        sp._stream_restart(st)
        st["ply"] += 1

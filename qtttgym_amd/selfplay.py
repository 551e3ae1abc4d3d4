"""SelfPlay — the data half of the reference's self_play.py for G games at once, on the device
(include/qttt_selfplay.h): play_game (self_play.py:43-76) with a TreeSearch per batch, and every visited
root turned into a training sample (self_play.py:193-216) by one kernel per ply.

    sp = SelfPlay(1024, n_rollouts=100, net=PolicyValueNet(sd))
    s, pi, mask, v, done = sp.play().flat()         # the reference's s_batch, pi_batch, mask_batch, v_batch, done

Training on the batch is ordinary torch autograd or qtttgym_amd.Trainer (examples/selfplay_train.py [--device-train]);
there is no loss, gradient or optimiser here.  By default the move played is MCTS.choose, as in the reference.  AlphaZero's root exploration is optional
(include/qttt_tree_explore.h): root_noise=(epsilon, alpha) mixes Dirichlet noise into the roots' priors
before every searched move, and sample_plies / temperature draw the move of the first plies from the visit counts.  The
board's eight symmetries, which the reference left as a stub (self_play.py expand_symetries), are SelfPlayBatch.augment (DESIGN.md
§14): one launch turns the batch of G games into the batch of 8 G games it stands for.  sp.stream(ring, plies) is
continuous self-play (include/qttt_selfplay_stream.h): the G slots stay full, a finished game hands its rows
to a ReplayBuffer and restarts in place.  exact_targets=M replaces the value and policy targets of the positions with at
least M moves played by the truth, enumerated on the device (include/qttt_selfplay_exact.h).
value_mix=L / td_lambda=L make the value targets of fresh samples out of the searched value of every recorded root instead
of the game's outcome alone (include/qttt_selfplay_value.h).
playout_cap=(p, n_fast) is KataGo's playout cap randomisation (include/qttt_selfplay_cap.h): a random
fraction p of the plies gets the full search and becomes a sample, the others are searched with n_fast rollouts, without
noise, and are played but not recorded.
play() and stream() run one ply through one method, SelfPlay._ply: the search (capped or not), record_value, the record, the
step, the sync and the compaction.
"""
import ctypes

import torch

from . import _native
from ._host import LibCaller, _ptr, _raw_stream, cap_full_mask, check_net, check_tensor, resolve_device
from .symmetry import check_symmetries
from .tree import TreeSearch
from .vec_env import VecEnv

ROWS = _native.SELFPLAY_ROWS


class SelfPlayBatch:
    """One play()'s samples as the kernel wrote them, row t = the t-th root of every game (rows at or past a game's
    `length` are zero): states u8[10, qttt_state_bytes(G)], pi f64[10, G, 36], mask u8[10, G, 36], done u8[10, G],
    v f32[10, G], action36 u8[10, G] (the move played from the row, 255 in the terminal row), length u8[G] (rows of
    the game, its terminal row included), winner i8[G] (1 / 0 / -1 = True / False / None) and actions u8[G, 2], the
    last ply's move.
    q f32[10, G], the searched value of every recorded root (include/qttt_selfplay_value.h), is there only when
    SelfPlay(value_mix= / td_lambda=) or alloc_q() asked for it; it is no part of _ROWS, _FIELDS or flat(), and an
    augmented batch has no q."""

    _ROWS = {"pi": (torch.float64, (36,)), "mask": (torch.uint8, (36,)), "done": (torch.uint8, ()),
             "v": (torch.float32, ()), "action36": (torch.uint8, ())}

    def __init__(self, num_games, device, state_bytes):
        G = self.num_games = int(num_games)
        self.device = device
        self.states = torch.zeros((ROWS, int(state_bytes)), dtype=torch.uint8, device=device)
        for k, (dt, shp) in self._ROWS.items():
            setattr(self, k, torch.zeros((ROWS, G) + shp, dtype=dt, device=device))
        self.length = torch.zeros(G, dtype=torch.uint8, device=device)
        self.winner = torch.zeros(G, dtype=torch.int8, device=device)
        self.actions = torch.zeros((G, 2), dtype=torch.uint8, device=device)

    def row_env(self, t):
        """Row t's states as a VecEnv (a view: encode(), evaluate(), export_boards() ... of the t-th roots)."""
        return VecEnv.from_state(self.states[t], self.num_games)

    _FIELDS = ("states", "pi", "mask", "done", "v", "action36", "length", "winner", "actions")

    def augment(self, symmetries=None):
        """The batch of K * G games this one stands for under the board's symmetries (include/qttt_symmetry.h
        qttt_selfplay_augment, one launch): `symmetries` = 1..8 of 0..7 (qtttgym_amd.symmetry), default all eight in
        order.  Game s * G + g of the result is game g under symmetries[s]: its states are the states of the mirrored
        game, pi / mask / action36 are permuted, v / done / length / winner are the game's own.  A new SelfPlayBatch."""
        sym = check_symmetries(symmetries)
        G, K, lib = self.num_games, len(sym), _native.lib()
        out = SelfPlayBatch(K * G, self.device, lib.qttt_state_bytes(K * G))
        with torch.cuda.device(self.device):
            rc = lib.qttt_selfplay_augment(G, (ctypes.c_uint8 * K)(*sym), K,
                                           *[getattr(self, f).data_ptr() for f in self._FIELDS],
                                           *[getattr(out, f).data_ptr() for f in self._FIELDS],
                                           _raw_stream(self.device.index))
        _native.check(rc, "qttt_selfplay_augment")
        return out

    def exact_targets(self, min_ply, policy=True, rows=None):
        """Relabels the late rows in place (include/qttt_selfplay_exact.h qttt_selfplay_exact_targets, one launch, no host
        synchronisation): every recorded, non-terminal row with at least `min_ply` (6..9) moves played gets v = the exact
        expectimax value of its position for the player to move and, with policy=True, pi = the uniform distribution
        over its optimal actions; every other byte of the batch stays.  rows (u8[G], optional) stands in for `length`: the
        rows below rows[g] of game g are looked at, none of a game with 0.  Returns u8[10, G], 1 where a row was
        relabelled.  The exact value is the mover's, in [-1, 1]: it belongs with value targets (1, -1), which SelfPlay
        enforces and this method cannot know."""
        m = SelfPlay.check_min_ply(min_ply, "min_ply")
        G, dev = self.num_games, self.device
        if rows is not None:
            check_tensor(rows, torch.uint8, (G,), dev, "rows")
        exact = torch.empty((ROWS, G), dtype=torch.uint8, device=dev)
        self._exact_targets(m, policy, rows, exact)
        return exact

    def _exact_targets(self, min_ply, policy, rows, exact):
        with torch.cuda.device(self.device):
            rc = _native.lib().qttt_selfplay_exact_targets(
                self.states.data_ptr(), self.num_games, min_ply, 1 if policy else 0, _ptr(rows), self.length.data_ptr(),
                self.done.data_ptr(), self.mask.data_ptr(), self.pi.data_ptr(), self.v.data_ptr(), _ptr(exact),
                _raw_stream(self.device.index))
        _native.check(rc, "qttt_selfplay_exact_targets")

    VALUE_MODES = {"mix": _native.VALUE_MIX, "td": _native.VALUE_TD}

    def alloc_q(self):
        """Gives the batch its q f32[10, G] row field, zero-filled (once); returns it."""
        if getattr(self, "q", None) is None:
            self.q = torch.zeros((ROWS, self.num_games), dtype=torch.float32, device=self.device)
        return self.q

    @staticmethod
    def check_lambda(lam, what):
        if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0.0 <= float(lam) <= 1.0:
            raise ValueError("%s must be a number in [0, 1]" % what)
        return float(lam)

    def value_targets(self, mode, lam, rows=None, exact=None):
        """Rewrites v in place from the searched values q (include/qttt_selfplay_value.h qttt_selfplay_value_targets, one
        launch, no host synchronisation).  mode "mix": v = (1 - lam) v + lam q on every recorded, non-terminal row,
        Reanalyser's rule; mode "td": the TD(lam) return of the rest of the game, backwards from the last row, negated from
        row to row (lam = 1 is the outcome, bit for bit; lam = 0 the one-step target).  rows (u8[G], optional) stands in
        for `length`, as in exact_targets; exact (u8[10, G], optional: exact_targets' result) marks rows that keep their v
        and, under "td", restart the recursion from it.  Needs q: a batch recorded with SelfPlay(value_mix= / td_lambda=),
        or alloc_q() and SelfPlay.record_value."""
        if mode not in self.VALUE_MODES:
            raise ValueError('mode must be "mix" or "td"')
        lam = self.check_lambda(lam, "lam")
        G, dev = self.num_games, self.device
        if getattr(self, "q", None) is None:
            raise ValueError("the batch has no q: record it with SelfPlay(value_mix= / td_lambda=) or alloc_q()")
        check_tensor(self.q, torch.float32, (ROWS, G), dev, "q")
        if rows is not None:
            check_tensor(rows, torch.uint8, (G,), dev, "rows")
        if exact is not None:
            check_tensor(exact, torch.uint8, (ROWS, G), dev, "exact")
        with torch.cuda.device(dev):
            rc = _native.lib().qttt_selfplay_value_targets(
                G, self.VALUE_MODES[mode], lam, _ptr(rows), self.length.data_ptr(), self.done.data_ptr(), _ptr(exact),
                self.q.data_ptr(), self.v.data_ptr(), _raw_stream(dev.index))
        _native.check(rc, "qttt_selfplay_value_targets")

    def flat(self):
        """The reference's batch, game-major and in the order self_play.py:200-216 appends: s f32[n, 18, 10]
        (GameState.to_vector, by encode()), pi f64[n, 36], mask bool[n, 36], v f32[n], done bool[n], with
        n = length.sum().  Reads `length` back: one host synchronisation."""
        s = torch.stack([self.row_env(t).encode(with_mask=False) for t in range(ROWS)])        # [10, G, 18, 10]
        t = torch.arange(ROWS, device=self.device)[None, :]
        g, t = torch.nonzero(t < self.length.to(torch.int64)[:, None], as_tuple=True)             # game-major
        return s[t, g], self.pi[t, g], self.mask[t, g].bool(), self.v[t, g], self.done[t, g].bool()


class SelfPlay(LibCaller):
    """play_game for `num_games` games at once.  net=None searches with MCTS's uniform priors and playouts, a
    PolicyValueNet with AlphaZero's.  alpha is the exponent of the policy target (N / n_rollouts) ** alpha.
    value_targets = (the first row's target when the first player wins, when the second player wins): the default
    (1.0, 0.0) is what the reference computes — its `elif winner:` (self_play.py:198) never fires, so a lost game
    trains towards 0 — and (1.0, -1.0) what it evidently meant.
    compact=True compacts the trees after every move: their pool then holds 2 * n_rollouts + carry nodes (carry
    defaults to 2 * n_rollouts + 2; a carry that turns out too small raises ValueError before a node is lost) instead
    of 1 + 10 * (2 * n_rollouts + 1), at the price of one host read-back per move.  Without it play() never waits
    for the device.
    leaf_eval is TreeSearch's: "playouts" (the reference's rollout) or "value" (the leaf scored by net's value head).
    leaves and virtual_loss are TreeSearch's too: leaves=K > 1 searches K leaves per game per round (value leaves only).
    eval_symmetries is TreeSearch's as well: the leaves' values and priors averaged over their images (value leaves only).
    root_noise=(epsilon, alpha): every searched ply runs one rollout (so that every live root has priors), then
    TreeSearch.add_root_noise(epsilon, alpha), then the other n_rollouts - 1.  sample_plies=k > 0: the move of plies
    0..k-1 is drawn with probability proportional to N ** (1 / temperature) (qttt_selfplay_record_sampled, with the
    trees' seed); later plies play MCTS.choose.  pi stays the visit-count target either way.  With the defaults play()
    issues the calls it always did.
    root_policy="gumbel" (with max_considered, c_visit, c_scale: TreeSearch's; value leaves only) searches every move with
    the Gumbel root: the move is the Gumbel choice and pi the improved policy softmax(logits + sigma(completed Q))
    (qttt_selfplay_record_gumbel); alpha is then unused.  root_noise and sample_plies are rejected with it: the Gumbel
    noise is the exploration.
    exact_from is TreeSearch's: leaves with at least that many moves played are solved exactly on the device (value leaves
    only; play() and stream() alike).  It changes the search, not the batch's targets: that is exact_targets.
    prove=True (with exact_from) is TreeSearch's too: every round also proves the interior nodes whose children are all
    terminal or solved (include/qttt_tree_prove.h).  The record kernels and the played move are what they were.
    exact_targets=M (6..9; independent of exact_from, leaf_eval, root_policy and net) relabels the targets themselves
    (SelfPlayBatch.exact_targets, one launch): every recorded, non-terminal position with at least M moves played gets its
    exact value as v and, with exact_policy=True, the uniform distribution over its optimal moves as pi.  play() does it
    after its last ply and keeps the mask of relabelled rows as batch.exact; stream() does it between the harvest and the
    ring's append, for the games that ply hands to the ring only.  No host synchronisation on either route.  It needs
    value_targets=(1.0, -1.0): the exact value is the mover's, in [-1, 1], and the reference's (1, 0) is not zero-sum.
    Cost: from M = 7 the launch is cheaper than VecEnv.solve per row and adds under a tenth to a stream
    ply; at M = 6 it is several times dearer than that composition and a stream ply takes about four times as long.
    With the default None play() and stream() issue the calls they always did, and batch.exact is absent.
    value_mix=L or td_lambda=L (L in [0, 1]; at most one of the two; with or without a net: W and N exist for MCTS too)
    makes the value targets out of the search (include/qttt_selfplay_value.h).  Every searched ply then adds
    one launch BEFORE its record, record_value: the root's searched value sum W / sum N, the mover's, goes to row
    length[g] of batch.q.  value_mix: v = (1 - L) v + L q on every non-terminal row, Reanalyser's rule for fresh samples.
    td_lambda: v = the TD(L) return of the rest of the game, a backward pass that alternates the sign from row to row;
    L = 1 is the outcome, L = 0 the one-step target.  play() runs exact_targets (if set) and after it
    SelfPlayBatch.value_targets(..., exact=batch.exact), following its last ply: the exact rows keep their value and the
    rows before them are bootstrapped through it.  stream() runs the two in that order between the harvest and the ring's
    append, with rows = the harvested lengths.  No host synchronisation on either route.  Both need
    value_targets=(1.0, -1.0), as Reanalyser's value_mix does.  With both None play() and stream() issue the calls they
    always did, and batch.q is absent.
    forced_playouts=k (TreeSearch's; value leaves and the PUCT root only) with prune_targets (default: True exactly when
    forced_playouts is given) are KataGo's pair of remedies for root noise at small budgets (include/qttt_tree_forced.h,
    DESIGN.md §30).  The trees search with forced playouts; with prune_targets the record is qttt_selfplay_record_pruned
    (qttt_selfplay_record_stream_pruned in stream()): pi is made of the visits that are left after every action but the most
    visited one has given back the forced visits PUCT would not have made; the move, v, mask and done are the sampled
    record's, read from the unpruned counts.  prune_targets=True needs forced_playouts; forced_playouts with
    prune_targets=False only forces.  With both at their defaults play() and stream() issue the calls they always did.
    playout_cap=(p, n_fast), p in (0, 1], 1 <= n_fast <= n_rollouts (a net and value leaves only), is playout cap
    randomisation (include/qttt_selfplay_cap.h).  One capped ply: the host draws full[g] for every game with
    the counter hash of (the trees' seed, board_offset + g, the ply's index) — no read-back, so it knows both groups — and
    uploads the mask and the two id lists; one plain rollout runs in all games; root_noise goes to the full group only; the
    fast group runs n_fast - 1 more rollouts with the plain root rule and the full group n_rollouts - 1, forced if
    forced_playouts is set, both in one TreeSearch.contemplate_groups(), so a round's network launch has (games in the
    group) * leaves rows; the trees' rollout index advances by n_rollouts.  The record is qttt_selfplay_record_capped: a
    full game's row is what it would have been, a fast game's move is played and nothing is recorded, so batch.length
    counts rows, not plies, and a game whose plies were all fast yields its terminal row alone; v is signed by the side to
    move of each recorded state.  stream() harvests with qttt_selfplay_harvest_capped.  play() uses the same record; it
    cannot know which games are over without a read-back, so a finished game stays in the group its draw names and costs
    that group's rows (its root is terminal: every descent ends there and nothing changes).  value_mix, exact_targets,
    root_noise, forced_playouts, prune_targets, sample_plies and compact compose; root_policy="gumbel", exact_from and
    prove are refused (their kernels index their records by game), and so is td_lambda: TD(lambda) chains consecutive
    plies, and the rows are no longer consecutive.  playout_cap=(1.0, n) records every ply: the batch of playout_cap=None.
    With the default None every call, buffer and launch sequence is what it was.
    resident=True with rounds_per_launch (TreeSearch's; a net, value leaves and the PUCT root only) searches every ply of
    play() and stream() with the resident search (include/qttt_tree_resident.h): the rounds of a ply run
    inside launches of qttt_tree_search_resident and every tensor of the batch, the ring and the statistics is what it was.
    root_noise, sample_plies, forced_playouts, prune_targets, compact, value_mix, td_lambda and exact_targets compose;
    playout_cap (subset rounds), root_policy="gumbel", exact_from, prove and eval_symmetries are refused, here and in a
    Reanalyser made of such a SelfPlay.  With the default False every call, buffer and launch is what it was."""

    def __init__(self, num_games, n_rollouts=100, num_simulations=10, net=None, alpha=1.0, c_puct=1.0,
                 value_targets=(1.0, 0.0), seed=0, compact=False, carry=None, device=None, leaf_eval="playouts",
                 root_noise=None, temperature=1.0, sample_plies=0, leaves=1, virtual_loss=1.0,
                 eval_symmetries=None, root_policy="puct", max_considered=16, c_visit=50.0, c_scale=1.0, exact_from=None,
                 exact_targets=None, exact_policy=True, prove=False, value_mix=None, td_lambda=None,
                 forced_playouts=None, prune_targets=None, playout_cap=None, resident=False, rounds_per_launch=64):
        self.playout_cap = self.check_playout_cap(playout_cap, n_rollouts, leaf_eval, net, root_policy, exact_from, prove,
                                                  td_lambda)
        vars(self).update(TreeSearch.check_search(leaf_eval, net, leaves, virtual_loss, eval_symmetries, root_policy,
                                                  max_considered, c_visit, c_scale, exact_from, prove, forced_playouts,
                                                  resident, rounds_per_launch))
        if self.resident and playout_cap is not None:
            raise ValueError("resident=True with playout_cap: the cap's two groups are searched in subset rounds, "
                             "which the fused launch does not run")
        self.value_mode, self.value_lambda = self.check_value_args(value_mix, td_lambda, value_targets)
        self.exact_targets = self.check_exact_targets(exact_targets, value_targets)
        self.exact_policy = bool(exact_policy)
        self.prune_targets = self.check_prune_targets(self.forced_playouts, prune_targets)
        self.num_games, self.n_rollouts = int(num_games), int(n_rollouts)
        self.num_simulations, self.net = int(num_simulations), net
        self.alpha, self.c_puct, self.seed, self.compact = float(alpha), float(c_puct), int(seed), bool(compact)
        self.v_first, self.v_second = (float(x) for x in value_targets)
        if self.num_games < 0 or self.n_rollouts < 1:
            raise ValueError("num_games must be >= 0 and n_rollouts >= 1")
        if not (0.0 < self.alpha < float("inf")):
            raise ValueError("alpha must be positive and finite")
        if not all(abs(x) < float("inf") for x in (self.v_first, self.v_second)):
            raise ValueError("value_targets must be finite")
        self.root_noise = None if root_noise is None else tuple(float(x) for x in root_noise)
        self.temperature, self.sample_plies = float(temperature), int(sample_plies)
        if self.root_noise is not None:
            if len(self.root_noise) != 2 or not 0.0 <= self.root_noise[0] <= 1.0 \
                    or not 0.0 < self.root_noise[1] < float("inf"):
                raise ValueError("root_noise must be None or (epsilon in [0, 1], alpha positive and finite)")
        if not 0.0 < self.temperature < float("inf"):
            raise ValueError("temperature must be positive and finite")
        if not 0 <= self.sample_plies <= ROWS:
            raise ValueError("sample_plies must be in 0..%d" % ROWS)
        if self.root_policy == "gumbel" and (self.root_noise is not None or self.sample_plies > 0):
            raise ValueError('root_policy="gumbel" takes neither root_noise nor sample_plies: Gumbel noise is the exploration')
        if self.root_policy == "gumbel" and self.n_rollouts < 2:
            raise ValueError('root_policy="gumbel" needs n_rollouts >= 2: the rollout that gives the root its priors, then the budget')
        R = self.n_rollouts
        if self.compact:
            self.carry = 2 * R + 2 if carry is None else int(carry)
            if self.carry < 0:
                raise ValueError("carry must be >= 0")
            self.capacity = 2 * R + self.carry
        else:
            if carry is not None:
                raise ValueError("carry needs compact=True")
            self.carry, self.capacity = None, 1 + ROWS * (2 * R + 1)
        if device is None:
            device = net.device if net is not None else "cuda"
        self._open(resolve_device(device, "SelfPlay"))
        if net is not None:
            check_net(net, self.device)
        self.plays = 0                # play() calls so far: the default seed of the next
        self.env = self.tree = None   # the last play()'s or stream()'s environment (at its positions) and trees
        self._stream = None           # stream()'s games in progress: environment, trees, staging batch, counters
        self._cap_full = None         # the last capped search's mask full u8[G], on the device
        self.stream_epoch_plies = None    # None: a seed serves as many plies as the draw counters allow (epoch_plies)

    @staticmethod
    def check_playout_cap(playout_cap, n_rollouts, leaf_eval, net, root_policy, exact_from, prove, td_lambda):
        """The constructor's check of playout_cap: None, or (p, n_fast) as (float, int)."""
        if playout_cap is None:
            return None
        try:
            p, n_fast = playout_cap
        except (TypeError, ValueError):
            raise ValueError("playout_cap must be None or (p, n_fast)") from None
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 < float(p) <= 1.0:
            raise ValueError("playout_cap: p must be a number in (0, 1]")
        if isinstance(n_fast, bool) or not isinstance(n_fast, int) or not 1 <= n_fast <= int(n_rollouts):
            raise ValueError("playout_cap: n_fast must be an integer in 1..n_rollouts")
        if leaf_eval != "value" or net is None:
            raise ValueError('playout_cap needs a net and leaf_eval="value": the two groups are searched in subset rounds')
        if TreeSearch.subset_refused(root_policy, exact_from, prove):
            raise ValueError('playout_cap is not available with root_policy="gumbel", exact_from or prove: their kernels '
                             "index their records by game, not by a subset's dense rows")
        if td_lambda is not None:
            raise ValueError("playout_cap is not available with td_lambda: TD(lambda) chains consecutive plies, and the "
                             "recorded rows are no longer consecutive")
        return float(p), int(n_fast)

    @staticmethod
    def check_prune_targets(forced_playouts, prune_targets):
        """The constructor's check of prune_targets: a bool; None stands for "exactly when forced_playouts is given"."""
        if prune_targets is None:
            return forced_playouts is not None
        if not isinstance(prune_targets, bool):
            raise ValueError("prune_targets must be True or False")
        if prune_targets and forced_playouts is None:
            raise ValueError("prune_targets=True needs forced_playouts: it subtracts the visits that forcing added")
        return prune_targets

    @staticmethod
    def check_min_ply(m, what):
        if isinstance(m, bool) or not isinstance(m, (int, float)) or int(m) != m or \
                not _native.SELFPLAY_EXACT_MIN_PLY <= int(m) <= _native.SELFPLAY_EXACT_MAX_PLY:
            raise ValueError("%s must be an integer in %d..%d (moves played): below six one board is milliseconds of work, "
                             "which VecEnv.solve is for" % (what, _native.SELFPLAY_EXACT_MIN_PLY,
                                                            _native.SELFPLAY_EXACT_MAX_PLY))
        return int(m)

    @staticmethod
    def check_exact_targets(exact_targets, value_targets):
        """The constructor's check of exact_targets: None, or the least number of moves played of a relabelled row."""
        if exact_targets is None:
            return None
        m = SelfPlay.check_min_ply(exact_targets, "exact_targets")
        if tuple(float(x) for x in value_targets) != (1.0, -1.0):
            raise ValueError("exact_targets needs value_targets=(1.0, -1.0): the exact value is the mover's, in [-1, 1], and "
                             "the reference's (1, 0) is not zero-sum, so the relabelled rows would be on another scale "
                             "than the rest of the batch")
        return m

    @staticmethod
    def check_value_args(value_mix, td_lambda, value_targets):
        """The constructor's check of value_mix and td_lambda: (None, None), or ("mix" | "td", lambda)."""
        if value_mix is None and td_lambda is None:
            return None, None
        if value_mix is not None and td_lambda is not None:
            raise ValueError("at most one of value_mix and td_lambda may be given")
        what, mode, lam = ("value_mix", "mix", value_mix) if td_lambda is None else ("td_lambda", "td", td_lambda)
        lam = SelfPlayBatch.check_lambda(lam, what)
        if tuple(float(x) for x in value_targets) != (1.0, -1.0):
            raise ValueError("%s needs value_targets=(1.0, -1.0): the searched value is the mover's, in [-1, 1], "
                             "and the reference's (1, 0) is not zero-sum, so the mixed v would be on two scales" % what)
        return mode, lam

    def new_batch(self):
        """A zero-filled SelfPlayBatch for num_games games; with value_mix or td_lambda it has the q rows."""
        batch = SelfPlayBatch(self.num_games, self.device, self._lib.qttt_state_bytes(self.num_games))
        if self.value_mode is not None:
            batch.alloc_q()
        return batch

    def record_value(self, tree, ply, batch):
        """One qttt_selfplay_record_value, BEFORE the ply's record(): the searched value of every root that record is about
        to write goes to row `ply` of batch.q (ply=None: the stream form, row length[g]); a root without a visit gets the
        row's v."""
        G, dev = self.num_games, self.device
        if tree.num_games != G or tree.device != dev or batch.num_games != G:
            raise ValueError("tree and batch must hold %d games on %s" % (G, dev))
        if getattr(batch, "q", None) is None:
            raise ValueError("the batch has no q: alloc_q() first")
        check_tensor(batch.q, torch.float32, (ROWS, G), dev, "batch.q")
        check_tensor(batch.v, torch.float32, (ROWS, G), dev, "batch.v")
        check_tensor(batch.length, torch.uint8, (G,), dev, "batch.length")
        self._call("qttt_selfplay_record_value", tree.tree.data_ptr(), G, tree.capacity, -1 if ply is None else int(ply),
                   batch.length.data_ptr(), batch.q.data_ptr(), batch.v.data_ptr())
        return batch.q

    # mode -> (the entry's suffix, what it takes after the outputs); draw: (the draw index,) in the per-game form, else ().
    # The pruned record takes the sampled record's arguments (sample_plies = 0: no draw is taken), then the prune's.
    _RECORD_MODES = {
        "plain": ("", lambda sp, t, draw: ()),
        "sampled": ("_sampled", lambda sp, t, draw: (t.seed, t.board_offset, sp.temperature, sp.sample_plies) + draw),
        "pruned": ("_pruned", lambda sp, t, draw: (t.seed, t.board_offset, sp.temperature, sp.sample_plies) + draw
                   + (sp.forced_playouts, t.c_puct)),
        "gumbel": ("_gumbel", lambda sp, t, draw: (t._gumbel["rec"].data_ptr(), t.c_visit, t.c_scale)),
    }

    def record(self, tree, ply, batch, draw_index=None):
        """One qttt_selfplay_record: the roots of `tree` become row `ply` of `batch`; returns batch.actions, the move
        to step with.  With sample_plies > 0 it is qttt_selfplay_record_sampled, drawing with the tree's seed and
        board_offset.  With prune_targets it is qttt_selfplay_record_pruned: the same move, the pi row pruned with the
        tree's c_puct.  ply=None is the stream record (include/qttt_selfplay_stream.h): every game's row is its own
        length[g].  draw_index (the sampled move's draw, where it is not the ply: stream() and play(start_ply=p)) goes
        through the stream record too, which writes a lockstep batch's rows exactly as the lockstep entry does."""
        G, dev = self.num_games, self.device
        if tree.num_games != G or tree.device != dev or batch.num_games != G:
            raise ValueError("tree and batch must hold %d games on %s" % (G, dev))
        check_tensor(batch.states, torch.uint8, (ROWS, int(self._lib.qttt_state_bytes(G))), dev, "batch.states")
        for k, (dt, shp) in SelfPlayBatch._ROWS.items():
            check_tensor(getattr(batch, k), dt, (ROWS, G) + shp, dev, "batch." + k)
        check_tensor(batch.length, torch.uint8, (G,), dev, "batch.length")
        check_tensor(batch.winner, torch.int8, (G,), dev, "batch.winner")
        check_tensor(batch.actions, torch.uint8, (G, 2), dev, "batch.actions")
        sampled = self.root_policy != "gumbel" and self.sample_plies > 0
        per_game = ply is None or (sampled and draw_index is not None)
        if sampled and ply is None and draw_index is None:
            raise ValueError("the sampled stream record needs a draw_index")
        if self.prune_targets and tree.root_policy == "gumbel":
            raise ValueError("the pruned record needs a tree searched with the PUCT root")
        mode = "gumbel" if self.root_policy == "gumbel" else "pruned" if self.prune_targets else "sampled" if sampled else "plain"
        if mode == "gumbel" and (tree.root_policy != "gumbel" or tree._gumbel is None):
            raise ValueError("the Gumbel record needs a tree searched with root_policy=\"gumbel\"")
        suffix, extra = self._RECORD_MODES[mode]
        self._call(("qttt_selfplay_record_stream" if per_game else "qttt_selfplay_record") + suffix,
                   tree.tree.data_ptr(), G, tree.capacity, *(() if per_game else (int(ply),)),
                   self.n_rollouts, self.alpha, self.v_first, self.v_second, *self._staging(batch, SelfPlayBatch._FIELDS),
                   *extra(self, tree, (int(draw_index or 0),) if per_game else ()))
        return batch.actions

    def search_kwargs(self):
        """The search keywords that TreeSearch takes from a SelfPlay: what its trees, and a Reanalyser's, are built with."""
        return {k: getattr(self, k) for k in TreeSearch.SEARCH_KEYS}

    def _new_game_objects(self, s):
        """The environment (seed s) and the trees (seed 2 s + 1) of a play() or a stream, the trees reset at the empty
        boards."""
        env = VecEnv(self.num_games, device=self.device, seed=s)
        tree = TreeSearch(self.num_games, capacity=self.capacity, seed=2 * s + 1, device=self.device, **self.search_kwargs())
        tree.reset(env)
        return env, tree

    def _search(self, tree):
        """The search before a move, play()'s and stream()'s: R rollouts, with root_noise the noise after the one that
        gives the priors."""
        R = self.n_rollouts
        if self.root_noise is None:
            tree.contemplate(R)
        else:
            tree.contemplate(1)
            tree.add_root_noise(*self.root_noise)
            tree.contemplate(R - 1)

    def _search_capped(self, tree, ply_index):
        """The search of one capped ply (playout_cap): returns full u8[G] on the device, the record's mask.  The draw is
        the host's (include/qttt_selfplay_cap.h), addressed by (the trees' seed, board_offset + g, ply_index); the mask and
        the two id lists are uploaded from pinned memory and nothing waits for the device."""
        (p, n_fast), R, G = self.playout_cap, self.n_rollouts, self.num_games
        full = torch.from_numpy(cap_full_mask(tree.seed, tree.board_offset, G, ply_index, p))
        mask = full.pin_memory().to(self.device, non_blocking=True)
        group_full, group_fast = tree.subset(full), tree.subset(1 - full)
        tree.contemplate(1)
        if self.root_noise is not None:
            tree.add_root_noise(*self.root_noise, games=group_full)
        # a game is in one group: both groups take the rollout indices after the first, and no game more than R - 1 of them
        tree.contemplate_groups(R - 1, [(group_fast, n_fast - 1, False), (group_full, R - 1, None)])
        return mask

    def record_capped(self, tree, batch, full, draw_index=0):
        """One qttt_selfplay_record_capped (include/qttt_selfplay_cap.h): record(tree, None, batch, draw_index) for the live
        games with full[g] != 0 or a terminal root; a fast game's move goes to batch.actions and nothing else is written.
        full u8[G] on the device.  The pi row is the pruned one with prune_targets, else the plain one."""
        G, dev = self.num_games, self.device
        if tree.num_games != G or tree.device != dev or batch.num_games != G:
            raise ValueError("tree and batch must hold %d games on %s" % (G, dev))
        check_tensor(full, torch.uint8, (G,), dev, "full")
        self._call("qttt_selfplay_record_capped", tree.tree.data_ptr(), G, tree.capacity, self.n_rollouts, self.alpha,
                   self.v_first, self.v_second, *self._staging(batch, SelfPlayBatch._FIELDS), tree.seed, tree.board_offset,
                   self.temperature, self.sample_plies, int(draw_index),
                   self.forced_playouts if self.prune_targets else -1.0, tree.c_puct, full.data_ptr())
        return batch.actions

    def epoch_plies(self, tree):
        """Searched plies that one seed serves before one of the draw counters would pass its limit: the environment's
        step index (u32), the trees' rollout index (R per ply), the noise and Gumbel indices and the sampled move's
        (one per ply each).  stream() moves to a fresh seed after that many plies; play(start_ply=p) needs p + 10 of
        them.  stream_epoch_plies, when set, replaces it by something smaller (tests)."""
        limits = [1 << 32, tree.max_rollouts // self.n_rollouts, _native.SELFPLAY_MAX_MOVE_DRAWS]
        if self.root_noise is not None:
            limits.append(_native.TREE_MAX_NOISE)
        if self.playout_cap is not None:
            limits.append(_native.SELFPLAY_MAX_CAP_DRAWS)
        if self.root_policy == "gumbel":
            limits.append(_native.TREE_MAX_GUMBEL)
        n = min(limits)
        return n if self.stream_epoch_plies is None else min(n, int(self.stream_epoch_plies))

    def _set_counters(self, env, tree, p):
        """Every draw counter at what p searched plies since the seed's first consume: the environment's step index, the
        trees' rollout index, and the noise and Gumbel indices where the search uses them."""
        env.step_idx = p
        tree.rollout_idx = p * self.n_rollouts
        tree.noise_idx = p if self.root_noise is not None else 0
        tree.gumbel_idx = p if self.root_policy == "gumbel" else 0

    def _ply(self, env, tree, batch, row, index, search=True):
        """One ply, play()'s and stream()'s: the search (capped or not; none where search is False), record_value, the record,
        the step, the sync and the compaction.  row: the batch row, or None for the record at every game's own length[g]
        (stream(), and every capped ply: a capped batch's rows are per game).  index: the ply's number since the seed's
        first, which addresses the cap's draw and the sampled move's."""
        capped = self.playout_cap is not None
        if capped:
            row = None
        if search:
            if capped:
                self._cap_full = self._search_capped(tree, index)
            else:
                self._search(tree)
            if self.value_mode is not None:
                self.record_value(tree, row, batch)
        if capped:      # an unsearched ply (play()'s last: every root is terminal and recorded as such) reads no bit of the mask
            actions = self.record_capped(tree, batch, self._cap_full, draw_index=index)
        else:
            actions = self.record(tree, row, batch, draw_index=None if row == index else index)
        env.step_raw(actions)
        tree.sync(env)
        if self.compact:
            tree.compact()

    def play(self, seed=None, start_ply=0):
        """play_game (self_play.py:43-76) of num_games games from the empty board and their samples
        (self_play.py:193-216) as a SelfPlayBatch.  seed=None: self.seed + the number of earlier play() calls.  The
        environment draws its collapse bits with `seed`, the trees their playouts with 2 * seed + 1.  A finished game
        rides along: its moves are noops, its tree keeps its root.
        start_ply=p > 0 plays the same games with every draw counter started at what p plies of a stream() consume
        (the environment's step index, the trees' rollout, noise and Gumbel indices, the sampled move's index) instead
        of 0: the games that a stream with this seed starts at its ply p.  With 0 the calls are what they always were."""
        s = self.seed + self.plays if seed is None else int(seed)
        p = int(start_ply)
        if p < 0:
            raise ValueError("start_ply must be >= 0")
        self.plays += 1
        env, tree = self.env, self.tree = self._new_game_objects(s)
        if p:
            if p + ROWS > self.epoch_plies(tree):
                raise ValueError("start_ply %d passes the draw counters' limit of %d plies" % (p, self.epoch_plies(tree)))
            self._set_counters(env, tree, p)
        batch = self.new_batch()
        for ply in range(ROWS):                 # at ply 9 every game is over: nine moves fill the board
            self._ply(env, tree, batch, ply, p + ply, search=ply < ROWS - 1)
        if self.exact_targets is not None:
            batch.exact = batch.exact_targets(self.exact_targets, self.exact_policy)
        if self.value_mode is not None:
            batch.value_targets(self.value_mode, self.value_lambda, exact=getattr(batch, "exact", None))
        return batch

    # ------------------------------------------------------------------ continuous self-play
    def stream_reset(self):
        """Forgets the games of stream(): the next call starts every slot from the empty board, with fresh counters."""
        self._stream = None

    def stream(self, ring, plies, seed=None):
        """Advances the persistent batch of num_games game slots by `plies` stream plies (include/qttt_selfplay_stream.h).
        One stream ply: the search of play() in every slot (every root is live) -> the record at each slot's OWN ply
        (row length[g] of the staging batch) -> step, sync [, compact] -> harvest: a slot whose new root is terminal
        gets its terminal row and value targets, its rows are appended to `ring` (a ReplayBuffer on this device; slots
        ascending, rows in order; with exact_targets relabelled first), and the slot restarts from the empty board.
        Three launches and the append's on top of play()'s per ply, and no host read-back (compact=True keeps its one per
        move).
        The first call (and the first after stream_reset()) starts every slot from the empty board with `seed`
        (None: self.seed + the number of earlier play() / stream starts); later calls continue the games in progress,
        and take seed=None or the running stream's.  The draw counters run on across restarts and calls, so no
        (seed, board, index) is used twice: until a slot first finishes its game is play(seed)'s in that slot, and a
        game that starts at stream ply p is play(seed, start_ply=p)'s.  After epoch_plies() plies the stream moves to
        the seed `seed + 2**32` (and so on) with the counters at 0; games in progress carry on.
        Returns StreamStats: games i64[G] finished per slot, samples i64 rows appended, winners i64[3] first / second /
        none, all cumulative since the stream began, device tensors that nothing here reads back."""
        from .replay import ReplayBuffer
        T = int(plies)
        if T < 0:
            raise ValueError("plies must be >= 0")
        if not isinstance(ring, ReplayBuffer) or ring.device != self.device:
            raise ValueError("ring must be a ReplayBuffer on %s" % (self.device,))
        st = self._stream
        if st is None:
            s = self.seed + self.plays if seed is None else int(seed)
            self.plays += 1
            st = self._stream = self._stream_begin(s)
        elif seed is not None and int(seed) != st["seed"]:
            raise ValueError("a stream with seed %d is in progress: stream_reset() first" % st["seed"])
        self.env, self.tree = st["env"], st["tree"]
        for _ in range(T):
            self._stream_ply(st, ring)
        totals = st["tally"].sum(0)
        return StreamStats(st["games_done"].clone(), totals[3], totals[:3])

    def _stream_begin(self, s):
        G, dev = self.num_games, self.device
        env, tree = self._new_game_objects(s)
        return {"seed": s, "epoch": 0, "ply": 0, "plies": 0, "env": env, "tree": tree, "batch": self.new_batch(),
                "harvest_len": torch.zeros(G, dtype=torch.uint8, device=dev),
                "finished": torch.zeros(G, dtype=torch.uint8, device=dev),
                "games_done": torch.zeros(G, dtype=torch.int64, device=dev),
                "tally": torch.zeros((G, _native.SELFPLAY_TALLIES), dtype=torch.int64, device=dev)}

    def _stream_ply(self, st, ring):
        env, tree, batch, R = st["env"], st["tree"], st["batch"], self.n_rollouts
        if st["ply"] >= self.epoch_plies(tree):         # a counter would pass its limit: a fresh seed, the counters at 0
            st["epoch"] += 1
            s = st["seed"] + (st["epoch"] << 32)
            env.seed = s
            tree.reseed(2 * s + 1)
            st["ply"] = 0
            self._set_counters(env, tree, 0)
        if not self.compact:
            # what the host cannot know without a read-back, it knows from the game: a live root has at most eight moves
            # behind it, and a restart gives the slot's nodes back, so no slot holds more than this before its search
            tree._bound = 1 + (ROWS - 2) * (2 * R + 1)
        self._ply(env, tree, batch, None, st["ply"])
        self._stream_harvest(st)
        exact = None
        if self.exact_targets is not None:          # only the games this ply hands to the ring, once each
            if self.value_mode is not None:         # the value targets need to know which rows hold the truth
                exact = st.get("exact")
                if exact is None:
                    exact = st["exact"] = torch.empty((ROWS, self.num_games), dtype=torch.uint8, device=self.device)
            batch._exact_targets(self.exact_targets, self.exact_policy, st["harvest_len"], exact)
        if self.value_mode is not None:
            batch.value_targets(self.value_mode, self.value_lambda, rows=st["harvest_len"], exact=exact)
        ring.add(batch, length=st["harvest_len"])
        self._stream_restart(st)
        st["ply"] += 1
        st["plies"] += 1

    def _staging(self, batch, fields):
        return [getattr(batch, f).data_ptr() for f in fields]

    def _stream_harvest(self, st):
        tree = st["tree"]
        self._call("qttt_selfplay_harvest" if self.playout_cap is None else "qttt_selfplay_harvest_capped", tree.tree.data_ptr(), self.num_games, tree.capacity, self.v_first, self.v_second,
                   *self._staging(st["batch"], SelfPlayBatch._FIELDS), st["harvest_len"].data_ptr(),
                   st["finished"].data_ptr(), st["games_done"].data_ptr(), st["tally"].data_ptr())

    def _stream_restart(self, st):
        tree = st["tree"]
        self._call("qttt_selfplay_restart", tree.tree.data_ptr(), self.num_games, tree.capacity, st["env"].state.data_ptr(),
                   st["finished"].data_ptr(), *self._staging(st["batch"], SelfPlayBatch._FIELDS[:7]))


class StreamStats:
    """What SelfPlay.stream() returns: games i64[G] (finished per slot), samples i64 (rows appended) and winners i64[3]
    (first player / second player / nobody), cumulative since the stream began; device tensors."""

    def __init__(self, games, samples, winners):
        self.games, self.samples, self.winners = games, samples, winners

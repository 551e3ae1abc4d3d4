"""TreeSearch — the reference's MCTS / AlphaZero search tree (mcts.py:132-337, alphazero.py shares the tree code) for
G independent games, kept on the device (include/qttt_tree.h).

A rollout is select -> playouts from the leaf (VecEnv.rollout_many, or VecEnv.rollout_policy under a network) ->
backup, three launches on the current stream with no host synchronisation.  leaf_eval="value" is the standard AlphaZero
search instead (include/qttt_tree_value.h): the leaf's value is the network's value head and its priors
the policy head, one evaluation fused with the backup, so a rollout is select -> value rollout, two launches and no
playout.  Nodes that sync leaves behind stay
allocated until compact() (the reference's _prune) gives them back: with a compact() after every sync, `capacity` has
to hold the kept subtree and one move's rollouts; without it, every rollout and sync since the last reset.  The host
keeps an upper bound on the nodes used (+2 per rollout, +1 per sync; compact() replaces it by the real maximum) and
raises ValueError before launching work that could pass it.

leaves=K > 1 (value leaves only) is the leaf-parallel search (include/qttt_tree_leaves.h): a round of K
rollouts is select_batch -> VecEnv.evaluate on the G * K leaves -> backup_batch, three launches; the K descents of a game
are kept apart by `virtual_loss`, which lives in spare bits of the visit counts between the two tree launches of a round
and never touches W.

eval_symmetries (value leaves only) averages the network over every leaf's images under the board's symmetries
(include/qttt_nn_symmetric.h): every rollout is then such a round, a round of one leaf where leaves == 1.

root_policy="gumbel" (value leaves only) is the Gumbel root (include/qttt_tree_gumbel.h): contemplate(n)
samples max_considered actions without replacement with Gumbel noise, spends the n simulations on them by sequential
halving, rounds of `leaves` at a time, and choose() / root_stats() give the best survivor and the improved policy
softmax(logits + sigma(completed Q)).  Below the root the search is the leaf-parallel one.

exact_from=M (value leaves only) gives the search exact leaves (include/qttt_tree_exact.h): a leaf with at
least M moves played is solved on the device, once, by the endgame solver's definition, backed up with its exact value
instead of the network's, and stays a leaf.  Every rollout is then a round with qttt_tree_solve_leaves between the
evaluation and the backup.

prove=True (with exact_from) proves interior nodes as well (include/qttt_tree_prove.h): after every round's
backup qttt_tree_prove walks the round's paths upwards and solves each node all of whose legal actions lead to terminal or
solved children, with the solver's own formula; a proven node below the root ends every later descent like an exact leaf.
root_stats() then says which root actions are proven and their exact q, and choose(exact=True) plays the solver's move at
a proven root.

forced_playouts=k (value leaves only, the PUCT root) is KataGo's remedy for noise at small budgets
(include/qttt_tree_forced.h): at the root a visited action a with n(a)^2 < k P(a) sum(n) is searched before
the PUCT choice.  Every rollout after the first of a reset() or sync() is then a leaf-parallel round through
qttt_tree_select_batch_forced, and root_stats() says which actions are forced now and what the pruned policy target would
keep of the visits.

contemplate(n, games=...) and add_root_noise(..., games=...) search and noise a listed subset of the games
(include/qttt_tree_subset.h): the listed games' leaves are packed densely, so a round's network launch has
n_ids * K rows and the other games cost nothing and keep every byte.  contemplate_groups(n, groups) searches several disjoint
subsets from the same rollout index, each with a budget and a root rule of its own: what SelfPlay(playout_cap=) is made of.

Every one of these searches follows one plan, search_plan(): one single rollout while the roots are fresh, then rounds of
`leaves`, then one shorter round.  _round() is the one round — select, one evaluation, backup — of the plain, forced, Gumbel
and subset forms, and contemplate() the one place where the node bound advances.

resident=True (value leaves, the PUCT root) is the resident search (include/qttt_tree_resident.h): after the
single rollout that follows a reset() or sync(), contemplate() runs its rounds — the same rounds, the same draws, the same
bytes — inside launches of qttt_tree_search_resident, at most rounds_per_launch rounds each, instead of three launches a
round.

add_root_noise() is AlphaZero's root exploration (include/qttt_tree_explore.h): Dirichlet noise mixed into
the priors of every root that has them, one launch.
"""
import torch

from . import _native
from ._host import LibCaller, _ptr, check_net, check_tensor, out_rows, out_tensor, resolve_device
from .symmetry import check_eval_symmetries
from .vec_env import VecEnv


def search_plan(rollouts, leaves, fresh, rounds=True):
    """The plan of a search of `rollouts` rollouts, every path's of TreeSearch.contemplate: (singles, sizes).  A search in
    rounds (rounds=True) takes one single rollout while the roots are fresh — no contemplate since the last reset() or
    sync(): K descents would all end on a root without priors — then rounds of K = leaves and one shorter round for what
    is left.  A search without rounds (leaves == 1 at the plain PUCT root, outside the resident search) is `rollouts`
    singles.  What a single is — _rollout, or a round of one leaf — is the caller's; it counts one rollout and two nodes
    either way, so singles + sum(sizes) == rollouts and the node bound advances by 2 * rollouts."""
    r, K = int(rollouts), int(leaves)
    if not rounds:
        return r, []
    singles = 1 if r and fresh else 0
    r -= singles
    return singles, [K] * (r // K) + [r % K] * (r % K > 0)


class TreeSearch(LibCaller):
    # the roots' statistics (qttt_tree_root): name -> (dtype, per-game shape)
    _ROOT_ROWS = {"N": (torch.int32, (36,)), "W": (torch.float64, (36,)), "Q": (torch.float64, (36,)),
                  "P": (torch.float64, (36,)), "Ntot": (torch.int32, ()), "choose": (torch.uint8, ()),
                  "nodes_used": (torch.int32, ()), "overflow": (torch.uint8, ())}

    # what prove=True adds to them (qttt_tree_root_exact): key -> (dtype, per-game shape)
    _EXACT_ROWS = {"q_exact": (torch.float32, (36,)), "proven": (torch.uint8, (36,)),
                   "root_value_exact": (torch.float32, ()), "root_solved": (torch.uint8, ())}

    # what the Gumbel root adds to them (qttt_tree_gumbel_root)
    _GUMBEL_ROWS = {"choose": (torch.uint8, ()), "pi": (torch.float64, (36,)), "q_completed": (torch.float64, (36,))}

    # what forced_playouts adds to them (qttt_tree_root_forced)
    _FORCED_ROWS = {"forced": (torch.uint8, (36,)), "n_pruned": (torch.int32, (36,))}

    LEAF_EVALS = ("playouts", "value")
    ROOT_POLICIES = ("puct", "gumbel")
    leaf_eval = "playouts"
    root_policy = "puct"
    eval_symmetries = None
    exact_from = None
    prove = False
    forced_playouts = None
    resident = False
    rounds_per_launch = 64

    def __init__(self, num_games, capacity, num_simulations=10, c_puct=1.0, net=None, seed=0, board_offset=0,
                 device=None, leaf_eval="playouts", leaves=1, virtual_loss=1.0, eval_symmetries=None, root_policy="puct",
                 max_considered=16, c_visit=50.0, c_scale=1.0, exact_from=None, prove=False, forced_playouts=None,
                 resident=False, rounds_per_launch=64):
        """leaf_eval="playouts": the reference's rollout, num_simulations playouts from the leaf (uniform, or guided by
        `net`).  leaf_eval="value" (needs `net`): the leaf is scored by the value head, seen by the player to move
        there; a terminal leaf by its reward.  num_simulations is then ignored: no playout draw is taken.
        leaves=K > 1 (needs leaf_eval="value"): contemplate() searches K leaves per game per round, each descent counted
        as a loss of `virtual_loss` by the ones after it until the round is backed up.  leaves=1 is the search as it
        always was.
        eval_symmetries ("all" or 1, 2, 4 or 8 symmetries 0..7; needs leaf_eval="value"): every leaf's value and priors are
        the network's mean over the leaf's images under them (VecEnv.evaluate(symmetries=...)).  Every
        rollout is then a round — select_batch, evaluate, backup_batch — a round of one leaf where leaves == 1.
        root_policy="gumbel" (needs leaf_eval="value"): the root considers max_considered actions drawn with Gumbel noise
        and halves them down over the budget of a contemplate(); sigma(q) = (c_visit + max N) * c_scale * q weighs the
        completed Q against the logits.  root_policy="puct" is the search as it always was.
        exact_from=M (6..9; needs leaf_eval="value"): a leaf below the root with at least M moves played is solved
        exactly on the device the first time a round ends on it, and is from then on a leaf with that value: it is backed
        up with it and never gets priors or children.  Every rollout is then a round — select_batch, evaluate,
        solve_leaves, backup_batch_exact — also the first after a reset() or sync().  None is the search as it always was.
        prove=True (needs exact_from; 9 is allowed: only terminal children prove anything then): every round ends with
        qttt_tree_prove, a fifth launch, which solves the nodes on the round's paths whose children are all terminal or
        solved.  A proven node below the root loses its priors, so descents end on it and it is backed up with its exact
        value; the root keeps its priors.  False is the search as it always was.
        forced_playouts=k (finite, >= 0; needs a net and leaf_eval="value"; not with root_policy="gumbel"): a legal root
        action a with n(a) > 0 and n(a) * n(a) < (k * P(a)) * sum(n) is forced: the descent takes the forced action of
        largest score before it looks at the others (n counts the visits in flight).  contemplate() then runs one single
        rollout where the roots may lack priors and rounds of `leaves` through qttt_tree_select_batch_forced after it, a
        round of one leaf where leaves == 1.  k = 0 forces nothing.  None is the search as it always was.
        resident=True (needs a net and leaf_eval="value"; not with root_policy="gumbel", exact_from, prove or
        eval_symmetries): contemplate() runs the single rollout after a reset() or sync() as always and every round after
        it inside qttt_tree_search_resident, one launch per rounds_per_launch (>= 1) rounds; rounds of `leaves` also at
        leaves == 1.  rounds_per_launch bounds one launch's duration on a shared device and does not change a byte.
        forced_playouts, add_root_noise(), compact(), choose(), root_stats() and sync() compose; contemplate(games=...)
        does not.  False is the search as it always was, every call, buffer and launch."""
        vars(self).update(self.check_search(leaf_eval, net, leaves, virtual_loss, eval_symmetries, root_policy, max_considered,
                                            c_visit, c_scale, exact_from, prove, forced_playouts, resident, rounds_per_launch))
        self.num_games, self.capacity = int(num_games), int(capacity)
        self.num_simulations, self.c_puct = int(num_simulations), float(c_puct)
        self.net, self.seed, self.board_offset = net, int(seed), int(board_offset)
        if self.num_games < 0 or not 1 <= self.capacity <= _native.TREE_MAX_CAPACITY:
            raise ValueError("num_games must be >= 0 and capacity in 1..%d" % _native.TREE_MAX_CAPACITY)
        limit = _native.POLICY_ROLLOUT_MAX_SIMS if net is not None else _native.TREE_MAX_SIMS
        if leaf_eval != "value" and not 1 <= self.num_simulations <= limit:
            raise ValueError("num_simulations must be in 1..%d" % limit)
        if self.board_offset < 0:
            raise ValueError("board_offset must be >= 0")
        if device is None:
            device = net.device if net is not None else "cuda"
        self._open(resolve_device(device, "TreeSearch"))
        if net is not None:
            check_net(net, self.device)
        G, S, dev = self.num_games, self.num_simulations, self.device
        nbytes = int(self._lib.qttt_tree_bytes(G, self.capacity))
        if nbytes < 0:
            raise ValueError("qttt_tree_bytes(%d, %d) failed" % (G, self.capacity))
        self.tree = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        leaf_state = torch.zeros(int(self._lib.qttt_state_bytes(G)), dtype=torch.uint8, device=dev)
        self.leaf = VecEnv.from_state(leaf_state, G, seed=self.seed, board_offset=self.board_offset)
        # what the playouts write and the backup reads (a value rollout has neither)
        if leaf_eval == "value":
            self._out = None
        elif net is None:
            self._out = out_tensor(torch.int8, (S,), G, dev)
        else:
            self._out = out_rows(VecEnv._policy_rows(S), G, dev, keys=("result", "probs"))
        self.rollout_idx = 0          # k of include/qttt_tree.h: rollouts since the last reset
        self.noise_idx = 0            # add_root_noise() calls since the last reset: what addresses their draws
        self._bound = None            # upper bound on the nodes used (None: not reset yet)
        self._scratch = None          # compact()'s forwarding table, allocated by its first call
        self._rounds = {}             # k -> the buffers of a round of k leaves per game, allocated by its first round
        self._fresh = True            # no contemplate since the last reset() or sync(): the root may lack priors
        self.gumbel_idx = 0           # Gumbel begins since the last reset: what addresses their draws
        self._gumbel = None           # the Gumbel root's buffers, allocated by its first begin
        self._tables = {}             # n -> the visit table i32[37, n] of a budget of n simulations, on the device
        self._subset_rounds = {}      # (n_ids, k) -> a subset round's dense buffers: views of the full round's storage

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def check_search_args(leaf_eval, net, leaves, virtual_loss):
        """What the constructors of TreeSearch and SelfPlay check of the search's form, before anything is opened;
        returns (leaves, virtual_loss) as int and float."""
        if leaf_eval not in TreeSearch.LEAF_EVALS:
            raise ValueError("leaf_eval must be one of %s" % (TreeSearch.LEAF_EVALS,))
        if leaf_eval == "value" and net is None:
            raise ValueError('leaf_eval="value" needs a net')
        leaves, virtual_loss = int(leaves), float(virtual_loss)
        if not 1 <= leaves <= _native.TREE_MAX_LEAVES:
            raise ValueError("leaves must be in 1..%d" % _native.TREE_MAX_LEAVES)
        if leaves > 1 and leaf_eval != "value":
            raise ValueError('leaves > 1 needs leaf_eval="value"')
        if not 0.0 <= virtual_loss < float("inf"):
            raise ValueError("virtual_loss must be finite and >= 0")
        return leaves, virtual_loss

    @staticmethod
    def check_root_args(leaf_eval, net, root_policy, max_considered, c_visit, c_scale):
        """The constructors' check of the root's rule; returns (root_policy, max_considered, c_visit, c_scale)."""
        if root_policy not in TreeSearch.ROOT_POLICIES:
            raise ValueError("root_policy must be one of %s" % (TreeSearch.ROOT_POLICIES,))
        max_considered, c_visit, c_scale = int(max_considered), float(c_visit), float(c_scale)
        if root_policy == "gumbel" and (leaf_eval != "value" or net is None):
            raise ValueError('root_policy="gumbel" needs a net and leaf_eval="value"')
        if not 1 <= max_considered <= 36:
            raise ValueError("max_considered must be in 1..36")
        if not 0.0 <= c_visit < float("inf"):
            raise ValueError("c_visit must be finite and >= 0")
        if not abs(c_scale) < float("inf"):
            raise ValueError("c_scale must be finite")
        return root_policy, max_considered, c_visit, c_scale

    @staticmethod
    def check_eval_symmetries(leaf_eval, eval_symmetries):
        """The constructors' check of eval_symmetries: None, or the tuple VecEnv.evaluate(symmetries=...) takes."""
        if eval_symmetries is None:
            return None
        if leaf_eval != "value":
            raise ValueError('eval_symmetries needs leaf_eval="value"')
        return check_eval_symmetries(eval_symmetries)

    @staticmethod
    def check_exact_from(leaf_eval, net, exact_from):
        """The constructors' check of exact_from: None, or the least number of moves played of an exact leaf."""
        if exact_from is None:
            return None
        if leaf_eval != "value" or net is None:
            raise ValueError('exact_from needs a net and leaf_eval="value": exact leaves replace the value head\'s estimate')
        if isinstance(exact_from, bool) or int(exact_from) != exact_from or \
                not _native.TREE_EXACT_MIN_PLY <= int(exact_from) <= _native.SOLVE_MAX_PLY:
            raise ValueError("exact_from must be None or an integer in %d..%d (moves played)"
                             % (_native.TREE_EXACT_MIN_PLY, _native.SOLVE_MAX_PLY))
        return int(exact_from)

    @staticmethod
    def check_forced_playouts(leaf_eval, net, root_policy, forced_playouts):
        """The constructors' check of forced_playouts: None, or the factor k as a float."""
        if forced_playouts is None:
            return None
        if isinstance(forced_playouts, bool) or not isinstance(forced_playouts, (int, float)) or \
                not 0.0 <= float(forced_playouts) < float("inf"):
            raise ValueError("forced_playouts must be None or a finite number >= 0")
        if leaf_eval != "value" or net is None:
            raise ValueError('forced_playouts needs a net and leaf_eval="value": the forced rounds are leaf-parallel rounds')
        if root_policy == "gumbel":
            raise ValueError('forced_playouts is a rule of the PUCT root: root_policy="gumbel" replaces that root')
        return float(forced_playouts)

    @staticmethod
    def check_resident(resident, rounds_per_launch, leaf_eval, net, root_policy, exact_from, prove, eval_symmetries):
        """The constructors' check of resident and rounds_per_launch; returns (resident, rounds_per_launch).  Every pair
        that the fused launch cannot run is refused by name."""
        if not isinstance(resident, bool):
            raise ValueError("resident must be True or False")
        if isinstance(rounds_per_launch, bool) or not isinstance(rounds_per_launch, int) or rounds_per_launch < 1:
            raise ValueError("rounds_per_launch must be an integer >= 1")
        if not resident:
            return False, rounds_per_launch
        if leaf_eval != "value" or net is None:
            raise ValueError('resident=True with leaf_eval="playouts" (or without a net): the fused launch evaluates the '
                             'leaves with the value head, it plays no playouts')
        for name, on in (('root_policy="gumbel"', root_policy == "gumbel"), ("exact_from", exact_from is not None),
                         ("prove", bool(prove)), ("eval_symmetries", eval_symmetries is not None)):
            if on:
                raise ValueError("resident=True with %s: the fused launch runs the PUCT (or forced) select, one plain "
                                 "evaluation and the plain backup, nothing between them" % name)
        return True, rounds_per_launch

    @staticmethod
    def check_prove(exact_from, prove):
        """The constructors' check of prove: a bool, True only with exact_from."""
        if not isinstance(prove, bool):
            raise ValueError("prove must be True or False")
        if prove and exact_from is None:
            raise ValueError("prove=True needs exact_from: the plain backup would hand a proven node its priors back")
        return prove

    # what a SelfPlay hands to its trees, and a Reanalyser to its own: SelfPlay.search_kwargs()
    SEARCH_KEYS = ("num_simulations", "c_puct", "net", "leaf_eval", "leaves", "virtual_loss", "eval_symmetries", "root_policy",
                   "max_considered", "c_visit", "c_scale", "exact_from", "prove", "forced_playouts", "resident",
                   "rounds_per_launch")

    @staticmethod
    def check_search(leaf_eval, net, leaves, virtual_loss, eval_symmetries, root_policy, max_considered, c_visit, c_scale,
                     exact_from, prove, forced_playouts, resident, rounds_per_launch):
        """The search keywords' checks, every check_* above, for the constructors of TreeSearch and SelfPlay alike, before
        anything is opened; returns name -> normalised value for every SEARCH_KEYS name but num_simulations, c_puct and net.
        The order is one: resident, forced_playouts, exact_from, prove, the search's form, the root's rule, eval_symmetries.
        An input with several bad keywords is refused for the first of them in that order, by either constructor."""
        T, o = TreeSearch, {"leaf_eval": leaf_eval}
        o["resident"], o["rounds_per_launch"] = T.check_resident(resident, rounds_per_launch, leaf_eval, net, root_policy,
                                                                 exact_from, prove, eval_symmetries)
        o["forced_playouts"] = T.check_forced_playouts(leaf_eval, net, root_policy, forced_playouts)
        o["exact_from"] = T.check_exact_from(leaf_eval, net, exact_from)
        o["prove"] = T.check_prove(o["exact_from"], prove)
        o["leaves"], o["virtual_loss"] = T.check_search_args(leaf_eval, net, leaves, virtual_loss)
        o["root_policy"], o["max_considered"], o["c_visit"], o["c_scale"] = T.check_root_args(
            leaf_eval, net, root_policy, max_considered, c_visit, c_scale)
        o["eval_symmetries"] = T.check_eval_symmetries(leaf_eval, eval_symmetries)
        return o

    @staticmethod
    def subset_refused(root_policy, exact_from, prove):
        """Whether a search with these keywords cannot search a subset of its games (contemplate(games=),
        SelfPlay(playout_cap=)): the Gumbel, exact and prove kernels index their records by game."""
        return root_policy == "gumbel" or exact_from is not None or bool(prove)

    def _need_reset(self):
        if self._bound is None:
            raise RuntimeError("reset() first")

    def _check_env(self, env):
        if env.num_envs != self.num_games or env.state.device != self.device:
            raise ValueError("env must hold %d boards on %s" % (self.num_games, self.device))

    @property
    def max_rollouts(self):
        """Rollouts allowed between two resets: Ntot stays below QTTT_TREE_MAX_ROLLOUTS and the playouts' step indices
        below QTTT_TREE_SELECT_BASE (value rollouts draw nothing but select's bits, addressed by the rollout index)."""
        if self.leaf_eval == "value":
            return _native.TREE_MAX_ROLLOUTS
        return min(_native.TREE_MAX_ROLLOUTS, _native.TREE_SELECT_BASE // (self.num_simulations * _native.SIM_STRIDE))

    # ------------------------------------------------------------------ the reference's interface, batched
    def reset(self, env):
        """MCTS.reset (mcts.py:139-164) of every game at env's positions (their full state, open entanglements
        included)."""
        self._check_env(env)
        self._call("qttt_tree_reset", self.tree.data_ptr(), self.num_games, self.capacity, env.state.data_ptr())
        self.rollout_idx, self.noise_idx, self._bound, self._fresh = 0, 0, 1, True
        self.gumbel_idx = 0

    def reseed(self, seed):
        """A fresh seed for every draw from here on, the draw counters (rollout, noise, Gumbel) back at 0; the trees are
        not touched.  What a search that never resets (SelfPlay.stream) does before a counter would pass its bound."""
        self.seed = int(seed)
        envs = [self.leaf] + [b["leaf"] for b in self._rounds.values()] + ([self._gumbel["root"]] if self._gumbel else [])
        envs += [b["leaf"] for b in self._subset_rounds.values()]
        for env in envs:
            env.seed = self.seed
        self.rollout_idx = self.noise_idx = self.gumbel_idx = 0

    SUBSET_CACHE = 64                 # (n_ids, k) buffer sets kept before the cache is emptied (they are views: a few tensors each)

    def subset(self, games):
        """What `games=` of contemplate() and add_root_noise() is turned into: (ids, n) with ids i32[n] on this device,
        ascending and distinct.  games: a bool or u8 mask [G] on the host (a tensor, numpy array or sequence: the list is
        made on the host and uploaded from pinned memory, nothing waits for the device) or on this device (torch.nonzero:
        one host synchronisation), or an i32 tensor of ids, ascending, distinct and in range — the caller's word is taken
        for that on the device, checked on the host — whose length is its shape's.  A result of this method passes through."""
        G, dev = self.num_games, self.device
        if isinstance(games, tuple) and len(games) == 2 and torch.is_tensor(games[0]):
            ids, n = games
            check_tensor(ids, torch.int32, (int(n),), dev, "games ids")
            return ids, int(n)
        t = games if torch.is_tensor(games) else torch.as_tensor(games)
        upload = lambda ids: (ids.contiguous().pin_memory().to(dev, non_blocking=True) if ids.numel()      # noqa: E731
                              else torch.empty(0, dtype=torch.int32, device=dev))
        if t.dtype == torch.int32:
            if t.dim() != 1 or t.numel() > G:
                raise ValueError("an id list must be a 1-d int32 tensor of at most %d entries" % G)
            if t.device.type == "cpu":
                if t.numel() and (int(t.min()) < 0 or int(t.max()) >= G or bool((t[1:] <= t[:-1]).any())):
                    raise ValueError("ids must be ascending, distinct and in 0..%d" % (G - 1))
                return upload(t), t.numel()
            return check_tensor(t, torch.int32, (t.numel(),), dev, "games ids"), t.numel()
        if t.dtype not in (torch.bool, torch.uint8) or tuple(t.shape) != (G,):
            raise ValueError("games must be a bool or uint8 mask of shape (%d,) or an int32 id tensor" % G)
        if t.device.type == "cpu":
            ids = torch.nonzero(t, as_tuple=True)[0].to(torch.int32)
            return upload(ids), ids.numel()
        if t.device != dev:
            raise ValueError("a device mask must be on %s" % (dev,))
        ids = torch.nonzero(t, as_tuple=True)[0].to(torch.int32)
        return ids, ids.numel()

    def _check_subset_search(self):
        if self.subset_refused(self.root_policy, self.exact_from, self.prove):
            raise ValueError('a subset search (games=...) is not available with root_policy="gumbel", exact_from or prove: '
                             "their kernels index their records by game, not by the subset's dense rows")
        if self.leaf_eval != "value":
            raise ValueError('a subset search (games=...) needs leaf_eval="value": its rounds are leaf-parallel rounds')

    def _subset_buffers(self, n, k):
        """The dense buffers of a subset round of n listed games and k leaves each: the n * k leaves as a VecEnv, the path
        records and the network's rows, all views of the first n * k rows of the full round's storage for k (the two
        kinds of round never overlap on a stream)."""
        b = self._subset_rounds.get((n, k))
        if b is None:
            full, rows = self._round_buffers(k), n * k
            if len(self._subset_rounds) >= self.SUBSET_CACHE:
                self._subset_rounds.clear()
            nbytes = int(self._lib.qttt_tree_paths_bytes(n, k))
            state = full["leaf"].state[:int(self._lib.qttt_state_bytes(rows))]
            b = self._subset_rounds[(n, k)] = {
                "leaf": VecEnv.from_state(state, rows, seed=self.seed, board_offset=self.board_offset),
                "paths": full["paths"][:max(nbytes, 16)],
                "out": {key: t[:rows] for key, t in full["out"].items()}}
        return b

    def contemplate(self, rollouts, games=None, forced=None):
        """`rollouts` x MCTS._rollout (mcts.py:166-176) in every game, by the one plan of search_plan(): after a reset() or
        sync() one single rollout first (K descents would all end on a root without priors), then rounds of K = leaves and
        one shorter round for what is left.  What a single and a round are is the search's form:
        leaves == 1 at the plain PUCT root: no rounds, every rollout a single; the calls are what they always were.
        eval_symmetries or exact_from: a single is a round of one leaf.
        root_policy="gumbel": after the single (the root needs its priors to be descended from) the roots are evaluated, the
        Gumbel state of the move is drawn for the budget n = the rollouts that remain, and the rounds go through the Gumbel
        select; every contemplate() is one budget of its own.
        forced_playouts: the rounds (also at K = 1) go through the forced select.
        resident=True: the rounds run inside ceil(rounds / rounds_per_launch) launches of qttt_tree_search_resident;
        rollout_idx and the node bound advance as for the launches they replace.  Not with games=.
        games (see subset()): contemplate_groups(rollouts, [(games, rollouts, forced)]).  forced= goes with games=."""
        if games is not None:
            return self.contemplate_groups(rollouts, [(games, rollouts, forced)])
        if forced is not None:
            raise ValueError("forced= goes with games=: a search of all games takes the tree's own root rule")
        self._contemplate(rollouts, [(None, rollouts, None)])

    def contemplate_groups(self, rollouts, groups):
        """groups = [(games, n, forced), ...]: every group's listed games (see subset()) are searched for n <= rollouts
        rollouts, by the same plan and with the same draws as a search of all games — the collapse bits are addressed by the
        game and by rollout_idx, and every group starts at the rollout_idx of the call — through
        qttt_tree_select_batch_subset / qttt_tree_backup_batch_subset (include/qttt_tree_subset.h): a single is a round of one
        with the plain root, the rounds are rounds of K (also at K = 1), the network launch has n_ids * K rows, and the other
        games keep every byte.  rollout_idx and the node bound then advance by `rollouts`, once, so draw indices stay a
        function of the schedule alone.  forced=False searches a group with the plain PUCT root although the tree has
        forced_playouts (None: the tree's rule).  An empty list launches nothing.  Every bound is checked before the first
        launch.  The groups' games must be disjoint: a game listed twice would be searched twice with the same draws.  That
        is the caller's word; nothing checks it on the device.  Not with root_policy="gumbel", exact_from, prove or resident."""
        if self.resident:
            raise ValueError("resident=True with contemplate(games=...): the fused launch tiles all the games, "
                             "a subset search needs the subset rounds")
        self._check_subset_search()
        self._contemplate(rollouts, [(self.subset(games), n, forced) for games, n, forced in groups])

    def _contemplate(self, rollouts, groups):
        """The bounds of `rollouts` rollouts, then every group's search (ids = subset()'s pair, None: all games) from the same
        rollout_idx, then the one place where rollout_idx and the node bound move on."""
        r, budgets = int(rollouts), [int(n) for _, n, _ in groups]
        if r < 0:
            raise ValueError("rollouts must be >= 0")
        self._need_reset()
        if self.rollout_idx + r > self.max_rollouts:
            raise ValueError("%d rollouts since reset would pass the bound of %d (draw indices)"
                             % (self.rollout_idx + r, self.max_rollouts))
        if self._bound + 2 * r > self.capacity:
            raise ValueError("%d rollouts could use %d nodes, more than capacity %d"
                             % (r, self._bound + 2 * r, self.capacity))
        if not all(0 <= n <= r for n in budgets):
            raise ValueError("a group's rollouts must be in 0..%d, the rollouts of the call" % r)
        if self.root_policy == "gumbel" and r > (1 if self._fresh else 0) and self.gumbel_idx >= _native.TREE_MAX_GUMBEL:
            raise ValueError("%d Gumbel roots since reset: the bound is %d (draw indices)"
                             % (self.gumbel_idx, _native.TREE_MAX_GUMBEL))
        idx0 = self.rollout_idx
        for (ids, _, forced), n in zip(groups, budgets):
            self.rollout_idx = idx0
            self._search(n, ids, forced)
        self.rollout_idx = idx0 + r
        self._bound += 2 * r

    def _search(self, r, ids=None, forced=None):
        """r rollouts by search_plan(), without contemplate's bounds and without the node bound: in all games, or (ids =
        subset()'s pair) in the listed ones, which leave _fresh alone: the games not listed stay fresh."""
        gumbel, K = self.root_policy == "gumbel", self.leaves
        rounds = K > 1 or self.forced_playouts is not None or gumbel or self.resident or ids is not None
        singles, sizes = search_plan(r, K, self._fresh, rounds)
        for _ in range(singles):
            if ids is not None:         # a listed root may lack priors: one plain descent
                self._round(1, ids=ids, forced=False)
            elif self.eval_symmetries is not None or self.exact_from is not None:
                self._round(1)          # no fused value rollout under these: a round of one leaf
            else:
                self._rollout()
        if ids is not None:
            fk = self.forced_playouts if forced is not False and self.forced_playouts is not None else False
            for k in sizes:
                self._round(k, ids=ids, forced=fk)
            return
        if rounds and singles:
            self._fresh = False
        if self.resident:
            return self._resident_rounds(r - singles)
        if gumbel and sizes:
            self._gumbel_begin(r - singles)
        elif gumbel and self._gumbel is not None:
            self._gumbel["n"] = 0     # no budget: no Gumbel state of this root
        for k in sizes:
            (self._gumbel_round if gumbel else self._round)(k)

    def _resident_rounds(self, r):
        """r rollouts in rounds of `leaves` (and one shorter round for what is left) inside qttt_tree_search_resident,
        without contemplate's bounds: one launch per rounds_per_launch rounds, cut at round boundaries, so the rounds and
        their draw indices are those of one launch of r."""
        per_launch = self.rounds_per_launch * self.leaves
        forced_k = -1.0 if self.forced_playouts is None else self.forced_playouts
        while r > 0:
            n = min(r, per_launch)
            self._call("qttt_tree_search_resident", self.tree.data_ptr(), self.num_games, self.capacity, self.seed,
                       self.rollout_idx, self.leaves, n, self.board_offset, self.c_puct, self.virtual_loss, forced_k,
                       self.net.blob.data_ptr(), self.net.precision)
            self.rollout_idx += n
            r -= n

    def _round_buffers(self, k):
        """The buffers of a round of k leaves per game: the G * k leaves as a VecEnv, the path records, and the rows that
        the network writes and the backup reads."""
        b = self._rounds.get(k)
        if b is None:
            n, dev = self.num_games * k, self.device
            nbytes = int(self._lib.qttt_tree_paths_bytes(self.num_games, k))
            if nbytes < 0:
                raise ValueError("qttt_tree_paths_bytes(%d, %d) failed" % (self.num_games, k))
            state = torch.zeros(int(self._lib.qttt_state_bytes(n)), dtype=torch.uint8, device=dev)
            b = self._rounds[k] = {"leaf": VecEnv.from_state(state, n, seed=self.seed, board_offset=self.board_offset),
                                   "paths": torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev),
                                   "out": out_rows(VecEnv._EVAL_ROWS, n, dev, keys=("value", "probs"))}
            if self.exact_from is not None:
                b["exact"] = torch.zeros(n, dtype=torch.uint8, device=dev)
            if self.prove:
                b["proved"] = torch.zeros(self.num_games, dtype=torch.int32, device=dev)
        return b

    def _backup_round(self, b, k, ids=()):
        """The backup of a round of k leaves whose leaves were just evaluated into b["out"]; with exact_from the eligible
        leaves are solved first (their rows of b["out"]["value"] become exact, b["exact"] says which) and the backup is
        the one that honours solved nodes; with prove the round's paths are then walked upwards (b["proved"] counts the
        nodes of every game that this round proved).  ids: a subset round's (ids, n) as pointer and count, its backup."""
        G, cap, tree = self.num_games, self.capacity, self.tree.data_ptr()
        value, probs = b["out"]["value"].data_ptr(), b["out"]["probs"].data_ptr()
        if ids:
            self._call("qttt_tree_backup_batch_subset", tree, G, cap, k, *ids, b["paths"].data_ptr(), value, probs)
        elif self.exact_from is None:
            self._call("qttt_tree_backup_batch", tree, G, cap, k, b["paths"].data_ptr(), value, probs)
        else:
            self._call("qttt_tree_solve_leaves", tree, G, cap, k, b["paths"].data_ptr(), b["leaf"].state.data_ptr(),
                       self.exact_from, value, b["exact"].data_ptr())
            self._call("qttt_tree_backup_batch_exact", tree, G, cap, k, b["paths"].data_ptr(), value, probs)
            if self.prove:
                self._call("qttt_tree_prove", tree, G, cap, k, b["paths"].data_ptr(), b["proved"].data_ptr())

    # a round's form -> (its select's entry, whether the form's own arguments stand before the paths and the leaves or after)
    _ROUND_FORMS = {"plain": ("qttt_tree_select_batch", False), "forced": ("qttt_tree_select_batch_forced", False),
                    "gumbel": ("qttt_tree_select_batch_gumbel", False), "subset": ("qttt_tree_select_batch_subset", True)}

    def _round(self, k, g=None, ids=None, forced=None):
        """One round of k rollouts (1..TREE_MAX_LEAVES) through the leaf-parallel entries, without contemplate's bounds: k
        descents per game under virtual loss, one evaluation of the leaves, their backup.  g: _gumbel_round's buffers, its
        select.  ids: subset()'s (ids, n), the round of the n listed games through the subset entries on n * k dense rows; no
        games, no launch.  forced: the root's rule; None is the tree's (forced_playouts, but never at a root that may lack
        priors: the single rollout after a reset() or sync()), False or a negative number the plain PUCT root, a number
        >= 0 that factor."""
        k = int(k)
        if not 1 <= k <= _native.TREE_MAX_LEAVES:
            raise ValueError("a round holds 1..%d leaves" % _native.TREE_MAX_LEAVES)
        if self.leaf_eval != "value":
            raise ValueError('a leaf-parallel round needs leaf_eval="value"')
        if forced is None:
            forced = False if self._fresh else self.forced_playouts
        fk = -1.0 if forced is None or forced is False else float(forced)
        if g is not None:
            form, own = "gumbel", (g["rec"].data_ptr(), g["table"].data_ptr(), g["n"], g["sim"], self.c_visit, self.c_scale)
        elif ids is not None:
            form, own = "subset", (fk, ids[0].data_ptr(), ids[1])
        else:
            form, own = ("forced", (fk,)) if fk >= 0 else ("plain", ())
        if ids is None or ids[1]:
            b = self._round_buffers(k) if ids is None else self._subset_buffers(ids[1], k)
            entry, own_first = self._ROUND_FORMS[form]
            buffers = (b["paths"].data_ptr(), b["leaf"].state.data_ptr())
            self._call(entry, self.tree.data_ptr(), self.num_games, self.capacity, self.seed, self.rollout_idx, k,
                       self.board_offset, self.c_puct, self.virtual_loss, *(own + buffers if own_first else buffers + own))
            b["leaf"].evaluate(self.net, out=b["out"], symmetries=self.eval_symmetries)
            self._backup_round(b, k, own[1:] if ids is not None else ())
        self.rollout_idx += k

    def _gumbel_buffers(self):
        g = self._gumbel
        if g is None:
            G, dev = self.num_games, self.device
            nbytes = int(self._lib.qttt_tree_gumbel_bytes(G))
            if nbytes < 0:
                raise ValueError("qttt_tree_gumbel_bytes(%d) failed" % G)
            state = torch.zeros(int(self._lib.qttt_state_bytes(G)), dtype=torch.uint8, device=dev)
            g = self._gumbel = {"root": VecEnv.from_state(state, G, seed=self.seed, board_offset=self.board_offset),
                                "rec": torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev),
                                "out": out_rows(VecEnv._EVAL_ROWS, G, dev, keys=("value", "logits")),
                                "n": 0, "sim": 0, "table": None}
        return g

    def _visit_table(self, n):
        """The visit table i32[37, n] of a budget of n simulations (qttt_gumbel_visit_sequence), on the device."""
        t = self._tables.get(n)
        if t is None:
            host = torch.empty((37, n), dtype=torch.int32)
            for m in range(37):
                _native.check(self._lib.qttt_gumbel_visit_sequence(m, n, host[m].data_ptr()), "qttt_gumbel_visit_sequence")
            t = self._tables[n] = host.to(self.device)
        return t

    def _gumbel_begin(self, n):
        """The Gumbel state of a move with a budget of n simulations, without contemplate's bounds: the roots' states,
        their evaluation (value and masked logits, over eval_symmetries), qttt_tree_gumbel_begin."""
        n = int(n)
        if self.root_policy != "gumbel" or n < 1:
            raise ValueError('a Gumbel root needs root_policy="gumbel" and a budget >= 1')
        g = self._gumbel_buffers()
        G, cap, tree = self.num_games, self.capacity, self.tree.data_ptr()
        g["table"], g["n"], g["sim"] = self._visit_table(n), n, 0
        self._call("qttt_tree_root_states", tree, G, cap, g["root"].state.data_ptr())
        g["root"].evaluate(self.net, out=g["out"], symmetries=self.eval_symmetries)
        self._call("qttt_tree_gumbel_begin", tree, G, cap, self.seed, self.gumbel_idx, self.board_offset, self.max_considered,
                   g["out"]["value"].data_ptr(), g["out"]["logits"].data_ptr(), g["rec"].data_ptr())
        self.gumbel_idx += 1

    def _gumbel_round(self, k):
        """One round of k simulations of the budget that the last _gumbel_begin opened: _round(k) with the Gumbel select."""
        k, g = int(k), self._gumbel
        if g is None or not 1 <= k <= _native.TREE_MAX_LEAVES or g["sim"] + k > g["n"]:
            raise ValueError("a Gumbel round holds 1..%d leaves within the budget of the last begin" % _native.TREE_MAX_LEAVES)
        self._round(k, g)
        g["sim"] += k

    def _gumbel_root(self, choose=None, pi=None, q_completed=None):
        self._need_reset()
        if self._gumbel is None or self._gumbel["n"] == 0:
            raise RuntimeError("contemplate() first: the Gumbel root has no state yet")
        self._call("qttt_tree_gumbel_root", self.tree.data_ptr(), self._gumbel["rec"].data_ptr(), self.num_games,
                   self.capacity, self.c_visit, self.c_scale, _ptr(choose), _ptr(pi), _ptr(q_completed))

    def _rollout(self):
        """One rollout, without contemplate's bounds: select, the playouts from the leaves, backup; or select and the
        value rollout."""
        G, cap, S, k = self.num_games, self.capacity, self.num_simulations, self.rollout_idx
        tree, leaf = self.tree.data_ptr(), self.leaf.state.data_ptr()
        step_idx0 = k * S * _native.SIM_STRIDE
        self._call("qttt_tree_select", tree, G, cap, self.seed, k, self.board_offset, self.c_puct, leaf)
        if self.leaf_eval == "value":
            self._call("qttt_tree_value_rollout", tree, G, cap, leaf, self.net.blob.data_ptr(), self.net.precision,
                       None, None)
        elif self.net is None:
            self.leaf.rollout_many(S, step_idx0=step_idx0, out=self._out)
            self._call("qttt_tree_backup", tree, G, cap, self._out.data_ptr(), S, None)
        else:
            self.leaf.rollout_policy(self.net, S, step_idx0=step_idx0, out=self._out)
            self._call("qttt_tree_backup", tree, G, cap, self._out["result"].data_ptr(), S,
                       self._out["probs"].data_ptr())
        self.rollout_idx = k + 1

    def add_root_noise(self, epsilon=0.25, alpha=0.3, noise=None, applied=None, games=None):
        """P <- (1 - epsilon) P + epsilon Dirichlet(alpha) at every root that has priors, is not terminal and has a
        legal action (qttt_tree_root_noise); a root that has no priors yet is left alone, so run one rollout first.
        The draws are addressed by (seed, board_offset + g, noise_idx), and noise_idx counts these calls since reset():
        a call never repeats an earlier one's noise, and a second call on the same root mixes again.  noise f64[G, 36]
        and applied u8[G], both optional, receive the normalised noise and whether the game was noised.
        games (see subset()): only the listed games are noised (qttt_tree_root_noise_subset), each with exactly the noise
        that the full call would give it; the other games keep every byte, and their rows of noise and applied keep what
        they held.  The call counts as one noise call either way."""
        eps, alpha = float(epsilon), float(alpha)
        if not 0.0 <= eps <= 1.0:
            raise ValueError("epsilon must be in [0, 1]")
        if not 0.0 < alpha < float("inf"):
            raise ValueError("alpha must be positive and finite")
        self._need_reset()
        if self.noise_idx >= _native.TREE_MAX_NOISE:
            raise ValueError("%d noise calls since reset: the bound is %d (draw indices)"
                             % (self.noise_idx, _native.TREE_MAX_NOISE))
        G, dev = self.num_games, self.device
        if noise is not None:
            check_tensor(noise, torch.float64, (G, 36), dev, "noise")
        if applied is not None:
            check_tensor(applied, torch.uint8, (G,), dev, "applied")
        if games is None:
            self._call("qttt_tree_root_noise", self.tree.data_ptr(), G, self.capacity, self.seed, self.noise_idx,
                       self.board_offset, eps, alpha, _ptr(noise), _ptr(applied))
        else:
            ids, n = self.subset(games)
            if n:
                self._call("qttt_tree_root_noise_subset", self.tree.data_ptr(), G, self.capacity, self.seed, self.noise_idx,
                           self.board_offset, eps, alpha, ids.data_ptr(), n, _ptr(noise), _ptr(applied))
        self.noise_idx += 1

    def root_stats(self):
        """The roots' statistics: N i32[G,36], W / Q / P f64[G,36], Ntot i32[G], choose u8[G], nodes_used i32[G],
        overflow bool[G].  root_policy="gumbel": choose is the Gumbel choice, and pi f64[G,36] (the improved policy) and
        q_completed f64[G,36] are there too.  forced_playouts: forced bool[G,36] (the predicate of
        include/qttt_tree_forced.h as the roots stand) and n_pruned i32[G,36] (the visits that the pruned policy target
        keeps), one qttt_tree_root_forced launch.  prove=True: proven bool[G,36] (the action's children are all terminal or
        solved), q_exact f32[G,36] (its exact q, NaN where it is not proven), root_solved bool[G] and root_value_exact
        f32[G] (NaN where the root is not solved), one qttt_tree_root_exact launch."""
        o = out_rows(self._ROOT_ROWS, self.num_games, self.device)
        self._root(**o)
        o["overflow"] = o["overflow"].bool()
        if self.prove:
            o.update(self._root_exact())
        if self.root_policy == "gumbel":
            o.update(out_rows(self._GUMBEL_ROWS, self.num_games, self.device))
            self._gumbel_root(o["choose"], o["pi"], o["q_completed"])
        if self.forced_playouts is not None:
            f = out_rows(self._FORCED_ROWS, self.num_games, self.device)
            self._call("qttt_tree_root_forced", self.tree.data_ptr(), self.num_games, self.capacity, self.forced_playouts,
                       self.c_puct, f["forced"].data_ptr(), f["n_pruned"].data_ptr())
            f["forced"] = f["forced"].bool()
            o.update(f)
        return o

    def _root(self, N=None, W=None, Q=None, P=None, Ntot=None, choose=None, nodes_used=None, overflow=None):
        self._need_reset()
        self._call("qttt_tree_root", self.tree.data_ptr(), self.num_games, self.capacity, _ptr(N), _ptr(W), _ptr(Q),
                   _ptr(P), _ptr(Ntot), _ptr(choose), _ptr(nodes_used), _ptr(overflow))

    def _root_exact(self):
        """What the proofs say of the roots (qttt_tree_root_exact): proven, q_exact, root_solved, root_value_exact."""
        self._need_reset()
        e = out_rows(self._EXACT_ROWS, self.num_games, self.device)
        self._call("qttt_tree_root_exact", self.tree.data_ptr(), self.num_games, self.capacity, e["q_exact"].data_ptr(),
                   e["proven"].data_ptr(), e["root_value_exact"].data_ptr(), e["root_solved"].data_ptr())
        e["proven"], e["root_solved"] = e["proven"].bool(), e["root_solved"].bool()
        return e

    def choose(self, exact=False):
        """MCTS.choose (mcts.py:308-315) per game: action36 u8[G], 255 where the root has no legal action.
        exact=True (needs prove=True): a game whose root is solved plays the lowest action that attains the maximal
        q_exact, the solver's best move (where a root was solved as a leaf and not all its actions are proven yet: the
        lowest proven action whose q_exact is the root's value, if there is one); every other game its ordinary choice.  Composed on the device, no host
        synchronisation."""
        if exact and not self.prove:
            raise ValueError("choose(exact=True) needs prove=True")
        a = out_tensor(*self._ROOT_ROWS["choose"], self.num_games, self.device)
        if self.root_policy == "gumbel":      # the best survivor of the halving (255 also at a terminal root)
            self._gumbel_root(choose=a)
        else:
            self._root(choose=a)
        if not exact:
            return a
        e = self._root_exact()
        # a proven action whose q is the root's value is optimal; at a root that a round proved every legal action is
        # proven and the maximal q_exact is that value.  (A root that was solved as a leaf may have none: its own choice.)
        best = e["proven"] & (e["q_exact"] == e["root_value_exact"][:, None])          # NaN compares unequal
        first = best.to(torch.uint8).argmax(1).to(torch.uint8)                         # the lowest action among them
        return torch.where(best.any(1), first, a)

    def solved_count(self):
        """i64[G], on the device: the nodes of every game (below its `used`) that carry the solved flag of
        include/qttt_tree_exact.h; zeros without exact_from.  Torch on the tree buffer, for tests and reports."""
        self._need_reset()
        G, cap = self.num_games, self.capacity
        gb, nb = _native.TREE_GAME_BYTES, _native.TREE_NODE_BYTES
        used = self.tree[:G * gb].view(G, gb)[:, :4].contiguous().view(torch.int32).view(G)
        flags = self.tree[G * gb:G * gb + G * cap * nb].view(G, cap, nb)[:, :, 28:32].contiguous().view(torch.int32).view(G, cap)
        live = torch.arange(cap, device=self.device)[None, :] < used[:, None]
        return (((flags & _native.TREE_NODE_SOLVED) != 0) & live).sum(1)

    def nodes_used(self):
        n = out_tensor(*self._ROOT_ROWS["nodes_used"], self.num_games, self.device)
        self._root(nodes_used=n)
        return n

    def sync(self, env):
        """MCTS.sync (mcts.py:317-337) after a move: every game re-roots onto the child equal to env's position
        (keeping its statistics), or onto a fresh root when that child was never expanded; a game whose position did
        not change keeps its root."""
        self._check_env(env)
        self._need_reset()
        if self._bound + 1 > self.capacity:
            raise ValueError("a sync could use %d nodes, more than capacity %d" % (self._bound + 1, self.capacity))
        self._call("qttt_tree_sync", self.tree.data_ptr(), self.num_games, self.capacity, env.state.data_ptr())
        self._bound += 1
        self._fresh = True
        if self._gumbel is not None:
            self._gumbel["n"] = 0     # the Gumbel state belonged to the root that was left

    def compact(self, update_bound=True):
        """MCTS._prune as sync does it (mcts.py:222-231, 330-337): every game keeps the nodes reachable from its root,
        in their old order with the root at index 0, and gives the rest back.  The search goes on bit for bit as if
        nothing had been compacted: rollout_idx is not reset, the draws go on.  update_bound=True reads nodes_used
        back and makes its maximum the host's bound, which is what lets contemplate() accept the next move's rollouts
        in a small `capacity`: one host read-back (a device synchronisation) per call, so call it once per move,
        never per rollout.  update_bound=False reads nothing back; the old bound stays, still valid."""
        self._need_reset()
        if self._scratch is None:
            nbytes = int(self._lib.qttt_tree_compact_bytes(self.num_games, self.capacity))
            if nbytes < 0:
                raise ValueError("qttt_tree_compact_bytes(%d, %d) failed" % (self.num_games, self.capacity))
            self._scratch = torch.empty(max(nbytes // 4, 1), dtype=torch.int32, device=self.device)
        self._call("qttt_tree_compact", self.tree.data_ptr(), self.num_games, self.capacity, self._scratch.data_ptr())
        if update_bound:
            self._bound = int(self.nodes_used().max()) if self.num_games else 1

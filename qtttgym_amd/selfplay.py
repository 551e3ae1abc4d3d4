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
§14): one launch turns the batch of G games into the batch of 8 G games it stands for.
"""
import ctypes

import torch

from . import _native
from ._host import LibCaller, _raw_stream, check_net, check_tensor, resolve_device
from .symmetry import check_symmetries
from .tree import TreeSearch
from .vec_env import VecEnv

ROWS = _native.SELFPLAY_ROWS


class SelfPlayBatch:
    """One play()'s samples as the kernel wrote them, row t = the t-th root of every game (rows at or past a game's
    `length` are zero): states u8[10, qttt_state_bytes(G)], pi f64[10, G, 36], mask u8[10, G, 36], done u8[10, G],
    v f32[10, G], action36 u8[10, G] (the move played from the row, 255 in the terminal row), length u8[G] (rows of
    the game, its terminal row included), winner i8[G] (1 / 0 / -1 = True / False / None) and actions u8[G, 2], the
    last ply's move."""

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
    noise is the exploration."""

    def __init__(self, num_games, n_rollouts=100, num_simulations=10, net=None, alpha=1.0, c_puct=1.0,
                 value_targets=(1.0, 0.0), seed=0, compact=False, carry=None, device=None, leaf_eval="playouts",
                 root_noise=None, temperature=1.0, sample_plies=0, leaves=1, virtual_loss=1.0,
                 eval_symmetries=None, root_policy="puct", max_considered=16, c_visit=50.0, c_scale=1.0):
        self.leaves, self.virtual_loss = TreeSearch.check_search_args(leaf_eval, net, leaves, virtual_loss)
        self.root_policy, self.max_considered, self.c_visit, self.c_scale = TreeSearch.check_root_args(
            leaf_eval, net, root_policy, max_considered, c_visit, c_scale)
        self.eval_symmetries = TreeSearch.check_eval_symmetries(leaf_eval, eval_symmetries)
        self.leaf_eval = leaf_eval
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
        self.env = self.tree = None   # the last play()'s environment (at the final positions) and trees

    def new_batch(self):
        """A zero-filled SelfPlayBatch for num_games games."""
        return SelfPlayBatch(self.num_games, self.device, self._lib.qttt_state_bytes(self.num_games))

    def record(self, tree, ply, batch):
        """One qttt_selfplay_record: the roots of `tree` become row `ply` of `batch`; returns batch.actions, the move
        to step with.  With sample_plies > 0 it is qttt_selfplay_record_sampled, drawing with the tree's seed and
        board_offset."""
        G, dev = self.num_games, self.device
        if tree.num_games != G or tree.device != dev or batch.num_games != G:
            raise ValueError("tree and batch must hold %d games on %s" % (G, dev))
        check_tensor(batch.states, torch.uint8, (ROWS, int(self._lib.qttt_state_bytes(G))), dev, "batch.states")
        for k, (dt, shp) in SelfPlayBatch._ROWS.items():
            check_tensor(getattr(batch, k), dt, (ROWS, G) + shp, dev, "batch." + k)
        check_tensor(batch.length, torch.uint8, (G,), dev, "batch.length")
        check_tensor(batch.winner, torch.int8, (G,), dev, "batch.winner")
        check_tensor(batch.actions, torch.uint8, (G, 2), dev, "batch.actions")
        args = (tree.tree.data_ptr(), G, tree.capacity, int(ply), self.n_rollouts, self.alpha, self.v_first, self.v_second,
                batch.states.data_ptr(), batch.pi.data_ptr(), batch.mask.data_ptr(), batch.done.data_ptr(),
                batch.v.data_ptr(), batch.action36.data_ptr(), batch.length.data_ptr(), batch.winner.data_ptr(),
                batch.actions.data_ptr())
        if self.root_policy == "gumbel":
            if tree.root_policy != "gumbel" or tree._gumbel is None:
                raise ValueError("the Gumbel record needs a tree searched with root_policy=\"gumbel\"")
            self._call("qttt_selfplay_record_gumbel", *args, tree._gumbel["rec"].data_ptr(), tree.c_visit, tree.c_scale)
        elif self.sample_plies > 0:
            self._call("qttt_selfplay_record_sampled", *args, tree.seed, tree.board_offset, self.temperature,
                       self.sample_plies)
        else:
            self._call("qttt_selfplay_record", *args)
        return batch.actions

    def play(self, seed=None):
        """play_game (self_play.py:43-76) of num_games games from the empty board and their samples
        (self_play.py:193-216) as a SelfPlayBatch.  seed=None: self.seed + the number of earlier play() calls.  The
        environment draws its collapse bits with `seed`, the trees their playouts with 2 * seed + 1.  A finished game
        rides along: its moves are noops, its tree keeps its root."""
        s = self.seed + self.plays if seed is None else int(seed)
        self.plays += 1
        G, R = self.num_games, self.n_rollouts
        env = self.env = VecEnv(G, device=self.device, seed=s)
        tree = self.tree = TreeSearch(G, capacity=self.capacity, num_simulations=self.num_simulations,
                                      c_puct=self.c_puct, net=self.net, seed=2 * s + 1, device=self.device,
                                      leaf_eval=self.leaf_eval, leaves=self.leaves, virtual_loss=self.virtual_loss,
                                      eval_symmetries=self.eval_symmetries, root_policy=self.root_policy,
                                      max_considered=self.max_considered, c_visit=self.c_visit, c_scale=self.c_scale)
        tree.reset(env)
        batch = self.new_batch()
        for ply in range(ROWS):
            if ply < ROWS - 1:                  # at ply 9 every game is over: nine moves fill the board
                if self.root_noise is None:
                    tree.contemplate(R)
                else:                           # the same R rollouts, the noise after the one that gives the priors
                    tree.contemplate(1)
                    tree.add_root_noise(*self.root_noise)
                    tree.contemplate(R - 1)
            env.step_raw(self.record(tree, ply, batch))
            tree.sync(env)
            if self.compact:
                tree.compact()
        return batch

"""Reanalyser — MuZero-style reanalysis of the replay ring (Schrittwieser et al.; include/qttt_replay_reanalyse.h,
DESIGN.md §27): positions are taken out of a ReplayBuffer, searched again with the network as it is now, and their
targets overwritten in place, so that a window of many network generations does not train on policies of networks that
no longer exist.

    sp = SelfPlay(4096, n_rollouts=32, net=net, leaf_eval="value")
    ra = Reanalyser(sp, ring, 4096)
    ring.add(sp.play()); ra.run()                         # no host synchronisation in either

One run() is a gather, one searched ply of n trees, a record, and a guarded update: a sample that stream() or add() has
appended over in between, and a terminal row, keep what they hold.
"""
import torch

from ._host import LibCaller
from .replay import ReplayBuffer
from .selfplay import SelfPlay
from .tree import TreeSearch
from .vec_env import VecEnv


class ReanalyseStats:
    """What Reanalyser.run() returns, device tensors that nothing here reads back: updated bool[n] (the sample's targets
    were written), slot i32[n] (-1: the window was longer than the ring holds), and exact bool[n] (the sample was
    relabelled with its exact targets) where the SelfPlay has exact_targets, else None."""

    def __init__(self, updated, slot, exact):
        self.updated, self.slot, self.exact = updated, slot, exact


class Reanalyser(LibCaller):
    """Re-searches n positions of `ring` per run() with the search settings of the SelfPlay `sp` — net, n_rollouts,
    leaf_eval, leaves, eval_symmetries, root_policy, exact_from, prove, forced_playouts / prune_targets, alpha, c_puct,
    exact_targets / exact_policy; its
    root_noise and sample_plies are ignored, a reanalysis plays no move — and writes the new policy targets into their
    slots (ReplayBuffer.gather / update).  The policy target is the record kernels' own: the visit-count target, or the
    improved policy under root_policy="gumbel".
    value_mix = lambda in [0, 1]: with 0 the stored v, the game's outcome, stays.  Otherwise
    v = (1 - lambda) * v_stored + lambda * v_search with v_search = sum_a N[a] Q[a] / sum_a N[a] over the root's actions
    (the mover's value; a root without a visit keeps v_stored), computed in f64 and stored as f32.  With sp.exact_targets
    = M the samples with at least M moves played get their exact pi (sp.exact_policy) and v whatever lambda is.  Both need
    sp's value_targets = (1.0, -1.0): the stored v must be the mover's on [-1, 1] to be mixed with either.
    The trees of run number k draw with a seed of their own, tree_seed(k)."""

    def __init__(self, sp, ring, n, value_mix=0.0, seed=0):
        if not isinstance(sp, SelfPlay):
            raise ValueError("sp must be a SelfPlay")
        if not isinstance(ring, ReplayBuffer) or ring.device != sp.device:
            raise ValueError("ring must be a ReplayBuffer on %s" % (sp.device,))
        self.n, self.value_mix, self.seed = int(n), float(value_mix), int(seed)
        if self.n < 1:
            raise ValueError("n must be >= 1")
        if not 0.0 <= self.value_mix <= 1.0:
            raise ValueError("value_mix must be in [0, 1]")
        if self.value_mix > 0.0 and (sp.v_first, sp.v_second) != (1.0, -1.0):
            raise ValueError("value_mix > 0 needs value_targets=(1.0, -1.0): the searched value is the mover's, in [-1, 1], "
                             "and the reference's (1, 0) is not zero-sum, so the mixed v would be on two scales")
        self._open(sp.device)
        self.sp, self.ring = sp, ring
        # the recorder: sp's settings for n games, without the exploration a reanalysis has no move for
        self.recorder = SelfPlay(self.n, n_rollouts=sp.n_rollouts, alpha=sp.alpha, value_targets=(sp.v_first, sp.v_second),
                                 seed=self.seed, device=sp.device, exact_targets=sp.exact_targets,
                                 exact_policy=sp.exact_policy, prune_targets=sp.prune_targets, **sp.search_kwargs())
        self.env =VecEnv(self.n, device=self.device)
        self.tree = self.new_tree(self.tree_seed(0))
        self.batch = self.recorder.new_batch()
        self.runs = 0                   # run() calls so far: what the next run's trees are seeded with

    def tree_seed(self, k):
        """The seed of the trees of run number k."""
        return (2 * (self.seed + int(k)) + 1) & (2 ** 64 - 1)

    def new_tree(self, seed):
        """A TreeSearch of n games with the SelfPlay's search settings and the nodes of one searched ply: the root, two
        per rollout, one to spare (SelfPlay's 2 * n_rollouts + 1 per ply, and the root)."""
        sp = self.recorder
        return TreeSearch(self.n, capacity=2 * sp.n_rollouts + 2, seed=seed, device=self.device, **sp.search_kwargs())

    def run(self, start=None):
        """One reanalysis of n positions, without a host synchronisation: gather a window (start: ReplayBuffer.gather's) ->
        search it with the network's weights as they are now -> record the roots as row 0 of the staging batch [->
        exact targets] -> compose v where it is wanted -> guarded update.  Returns ReanalyseStats."""
        sp, tree, batch = self.recorder, self.tree, self.batch
        window = self.ring.gather(self.n, start, env=self.env)
        tree.reseed(self.tree_seed(self.runs))
        tree.reset(self.env)
        self.runs += 1
        tree.contemplate(sp.n_rollouts)
        batch.length.zero_()
        batch.done.zero_()
        sp.record(tree, 0, batch)
        exact = None
        if sp.exact_targets is not None:
            exact = batch.exact_targets(sp.exact_targets, sp.exact_policy)[0].bool()
        v_new = None
        if self.value_mix > 0.0:
            st = tree.root_stats()
            N = st["N"].double()
            total = N.sum(1)
            searched = torch.where(N > 0, N * st["Q"], torch.zeros_like(N)).sum(1) / total.clamp(min=1.0)
            mixed = (1.0 - self.value_mix) * window.v.double() + self.value_mix * searched
            v_new = torch.where(total > 0, mixed, window.v.double()).float()
        if exact is not None:
            v_new = torch.where(exact, batch.v[0], window.v if v_new is None else v_new)
        updated = self.ring.update(window, pi=batch.pi[0], v=v_new)
        return ReanalyseStats(updated, window.slot, exact)

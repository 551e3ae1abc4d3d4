#!/usr/bin/env python3
"""The reference's strat_eval.eval_strats (strat_eval.py:34-95) batched over G games, with real search trees on the
device (qtttgym_amd.TreeSearch).  Player 1 moves first in the first half of the games and second in the other half.
Each side keeps its own tree per half, contemplates `rollouts` times before each of its moves, chooses, and every tree
syncs after every move (strat_eval.play_game).  Finished games are frozen: their later moves are noops.

    python examples/tree_tournament.py --p1 az:300 --p2 mcts:3000 [--games 1024] [--sims 10] [--dtype f32|bf16]
                                       [--weights tests/golden/model_eval.npz | --model model.pt]
                                       [--compact [--carry N]] [--leaves K [--p2-leaves K2]]
                                       [--eval-symmetries all|0,4]

A player is mcts:R (uniform playouts and priors, MCTS(R)), az:R (the network's playouts and priors, AlphaZero(R)),
azv:R (the network's value head at the leaf and its priors, TreeSearch(leaf_eval="value"): no playouts), azg:R (azv with
the Gumbel root, TreeSearch(root_policy="gumbel", max_considered=--max-considered): R of 16-32 is its range) or random (the
uniform-legal policy).  --leaves K gives the azv players K leaves per game per round (TreeSearch(leaves=K), virtual
loss; --p2-leaves K2 when player 2's differs: azv:304 --leaves 8 --p2-leaves 1 plays the leaf-parallel search against
the plain one).  --eval-symmetries all (or a list of 1, 2, 4 or 8 symmetries such as 0,4) gives the azv players the
network's outputs averaged over every leaf's images (TreeSearch(eval_symmetries=...)).  Prints player 1's win, loss and draw counts and rates.

--compact: every tree gives the nodes outside its new root's subtree back after each sync (TreeSearch.compact, the
reference's _prune), so its pool holds 2 * R + carry nodes instead of every node of the game.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from qtttgym_amd import PolicyValueNet, TreeSearch, VecEnv  # noqa: E402
from qtttgym_amd import recommended_env  # noqa: E402
from qtttgym_amd.actions import action36_to_pairs  # noqa: E402
from qtttgym_amd.policy_value import SHAPES  # noqa: E402
recommended_env(apply=True)


def parse_player(spec):
    kind, _, n = spec.partition(":")
    if kind == "random":
        return ("random", 0)
    if kind not in ("mcts", "az", "azv", "azg") or not n.isdigit() or int(n) < 1:
        raise SystemExit("a player is mcts:R, az:R, azv:R, azg:R or random, not %r" % spec)
    return (kind, int(n))


def load_state_dict(args):
    if args.model:
        return torch.load(args.model, map_location="cpu")
    with np.load(args.weights) as d:
        return {k: torch.from_numpy(d[k.replace(".", "_")]) for k in SHAPES}


VALUE_KINDS = ("azv", "azg")           # the players that score a leaf by the value head


def play(players, G, sims, net, seed, carry=None, leaves=(1, 1), eval_symmetries=None, max_considered=16, exact_from=None,
         prove=False, forced_playouts=None, resident=False):
    """One half: players[0] moves first; leaves[i] = the leaves per round of players[i] when it is an azv player, and
    eval_symmetries what the azv players average the network over.  Returns winner i8[G] (1 = the first mover, 0 = the second, -1 = none).
    carry: None = the trees never compact; else they compact after every sync and hold 2 * R + carry nodes (carry < 0:
    2 * R + 2 of them).  exact_from: the azv and azg players solve leaves with that many moves played exactly; prove: they
    prove interior nodes as well (the played move stays the search's own choice).  forced_playouts: the azv players search
    with forced playouts at the root (TreeSearch(forced_playouts=k)); resident: the azv players that use neither exact leaves
    nor symmetry-averaged ones run their rounds inside the fused launch (TreeSearch(resident=True))."""
    env = VecEnv(G, seed=seed)
    trees = []
    for i, (kind, R) in enumerate(players):
        if kind == "random":
            trees.append(None)
            continue
        own_moves = 5 if i == 0 else 4
        capacity = 1 + 2 * R * own_moves + 9 if carry is None else 2 * R + (carry if carry >= 0 else 2 * R + 2)
        value = kind in VALUE_KINDS
        t = TreeSearch(G, capacity=capacity, num_simulations=sims, net=net if kind == "az" or value else None,
                       seed=seed * 2 + 1 + i, device=env.device, leaf_eval="value" if value else "playouts",
                       leaves=leaves[i] if value else 1, eval_symmetries=eval_symmetries if value else None,
                       root_policy="gumbel" if kind == "azg" else "puct", max_considered=max_considered,
                       exact_from=exact_from if value else None, prove=prove and value and exact_from is not None,
                       forced_playouts=forced_playouts if kind == "azv" else None,
                       resident=resident and kind == "azv" and exact_from is None and eval_symmetries is None)
        t.reset(env)
        trees.append(t)
    finished = torch.zeros(G, dtype=torch.bool, device=env.device)
    for ply in range(9):
        mover = ply % 2
        kind, R = players[mover]
        if trees[mover] is None:
            actions = env.sample_actions()
        else:
            trees[mover].contemplate(R)
            actions = action36_to_pairs(trees[mover].choose())
        actions = torch.where(finished[:, None], torch.full_like(actions, 255), actions).contiguous()
        _, term = env.step_raw(actions)
        finished |= term
        for t in trees:
            if t is not None:
                t.sync(env)
                if carry is not None:
                    t.compact()
    return env.node_info(python_key=False)["winner"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p1", default="az:300")
    ap.add_argument("--p2", default="mcts:3000")
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--model", default=None, help="state dict with nn.Model's keys (torch.load)")
    ap.add_argument("--weights", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                      "tests", "golden", "model_eval.npz"))
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--compact", action="store_true",
                    help="compact every tree after each sync; its capacity is then 2 * R + carry")
    ap.add_argument("--carry", type=int, default=None,
                    help="with --compact: room for the subtree a tree carries into its next move, beside the 2 * R "
                         "nodes that move's rollouts can add.  Default 2 * R + 2 (R = the tree's own rollouts): what "
                         "one move's rollouts and the two syncs until the next can allocate.  A kept subtree is "
                         "measured at a small fraction of that (DESIGN.md section 12), so a smaller carry usually "
                         "does; one that turns out too small raises ValueError before any node is lost")
    ap.add_argument("--leaves", type=int, default=1,
                    help="leaves per game per round of the azv players (TreeSearch(leaves=K): virtual loss)")
    ap.add_argument("--p2-leaves", type=int, default=None, help="player 2's, when it differs (default: --leaves)")
    ap.add_argument("--eval-symmetries", default=None, metavar="all|K,K,...",
                    help="the azv players average the network over these symmetries of every leaf")
    ap.add_argument("--max-considered", type=int, default=16, help="actions the azg players' Gumbel root samples (1..36)")
    ap.add_argument("--exact-from", type=int, default=None, metavar="M",
                    help="the azv and azg players solve leaves with at least M (6..9) moves played exactly on the device "
                         "(TreeSearch(exact_from=M))")
    ap.add_argument("--prove", action="store_true",
                    help="with --exact-from: those players prove interior nodes too (TreeSearch(prove=True))")
    ap.add_argument("--forced-playouts", type=float, default=None, metavar="K",
                    help="the azv players force root actions with n * n < K * P * sum(n) (TreeSearch(forced_playouts=K), "
                         "include/qttt_tree_forced.h)")
    ap.add_argument("--resident", action="store_true",
                    help="the azv players search with the resident search (TreeSearch(resident=True), "
                         "include/qttt_tree_resident.h): the same games, one fused launch for a move's rounds")
    args = ap.parse_args()
    if args.prove and args.exact_from is None:
        raise SystemExit("--prove needs --exact-from")
    syms = args.eval_symmetries
    syms = syms if syms in (None, "all") else tuple(int(k) for k in syms.split(","))
    p1, p2 = parse_player(args.p1), parse_player(args.p2)
    k1, k2 = args.leaves, args.leaves if args.p2_leaves is None else args.p2_leaves
    half = args.games // 2
    if half < 1:
        raise SystemExit("--games must be at least 2")
    net = None
    if {"az", "azv", "azg"} & {p1[0], p2[0]}:
        net = PolicyValueNet(load_state_dict(args), device="cuda",
                             dtype=torch.float32 if args.dtype == "f32" else torch.bfloat16)
    if args.carry is not None and not args.compact:
        raise SystemExit("--carry needs --compact")
    carry = None
    if args.compact:
        if args.carry is not None and args.carry < 0:
            raise SystemExit("--carry must be >= 0")
        carry = args.carry if args.carry is not None else -1
    w_a = play((p1, p2), half, args.sims, net, args.seed, carry, (k1, k2), syms, args.max_considered,
               args.exact_from, args.prove, args.forced_playouts, args.resident)                                        # player 1 moves first
    w_b = play((p2, p1), half, args.sims, net, args.seed + 1, carry, (k2, k1), syms, args.max_considered,
               args.exact_from, args.prove, args.forced_playouts, args.resident)                                        # player 2 moves first
    wins = int((w_a == 1).sum()) + int((w_b == 0).sum())
    losses = int((w_a == 0).sum()) + int((w_b == 1).sum())
    draws = int((w_a == -1).sum()) + int((w_b == -1).sum())
    n = 2 * half
    first = int((w_a == 1).sum())
    print("%s vs %s, %d games, %d simulations: wins %d, losses %d, draws %d; rates %.3f, %.3f, %.3f; "
          "moving first %d of %d wins (%.3f)"
          % (args.p1, args.p2, n, args.sims, wins, losses, draws, wins / n, losses / n, draws / n, first, half,
             first / half))
    return wins, losses, draws


if __name__ == "__main__":
    main()

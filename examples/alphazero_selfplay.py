#!/usr/bin/env python3
"""The reference's AlphaZero._rollout (alphazero.py:173-180) batched over G games: the simulations below a leaf are the
NETWORK's playouts (AlphaZero._simulate, :192-205), not uniform ones.  Each search iteration, for all G games at once:

  1. select an action at the root by PUCT on the network's priors, Q + c_puct * P * sqrt(Ntot) / (1 + N) (:287-292);
  2. expand it (`VecEnv.expand`, MCTS._step's one or two collapse children);
  3. run n_sims network playouts from each child in ONE launch per child (`VecEnv.rollout_policy(net, n_sims,
     leaf=("probs",))`): every ply evaluates the network, samples from Categorical(logits) and steps; the leaf's probs
     are the child's priors, node.P, kept for a later visit of that child;
  4. back up the mean over the children that exist of `r if leaf.turn else -r` (:177), weighted as
     az_puct_selfplay.py weights the two collapse branches.

    python examples/alphazero_selfplay.py [--weights tests/golden/model_eval.npz | --model model.pt]
                                          [--games 1024] [--iters 48] [--sims 4] [--dtype f32|bf16]

Player 1 (X) searches, player 2 (O) plays the uniform-legal random policy; prints P1's score.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from qtttgym_amd import PolicyValueNet, VecEnv  # noqa: E402
from qtttgym_amd.policy_value import SHAPES  # noqa: E402
from qtttgym_amd import recommended_env  # noqa: E402
recommended_env(apply=True)   # HIP_FORCE_DEV_KERNARG=1 etc., before the first HIP call
from qtttgym_amd.actions import action36_to_pairs  # noqa: E402


def load_state_dict(args):
    if args.model:
        return torch.load(args.model, map_location="cpu")
    with np.load(args.weights) as d:
        return {k: torch.from_numpy(d[k.replace(".", "_")]) for k in SHAPES}


def search_actions(env, net, iters, sims, ply, c_puct=1.0):
    G, dev = env.num_envs, env.device
    legal = env.node_info(python_key=False)["legal"]                                  # bit a = action a legal (mcts.py:20-27)
    mask = (legal[:, None] >> torch.arange(36, device=dev)[None, :]) & 1 == 1          # [G, 36]
    P = torch.nan_to_num(env.evaluate(net, rows=("probs",))["probs"], nan=0.0)          # the root's priors
    N = torch.zeros((G, 36), device=dev)
    W = torch.zeros((G, 36), device=dev)
    child_P = torch.zeros((G, 36, 2, 36), device=dev)                                   # node.P of each expanded child
    leaf_sign = 1.0 if ply % 2 == 1 else -1.0          # leaf.turn: the child's mover is P1 after an odd ply
    rows = torch.arange(G, device=dev)
    work = VecEnv.from_state(env.state, G, seed=env.seed + 7919 * (ply + 1), board_offset=env.board_offset)
    exp_out, roll = None, [None, None]
    for it in range(iters):
        Q = W / N.clamp(min=1)
        U = c_puct * P * torch.sqrt(N.sum(1, keepdim=True) + 1.0) / (1.0 + N)            # alphazero.py:289-291
        a = torch.where(mask, Q + U, torch.full_like(Q, -math.inf)).argmax(1)
        exp_out = work.expand(a.to(torch.uint8), out=exp_out, python_key=False)
        nch = exp_out["n_children"].to(torch.float32)
        v_leaf = torch.zeros(G, device=dev)
        for c in range(2):
            child = exp_out["child%d" % c]
            child.seed = work.seed
            roll[c] = child.rollout_policy(net, n_sims=sims, step_idx0=32 * sims * it + 16 * sims * c,
                                           leaf=("probs",), out=roll[c])
            r = roll[c]["result"].to(torch.float32).mean(1)
            exists = nch > c
            v_leaf += torch.where(exists, leaf_sign * r, torch.zeros_like(r))            # r if leaf.turn else -r
            child_P[rows, a, c] = torch.where(exists[:, None], torch.nan_to_num(roll[c]["probs"], nan=0.0),
                                              child_P[rows, a, c])
        v = -v_leaf / nch.clamp(min=1)                     # the value for the root's mover (_backpropogate's r = -r)
        N.scatter_add_(1, a[:, None], torch.ones((G, 1), device=dev))
        W.scatter_add_(1, a[:, None], v[:, None])
    return torch.where(mask, N, torch.full_like(N, -1.0)).argmax(1)                    # the most visited action


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=48)
    ap.add_argument("--sims", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--model", default=None, help="state dict with nn.Model's keys (torch.load)")
    ap.add_argument("--weights", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                      "tests", "golden", "model_eval.npz"))
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    args = ap.parse_args()
    G = args.games
    env = VecEnv(G, seed=args.seed)
    net = PolicyValueNet(load_state_dict(args), device=env.device,
                         dtype=torch.float32 if args.dtype == "f32" else torch.bfloat16)
    finished = torch.zeros(G, dtype=torch.bool, device=env.device)
    for ply in range(9):
        if ply % 2 == 0:
            actions = action36_to_pairs(search_actions(env, net, args.iters, args.sims, ply))
        else:
            actions = env.sample_actions()
        actions = torch.where(finished[:, None], torch.full_like(actions, 255), actions)   # freeze finished games
        _, term = env.step_raw(actions.contiguous())
        finished |= term
    w = env.node_info(python_key=False)["winner"]
    p1, p2, none = int((w == 1).sum()), int((w == 0).sum()), int((w == -1).sum())
    print("games %d  iterations %d x %d network playouts per child :  P1 (AlphaZero rollouts) wins %d (%.1f %%), "
          "P2 (random) wins %d, no winner %d" % (G, args.iters, args.sims, p1, 100.0 * p1 / G, p2, none))
    return p1 / G


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ucb_selfplay.py's root-level PUCT search with the NETWORK's priors: before each search the policy/value network
(the reference's nn.py, `PolicyValueNet`) gives P for the root of every game in ONE kernel (`VecEnv.evaluate(net,
rows=("probs",))`, where alphazero.py:294-300 runs Model.forward per node), and every iteration picks one action per game
by the rule of alphazero.py:287-292, Q + c_puct * P * sqrt(Ntot) / (1 + N), runs one MCTS rollout below it
(`VecEnv.expand_rollout`, ONE launch for all G games) and backs the value up.

    python examples/az_puct_selfplay.py [--weights tests/golden/model_eval.npz | --model model.pt]
                                        [--games 1024] [--iters 72] [--sims 4] [--dtype f32|bf16]

--model: a state dict with nn.Model's ten keys (torch.load); --weights: an .npz of the same ten tensors with '.' written
'_' (tests/golden/model_eval.npz, the default).  Player 1 (X) searches, player 2 (O) plays the uniform-legal random
policy; prints P1's score.
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


def search_actions(env, net, iters, sims, sweep, c_puct=1.0):
    G, dev = env.num_envs, env.device
    legal = env.node_info(python_key=False)["legal"]                                  # bit a = action a legal (mcts.py:20-27)
    mask = (legal[:, None] >> torch.arange(36, device=dev)[None, :]) & 1 == 1          # [G, 36]
    P = torch.nan_to_num(env.evaluate(net, rows=("probs",))["probs"], nan=0.0)          # priors, one kernel for all G games
    N = torch.zeros((G, 36), device=dev)
    W = torch.zeros((G, 36), device=dev)
    out = None
    work = VecEnv.from_state(env.state, G, seed=env.seed + 7919 * (sweep + 1), board_offset=env.board_offset)
    for it in range(iters):
        Q = W / N.clamp(min=1)
        U = c_puct * P * torch.sqrt(N.sum(1, keepdim=True) + 1.0) / (1.0 + N)            # alphazero.py:289-291
        a = torch.where(mask, Q + U, torch.full_like(Q, -math.inf)).argmax(1)
        out = work.expand_rollout(a.to(torch.uint8), n_sims=sims, step_idx0=32 * sims * it, out=out)
        nch = out["n_children"].to(torch.float32).clamp(min=1)
        # value_sum is signed for the player to move at the leaf (the mover's opponent, mcts.py:174); both collapse
        # branches are equally likely (mcts.py:195)
        v = -out["value_sum"].to(torch.float32).sum(1) / sims / nch
        N.scatter_add_(1, a[:, None], torch.ones((G, 1), device=dev))
        W.scatter_add_(1, a[:, None], v[:, None])
    return torch.where(mask, N, torch.full_like(N, -1.0)).argmax(1)                    # the most visited action


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=72)
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
    print("games %d  iterations %d x %d playouts per child :  P1 (root PUCT, network priors) wins %d (%.1f %%), P2 (random) wins %d, no winner %d"
          % (G, args.iters, args.sims, p1, 100.0 * p1 / G, p2, none))
    return p1 / G


if __name__ == "__main__":
    main()

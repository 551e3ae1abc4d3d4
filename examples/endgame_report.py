#!/usr/bin/env python3
"""How far the network and a search are from the truth, in absolute numbers: late positions are solved exactly
(VecEnv.solve, include/qttt_solve.h: the full expectimax tree, nothing sampled) and the value head, the policy and a
searched move are measured against the solution.

    python examples/endgame_report.py [--games 1024] [--min-ply 6] [--player azv:64] [--random]
                                      [--rollouts 32] [--sims 10] [--seed 0] [--dtype f32|bf16]
                                      [--weights tests/golden/model_eval.npz | --model model.pt]

The positions are the rows of SelfPlay.play() batches (the network's own value-leaf search, --rollouts per move) whose
position has at least --min-ply moves played and is not finished; with --random they come from the uniform-legal policy
(VecEnv.step_random_many) instead.  Printed:
  the value head's mean absolute error and bias against the exact value;
  the share of positions where the policy's argmax is an optimal move, and the policy's expected regret
    sum_a probs[a] * (V - Q(a));
  the same two figures for TreeSearch.choose() of --player (tree_tournament.py's mcts:R, az:R, azv:R, azg:R), searching
    from those positions, and for the uniform-legal policy as the baseline;
  the histogram of the exact values.
A regret is in units of game value: 0 for an optimal move, 2 for turning a certain win into a certain loss."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from qtttgym_amd import PolicyValueNet, SelfPlay, TreeSearch, VecEnv, _native  # noqa: E402
from qtttgym_amd import recommended_env  # noqa: E402
from tree_tournament import VALUE_KINDS, load_state_dict, parse_player  # noqa: E402
recommended_env(apply=True)


def joined(envs):
    """One VecEnv over the boards of several, in order (plane indexing only)."""
    P = torch.cat([e.state.view(torch.int64).view(2, -1)[:, :e.num_envs] for e in envs], dim=1)
    m = P.shape[1]
    st = torch.zeros(int(_native.lib().qttt_state_bytes(m)), dtype=torch.uint8, device=P.device)
    st.view(torch.int64).view(2, -1)[:, :m] = P
    return VecEnv.from_state(st, m)


def selfplay_positions(net, games, rollouts, min_ply, seed):
    sp = SelfPlay(games, n_rollouts=rollouts, net=net, leaf_eval="value", seed=seed)
    batch = sp.play()
    parts = []
    for t in range(min_ply, 9):                     # row t = the position after t moves; a ninth move ends every game
        live = (batch.length.to(torch.int64) > t) & (batch.done[t] == 0)
        sel = live.nonzero(as_tuple=True)[0]
        if sel.numel():
            parts.append(batch.row_env(t).take(sel))
    return joined(parts) if parts else None


def random_positions(games, min_ply, seed):
    env = VecEnv(games, seed=seed)
    env.step_random_many(min_ply)
    parts = []
    for t in range(min_ply, 9):
        info = env.node_info(python_key=False)
        sel = (~info["terminal"].bool() & (info["legal"] != 0)).nonzero(as_tuple=True)[0]
        if sel.numel():
            parts.append(env.take(sel))
        env.step_random_many(1)                     # a finished board's move is a noop
    return joined(parts) if parts else None


def searched_moves(pos, player, net, sims, seed, exact_from=None, prove=False):
    kind, R = player
    value = kind in VALUE_KINDS
    tree = TreeSearch(pos.num_envs, capacity=2 * R + 10, num_simulations=sims, net=net if kind == "az" or value else None,
                      seed=2 * seed + 1, device=pos.device, leaf_eval="value" if value else "playouts",
                      root_policy="gumbel" if kind == "azg" else "puct", exact_from=exact_from if value else None,
                      prove=prove and value and exact_from is not None)
    tree.reset(pos)
    tree.contemplate(R)
    return tree.choose(exact=True) if tree.prove else tree.choose()


def report(pos, sol, net, player, sims, seed, exact_from=None, prove=False):
    """The figures as a dict; `pos` holds unfinished positions only, all of them solved."""
    V, Q = sol.value.double(), sol.q.double()
    legal = torch.isfinite(Q)
    ev = pos.evaluate(net, rows=("value", "probs"))
    err = ev["value"].double() - V
    gap = torch.where(legal, V[:, None] - Q, torch.zeros_like(Q))              # V - Q(a), 0 at illegal actions
    probs = torch.where(legal, ev["probs"].double(), torch.zeros_like(Q))
    uniform = legal.double() / legal.sum(1, keepdim=True)
    out = {"positions": pos.num_envs, "value_mae": float(err.abs().mean()), "value_bias": float(err.mean()),
           "policy_optimal": float((sol.regret(probs.argmax(1)) == 0).double().mean()),
           "policy_regret": float((probs * gap).sum(1).mean()),
           "uniform_optimal": float(((gap == 0) & legal).double().sum(1).div(legal.sum(1)).mean()),
           "uniform_regret": float((uniform * gap).sum(1).mean())}
    if player[0] != "random":
        reg = sol.regret(searched_moves(pos, player, net, sims, seed, exact_from, prove)).double()
        out["search_optimal"], out["search_regret"] = float((reg == 0).double().mean()), float(reg.mean())
    values, counts = torch.unique(sol.value, return_counts=True)
    out["histogram"] = [(float(v), int(c)) for v, c in zip(values.cpu(), counts.cpu())]
    out["nodes"] = int(sol.nodes.sum())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--min-ply", type=int, default=6, help="solve positions with at least this many moves played (4..8)")
    ap.add_argument("--player", default="azv:64", help="the searched player: mcts:R, az:R, azv:R, azg:R or random (none)")
    ap.add_argument("--random", action="store_true", help="positions from the uniform-legal policy, not from self-play")
    ap.add_argument("--rollouts", type=int, default=32, help="rollouts per move of the self-play that makes the positions")
    ap.add_argument("--sims", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--model", default=None, help="state dict with nn.Model's keys (torch.load)")
    ap.add_argument("--weights", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                      "tests", "golden", "model_eval.npz"))
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--exact-from", type=int, default=None, metavar="M",
                    help="an azv or azg --player solves leaves with at least M (6..9) moves played exactly "
                         "(TreeSearch(exact_from=M))")
    ap.add_argument("--prove", action="store_true",
                    help="with --exact-from: prove interior nodes too and play the exact move at a proven root "
                         "(TreeSearch(prove=True), choose(exact=True))")
    args = ap.parse_args(argv)
    if args.prove and args.exact_from is None:
        raise SystemExit("--prove needs --exact-from")
    if not _native.SOLVE_MIN_PLY <= args.min_ply <= 8:
        raise SystemExit("--min-ply must be in %d..8" % _native.SOLVE_MIN_PLY)
    player = parse_player(args.player)
    net = PolicyValueNet(load_state_dict(args), device="cuda", dtype=torch.float32 if args.dtype == "f32" else torch.bfloat16)
    pos = random_positions(args.games, args.min_ply, args.seed) if args.random \
        else selfplay_positions(net, args.games, args.rollouts, args.min_ply, args.seed)
    if pos is None:
        raise SystemExit("no unfinished position with %d or more moves played" % args.min_ply)
    sol = pos.solve(min_ply=args.min_ply)
    assert bool(sol.solved.all()) and bool((sol.best < 36).all())
    r = report(pos, sol, net, player, args.sims, args.seed, args.exact_from, args.prove)
    src = "the uniform-legal policy" if args.random else "self-play (azv, %d rollouts per move)" % args.rollouts
    print("%d unfinished positions with >= %d moves played from %d games of %s, seed %d; %d positions enumerated"
          % (r["positions"], args.min_ply, args.games, src, args.seed, r["nodes"]))
    print("value head: mean absolute error %.4f, bias %+.4f" % (r["value_mae"], r["value_bias"]))
    print("policy: argmax optimal %.4f, expected regret %.4f" % (r["policy_optimal"], r["policy_regret"]))
    if "search_regret" in r:
        name = args.player + ("" if args.exact_from is None else " with exact leaves from %d moves" % args.exact_from) \
            + (" and proven nodes" if args.prove else "")
        print("search %s: move optimal %.4f, regret %.4f" % (name, r["search_optimal"], r["search_regret"]))
    print("uniform policy: move optimal %.4f, expected regret %.4f" % (r["uniform_optimal"], r["uniform_regret"]))
    print("exact values: " + ", ".join("%+.4f x %d" % vc for vc in r["histogram"]))
    return r


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The reference's self_play.py main loop (self_play.py:176-242) with the games on the device: every run plays --games
games of AlphaZero self-play under the current weights (qtttgym_amd.SelfPlay: the search trees, the moves and the
training samples never leave the GPU), trains the policy/value network on the batch with ordinary torch autograd (or,
with --device-train, on the device), packs the new weights for the search and repeats.

    python examples/selfplay_train.py [--games 1024] [--rollouts 100] [--sims 10] [--epochs 50] [--runs 30]
                                      [--dtype f32|bf16] [--out model.pt] [--model model.pt] [--value-targets 1,0]
                                      [--symmetries] [--leaf-eval playouts|value]
                                      [--root-noise EPS,ALPHA] [--temperature T] [--sample-plies K] [--leaves K]
                                      [--eval-symmetries all|0,4] [--replay CAPACITY --batch B --steps S]
                                      [--device-train] [--prioritized ALPHA,BETA] [--stream PLIES] [--exact-from M] [--prove]
                                      [--exact-targets M [--exact-value-only]]
                                      [--reanalyse N [--reanalyse-value-mix L]] [--value-mix L | --td-lambda L]

The network is nn.Model's (nn.py:7-28) under its own parameter names (qtttgym_amd.policy_value.SHAPES), so --out is a
state dict that the reference, PolicyValueNet and examples/tree_tournament.py --model all load.  The loss is the
reference's (self_play.py:226-236): 0.5 (v - v_target)^2 over every sample plus the KL divergence from the visit-count
target to the network's policy over the legal actions of the samples that are not terminal; the optimiser is its Adam
(lr 1e-3, weight decay 1e-3, amsgrad).  --value-targets 1,0 are the reference's targets, 1,-1 what it evidently meant
(qtttgym_amd.SelfPlay).  --dtype is the precision of the search's network; training is f32.  --symmetries trains on
every game's eight images under the board's symmetries (SelfPlayBatch.augment: eight times the samples for the same
search), which the reference left as a stub (self_play.py expand_symetries).  --leaf-eval value searches with the
network's value head at the leaves instead of --sims playouts (TreeSearch(leaf_eval="value")): the value head that every
run trains is then what the next run searches with; use --value-targets 1,-1 with it, the scale of a terminal leaf.
--root-noise 0.25,0.3 mixes Dirichlet(0.3) noise into the roots' priors before every searched move, and --sample-plies K
draws the move of the first K plies from the visit counts (N ** (1 / --temperature)) instead of playing the best one:
AlphaZero's root exploration (SelfPlay(root_noise=, temperature=, sample_plies=)), without which the games of a run under
--leaf-eval value all open alike.  --leaves K (with --leaf-eval value) searches K leaves per game per round, kept apart
by virtual loss (SelfPlay(leaves=K)): one network launch per round evaluates games * K leaves.  --eval-symmetries all
(or a list of 1, 2, 4 or 8 symmetries such as 0,4; with --leaf-eval value) searches with the network's outputs averaged
over every leaf's images (SelfPlay(eval_symmetries=...)): a search that treats mirrored positions alike.
--replay CAPACITY keeps a window of the last CAPACITY samples on the device (qtttgym_amd.ReplayBuffer) instead of training
on the latest run's games only: every run appends its games to the ring and trains --steps minibatches of --batch samples
drawn from it, each sample under a random symmetry of the board.  ReplayBuffer.add and .sample themselves never wait for
the host; the loss below (its boolean indexing) and the printed counts do.  --epochs and --symmetries are the full-batch
path's and are not used with it.
--device-train takes the training step to the device as well (qtttgym_amd.Trainer): the loss, its gradients and the
AMSGrad step run as HIP kernels on the packed weights that the search reads, so there is no autograd, no torch optimiser
and no repacking of the weights between runs; --out is then the trainer's state dict.
--prioritized ALPHA,BETA (with --replay and --device-train) draws the minibatches by priority (ReplayBuffer(prioritized=
True), Schaul et al.): every step weights the loss by the importance weights (F q / T) ** -BETA of its draw and writes
(L + J) ** ALPHA, the samples' own loss terms, back as their new priorities; a new sample enters at the largest priority
stored so far.  Nothing of it is read back.
--stream PLIES (with --replay) keeps the batch of --games game slots full instead of playing them in lockstep
(SelfPlay.stream): every run advances the slots by PLIES searched plies, a slot whose game ends hands its samples to the ring
and starts a new game at once, and the run's --steps minibatches follow.  The counters stay on the device; the printed
line reads them back once per run.
--exact-targets M (6..9) trains the late positions on the truth (SelfPlay(exact_targets=M)): every recorded, non-terminal
position with at least M moves played is enumerated on the device, its value target becomes its exact value for the
player to move and its policy target the uniform distribution over its optimal moves (--exact-value-only keeps the
visit-count policy).  The exact value is the mover's, in [-1, 1], so the option sets --value-targets to 1,-1 itself.
--reanalyse N (with --replay) refreshes the ring's targets (qtttgym_amd.Reanalyser): every run, after its games are in the
ring and before its minibatch steps, a window of N positions of the ring is searched again with the current weights and
the new policy targets are written into their slots; terminal rows and slots that were appended over in between keep what
they hold.  --reanalyse-value-mix L in (0, 1] also moves the value target towards the searched root value (needs
--value-targets 1,-1).  The printed count of refreshed samples is one more read-back per run.
--value-mix L and --td-lambda L (L in [0, 1], one of the two) take the value targets of the fresh samples from the search
that picked the moves (SelfPlay(value_mix= / td_lambda=), include/qttt_selfplay_value.h): the searched value of every
recorded root is kept on the device, and v becomes (1 - L) * outcome + L * searched value, or the TD(L) return over the
rest of the game, which runs through the exact rows of --exact-targets where there are some.  Either sets --value-targets
to 1,-1 itself; with --stream the rewrite sits between the harvest and the ring's append.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qtttgym_amd import PolicyValueNet, Reanalyser, ReplayBuffer, SelfPlay, Trainer  # noqa: E402
from qtttgym_amd import recommended_env  # noqa: E402
from qtttgym_amd.policy_value import HIDDEN, SHAPES  # noqa: E402
recommended_env(apply=True)


class Net(torch.nn.Module):
    """nn.Model (nn.py:7-42): three ReLU layers of 256 units on the flattened 18 x 10 input, a value head and a policy
    head, each a ReLU and a linear layer.  The parameter names are the reference's."""

    def __init__(self):
        super().__init__()
        relu, lin = torch.nn.ReLU, torch.nn.Linear
        self.fc = torch.nn.Sequential(lin(180, HIDDEN), relu(), lin(HIDDEN, HIDDEN), relu(), lin(HIDDEN, HIDDEN), relu())
        self.V_head = torch.nn.Sequential(relu(), lin(HIDDEN, 1))
        self.pi_head = torch.nn.Sequential(relu(), lin(HIDDEN, 36))
        assert {k: tuple(p.shape) for k, p in self.state_dict().items()} == SHAPES

    def forward(self, s):
        z = self.fc(s.flatten(-2, -1).float())
        return self.V_head(z).squeeze(-1), self.pi_head(z)


def loss_terms(net, s, pi, mask, v_target, done):
    """self_play.py:226-236: (L, J) = the value term per sample, the policy term per sample that is not terminal."""
    v, logits = net(s)
    keep = ~done
    logp = torch.log_softmax(logits[keep].masked_fill(~mask[keep], -float("inf")), dim=-1)      # nn.py:41
    p, legal = pi[keep], mask[keep]
    J = torch.zeros_like(p)
    J[legal] = p[legal] * (torch.log(p[legal] + 1e-7) - logp[legal])
    return 0.5 * (v - v_target).pow(2), J.sum(-1)


def train(model, optim, batches):
    """One optimiser step on every (s, pi, mask, v_target, done) of `batches`; the last step's (L, J)."""
    for samples in batches:
        L, J = loss_terms(model, *samples)
        loss = L.mean() + J.mean(0)
        optim.zero_grad()
        loss.backward()
        optim.step()
    return L, J


def train_on_device(trainer, batches):
    """The same with qtttgym_amd.Trainer: one step() per batch, no host synchronisation; the last step's (L, J), J over the
    samples that are not terminal as loss_terms gives it."""
    for samples in batches:
        L, J = trainer.step(*samples)
    return L, J[~samples[4]]


def train_prioritized(trainer, ring, batch, steps, alpha, beta):
    """`steps` minibatches drawn by priority: the importance weights of the draw go into the loss, the per-sample loss
    terms come back as the new priorities.  No host synchronisation; the last step's (L, J) as train_on_device gives them."""
    for _ in range(steps):
        samples = ring.sample(batch, "random")
        L, J = trainer.step(*samples, weight=ring.weights(beta))
        ring.update_priorities((L + J).clamp_min(0.0) ** alpha)
    return L, J[~samples[4]]


def parse_eval_symmetries(spec):
    """--eval-symmetries: None, "all", or the comma-separated list as ints."""
    return spec if spec in (None, "all") else tuple(int(k) for k in spec.split(","))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024, help="games per run (the reference's M = 50)")
    ap.add_argument("--rollouts", type=int, default=100, help="rollouts before every move (the reference's n_rollouts)")
    ap.add_argument("--sims", type=int, default=10, help="playouts per rollout (AlphaZero's num_simulations)")
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--out", default="model.pt")
    ap.add_argument("--model", default=None, help="state dict to start from (default: torch's initialisation)")
    ap.add_argument("--value-targets", default="1,0", help="v of the first row when the first / second player wins")
    ap.add_argument("--symmetries", action="store_true", help="train on the eight images of every game")
    ap.add_argument("--leaf-eval", choices=("playouts", "value"), default="playouts",
                    help="what scores a leaf of the search: --sims playouts, or the network's value head")
    ap.add_argument("--leaves", type=int, default=1,
                    help="leaves per game per round of the search (SelfPlay(leaves=K): virtual loss; needs --leaf-eval value)")
    ap.add_argument("--eval-symmetries", default=None, metavar="all|K,K,...",
                    help="average the search's network over these symmetries of every leaf (needs --leaf-eval value)")
    ap.add_argument("--root-noise", default=None, metavar="EPS,ALPHA",
                    help="Dirichlet(ALPHA) noise with weight EPS on the roots' priors before every searched move")
    ap.add_argument("--temperature", type=float, default=1.0, help="the sampled moves follow N ** (1 / temperature)")
    ap.add_argument("--sample-plies", type=int, default=0, help="plies whose move is drawn from the visit counts")
    ap.add_argument("--forced-playouts", type=float, default=None, metavar="K",
                    help="forced playouts at the PUCT root and pruned policy targets (SelfPlay(forced_playouts=K), "
                         "include/qttt_tree_forced.h; KataGo uses 2; needs --leaf-eval value): what makes --root-noise "
                         "work at small --rollouts")
    ap.add_argument("--no-prune-targets", action="store_true",
                    help="with --forced-playouts: force only, record the unpruned visit counts (SelfPlay(prune_targets=False))")
    ap.add_argument("--playout-cap", default=None, metavar="P,N",
                    help="playout cap randomisation (SelfPlay(playout_cap=(P, N)), include/qttt_selfplay_cap.h; KataGo uses "
                         "0.25 and a fifth of --rollouts; needs --leaf-eval value): a fraction P of the plies gets the full "
                         "search and is recorded, the others N rollouts without noise and no sample")
    ap.add_argument("--resident", action="store_true",
                    help="the resident search (SelfPlay(resident=True), include/qttt_tree_resident.h; needs --leaf-eval value): "
                         "every round of a ply inside one fused launch, the same games bit for bit")
    ap.add_argument("--root-policy", choices=("puct", "gumbel"), default="puct",
                    help="gumbel: the Gumbel root, sequential halving over --max-considered actions; pi is then the "
                         "improved policy and the move the best survivor (needs --leaf-eval value; --rollouts of 16-32 do)")
    ap.add_argument("--max-considered", type=int, default=16, help="actions the Gumbel root samples (1..36)")
    ap.add_argument("--replay", type=int, default=0, metavar="CAPACITY",
                    help="train on minibatches drawn from a ring of the last CAPACITY samples (0: on the latest run's games)")
    ap.add_argument("--batch", type=int, default=1024, help="with --replay: samples per minibatch")
    ap.add_argument("--steps", type=int, default=50, help="with --replay: minibatch steps per run")
    ap.add_argument("--device-train", action="store_true",
                    help="loss, gradients and the optimiser on the device, on the search's packed weights (Trainer)")
    ap.add_argument("--prioritized", default=None, metavar="ALPHA,BETA",
                    help="with --replay and --device-train: draw the minibatches by priority (L + J) ** ALPHA and weight the "
                         "loss by the importance weights (F q / T) ** -BETA")
    ap.add_argument("--stream", type=int, default=0, metavar="PLIES",
                    help="with --replay: every run is PLIES plies of continuous self-play (finished games restart in "
                         "place and feed the ring) instead of one batch of games in lockstep")
    ap.add_argument("--exact-from", type=int, default=None, metavar="M",
                    help="leaves with at least M (6..9) moves played are solved exactly on the device "
                         "(SelfPlay(exact_from=M); needs --leaf-eval value)")
    ap.add_argument("--prove", action="store_true",
                    help="with --exact-from: the search proves interior nodes too (SelfPlay(prove=True))")
    ap.add_argument("--exact-targets", type=int, default=None, metavar="M",
                    help="positions with at least M (6..9) moves played get their exact value and optimal-move policy as "
                         "targets (SelfPlay(exact_targets=M)); sets --value-targets 1,-1.  From M = 7 the relabelling is nearly "
                         "free; at M = 6 a --stream ply takes about four times as long (DESIGN.md §25)")
    ap.add_argument("--exact-value-only", action="store_true",
                    help="with --exact-targets: relabel the value target only, keep the visit-count policy")
    ap.add_argument("--reanalyse", type=int, default=0, metavar="N",
                    help="with --replay: every run searches N positions of the ring again with the current weights and "
                         "refreshes their policy targets in place (Reanalyser)")
    ap.add_argument("--reanalyse-value-mix", type=float, default=0.0, metavar="L",
                    help="with --reanalyse: v = (1 - L) * stored v + L * the searched root value (needs --value-targets 1,-1)")
    ap.add_argument("--value-mix", type=float, default=None, metavar="L",
                    help="v = (1 - L) * the game's outcome + L * the searched root value on every fresh sample "
                         "(SelfPlay(value_mix=L)); sets --value-targets 1,-1")
    ap.add_argument("--td-lambda", type=float, default=None, metavar="L",
                    help="v = the TD(L) return over the searched root values of the rest of the game "
                         "(SelfPlay(td_lambda=L): 1 is the outcome, 0 the one-step target); sets --value-targets 1,-1")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.value_mix is not None and args.td_lambda is not None:
        ap.error("--value-mix and --td-lambda exclude each other")
    if args.reanalyse < 0 or (args.reanalyse and not args.replay):
        ap.error("--reanalyse needs N >= 1 and --replay")
    if args.reanalyse_value_mix and not args.reanalyse:
        ap.error("--reanalyse-value-mix needs --reanalyse")
    if args.stream < 0 or (args.stream and not args.replay):
        ap.error("--stream needs PLIES >= 1 and --replay")
    if args.prove and args.exact_from is None:
        ap.error("--prove needs --exact-from")
    if args.replay and (args.batch < 1 or args.steps < 1):
        ap.error("--replay needs --batch >= 1 and --steps >= 1")
    if args.prioritized is not None and not (args.replay and args.device_train):
        ap.error("--prioritized needs --replay and --device-train (the weighted loss is the device trainer's)")
    alpha, beta = (float(x) for x in args.prioritized.split(",")) if args.prioritized is not None else (0.0, 0.0)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", torch.cuda.current_device())
    model = Net().to(dev)
    if args.model:
        model.load_state_dict(torch.load(args.model, map_location=dev))
    optim = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-3, amsgrad=True)      # nn.py:27
    net = PolicyValueNet(model, device=dev, dtype=torch.float32 if args.dtype == "f32" else torch.bfloat16)
    if args.no_prune_targets and args.forced_playouts is None:
        ap.error("--no-prune-targets needs --forced-playouts")
    if args.exact_value_only and args.exact_targets is None:
        ap.error("--exact-value-only needs --exact-targets")
    zero_sum = args.exact_targets is not None or args.value_mix is not None or args.td_lambda is not None
    targets = (1.0, -1.0) if zero_sum else tuple(float(x) for x in args.value_targets.split(","))
    sp = SelfPlay(args.games, n_rollouts=args.rollouts, num_simulations=args.sims, net=net, value_targets=targets,
                  seed=args.seed, leaf_eval=args.leaf_eval, leaves=args.leaves,
                  root_noise=None if args.root_noise is None else tuple(float(x) for x in args.root_noise.split(",")),
                  temperature=args.temperature, sample_plies=args.sample_plies,
                  eval_symmetries=parse_eval_symmetries(args.eval_symmetries), root_policy=args.root_policy,
                  max_considered=args.max_considered, exact_from=args.exact_from, prove=args.prove,
                  exact_targets=args.exact_targets, exact_policy=not args.exact_value_only,
                  value_mix=args.value_mix, td_lambda=args.td_lambda, forced_playouts=args.forced_playouts,
                  prune_targets=None if args.forced_playouts is None else not args.no_prune_targets,
                  playout_cap=None if args.playout_cap is None else (float(args.playout_cap.split(",")[0]),
                                                                     int(args.playout_cap.split(",")[1])),
                  resident=args.resident)
    ring = ReplayBuffer(args.replay, device=dev, seed=args.seed, prioritized=args.prioritized is not None) if args.replay else None
    reanalyser = Reanalyser(sp, ring, args.reanalyse, value_mix=args.reanalyse_value_mix, seed=args.seed) if args.reanalyse else None
    trainer = Trainer(model, device=dev, net=net) if args.device_train else None      # nn.py:27's defaults
    if args.prioritized is not None:
        fit, save = (lambda batches: train_prioritized(trainer, ring, args.batch, args.steps, alpha, beta)), trainer.state_dict
    elif trainer is not None:
        fit, save = (lambda batches: train_on_device(trainer, batches)), trainer.state_dict
    else:
        fit, save = (lambda batches: train(model, optim, batches)), model.state_dict
    seen = torch.zeros(5, dtype=torch.int64)                  # games, samples, winners[3] of the stream so far
    for run in range(args.runs):
        if args.stream:
            stats = sp.stream(ring, args.stream)
            refreshed = reanalyser.run().updated if reanalyser is not None else None
            L, J = fit(ring.sample(args.batch, "random") for _ in range(args.steps))
            now = torch.cat([stats.games.sum().view(1), stats.samples.view(1), stats.winners]).cpu()     # the one read-back
            new, seen = (now - seen).tolist(), now
            won = new[2:]
            what = ("%d plies: %d games harvested, %d samples appended, the ring holds %d; %d steps of %d"
                    % (args.stream, new[0], new[1], min(int(now[1]), args.replay), args.steps, args.batch))
        else:
            batch = sp.play()
            won = [int((batch.winner == w).sum()) for w in (1, 0, -1)]
            if ring is not None:
                ring.add(batch)
                refreshed = reanalyser.run().updated if reanalyser is not None else None
                L, J = fit(ring.sample(args.batch, "random") for _ in range(args.steps))
                what = ("%d games appended, the ring holds %d samples; %d steps of %d"
                        % (args.games, ring.size(), args.steps, args.batch))
            else:
                samples = (batch.augment() if args.symmetries else batch).flat()
                L, J = fit(samples for _ in range(args.epochs))
                what = "%d samples of %d games" % (len(samples[0]), args.games)
        if reanalyser is not None:
            what += "; %d of %d reanalysed samples refreshed" % (int(refreshed.sum()), args.reanalyse)
        print("run %d: %s (first player won %d, lost %d, drew %d); L: %.4f, J: %.4f"
              % (run, what, won[0], won[1], won[2], L.mean().item(), J.mean().item()), flush=True)
        if trainer is None:
            net.load_state_dict(model)                       # the next run searches with the new weights
        torch.save(save(), args.out)

if __name__ == "__main__":
    main()

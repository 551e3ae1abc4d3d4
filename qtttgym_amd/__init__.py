"""qtttgym_amd — MI355X-native vectorised Quantum Tic-Tac-Toe environment.

Exports the reference package's four names (qtttgym/__init__.py:1-4) plus `VecEnv`, `PolicyValueNet` (the
reference's nn.py network, evaluated on the GPU), `TreeSearch` (batched
MCTS / AlphaZero search trees on the device), `SelfPlay` (self_play.py's games and training samples, batched),
`ReplayBuffer` (the window of recent samples a trainer draws its minibatches from, on the device), `Reanalyser` (positions
of that window searched again with the current network, their targets refreshed in place), `Trainer` (the
reference's loss, its gradients and its AMSGrad step on the packed weights the search reads), `SolveResult` (what
`VecEnv.solve`, the exact endgame solver, returns) and the 36-action
indexing L3 callers share (mcts.py:339-350)."""
from .vec_env import VecEnv
from .board import Board, QEvalClassic, displayBoard
from .env import Env
from .actions import ind2move, move2ind
from ._native import recommended_env, retire_mailbox
from .policy_value import PolicyValueNet
from .tree import TreeSearch
from .selfplay import SelfPlay, SelfPlayBatch, StreamStats
from .replay import ReplayBuffer, ReplayWindow
from .reanalyse import Reanalyser, ReanalyseStats
from .train import Trainer
from .solve import SolveResult

__all__ = ["Board", "QEvalClassic", "displayBoard", "Env", "VecEnv", "PolicyValueNet", "TreeSearch", "SelfPlay", "SelfPlayBatch", "StreamStats", "ReplayBuffer", "ReplayWindow", "Reanalyser", "ReanalyseStats", "Trainer", "SolveResult", "ind2move", "move2ind", "recommended_env",
           "retire_mailbox"]

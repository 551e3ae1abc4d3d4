"""The training step on the MI355X (include/qttt_train.h, qtttgym_amd.Trainer) against the float64 autograd
model of tests/train_model.py: the gradients of every parameter tensor and the per-sample loss terms at the sizes that
cover the tile tails and the chunk tails, the exact properties (repeatable bits, nothing read before it is written, +0
where the contract says +0, guard bytes), the AMSGrad step against its float64 restatement, the two ways a PolicyValueNet
follows the training, and a loss that goes down.

Every bound is MARGIN (8) times what float32 itself does to the same inputs (the model run in float32 against the model
run in float64), with a floor of one f32 ulp of the tensor's largest element; none is taken from the kernel's results."""
import functools

import pytest
import torch

import train_model as M
from nn_reference64 import KEYS, golden_state_dict, load_golden, random_play_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = M.CHUNK
SIZES = list(dict.fromkeys([1, 63, 64, 65, 257, C + 1, 2 * C + 1]))      # C + 1 is 257 with a chunk of 256


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _state_dict(kind):
    if kind == "fixture":
        return golden_state_dict(load_golden())
    from qtttgym_amd.policy_value import SHAPES
    gen = torch.Generator().manual_seed(11)
    return {k: torch.randn(shp, generator=gen) * 0.05 for k, shp in SHAPES.items()}


@functools.lru_cache(maxsize=None)
def _batch(n, seed=0):
    """(s, pi, mask, v, done) on the device as flat() / ReplayBuffer.sample give them: positions of random play at every
    depth, the legal mask from evaluate's -inf pattern, a random normalised pi on the legal actions, v in {-1, 0, 1}, done
    on the positions without a legal action and on a random fifth of the others (never on sample 0 if it has a legal action)."""
    from qtttgym_amd import PolicyValueNet, VecEnv
    if n >= 24:
        env = random_play_env(n, 100 + n + seed, DEV)
    else:
        env = VecEnv(n, device=DEV, seed=100 + n + seed, auto_reset=True)
        env.step_random_many(5)
    s = env.encode(with_mask=False)
    logits = env.evaluate(PolicyValueNet(_state_dict("random"), device=DEV), rows=("logits",))["logits"]
    mask = ~torch.isneginf(logits).cpu()
    gen = torch.Generator().manual_seed(1000 * n + seed)
    pi = torch.rand((n, 36), generator=gen, dtype=torch.float64) * mask
    pi = pi / pi.sum(1, keepdim=True).clamp_min(1e-300)
    v = torch.randint(-1, 2, (n,), generator=gen).to(torch.float32)
    done = ~mask.any(1) | (torch.rand(n, generator=gen) < 0.2)
    done[0] = not bool(mask[0].any())                                    # every case keeps a sample that is not terminal
    return s, pi.to(DEV), mask.to(DEV), v.to(DEV), done.to(DEV)


@functools.lru_cache(maxsize=None)
def _reference(n, kind, seed=0):
    """The model's (grads, L, J, loss) in float64 and in float32, computed once per case."""
    return M.gradients(_state_dict(kind), _batch(n, seed), torch.float64), M.gradients(_state_dict(kind), _batch(n, seed), torch.float32)


def _trainer(kind="random", **kw):
    from qtttgym_amd import Trainer
    return Trainer(_state_dict(kind), device=DEV, **kw)


@pytest.mark.parametrize("kind", ["random", "fixture"])
@pytest.mark.parametrize("n", SIZES)
def test_gradients_against_float64(n, kind):
    batch = _batch(n)
    assert not bool(batch[4].all()), "the case needs a sample that is not terminal"
    (g64, L64, J64, _), (g32, L32, J32, _) = _reference(n, kind)
    tr = _trainer(kind)
    L, J = tr.gradients(*batch)
    got = {k: t.double().cpu() for k, t in tr.grad_dict().items()}
    got["L"], got["J"] = L.double().cpu(), J.double().cpu()
    ref64, ref32 = dict(g64, L=L64, J=J64), dict(g32, L=L32, J=J32)
    ratios = {}
    for k in KEYS + ("L", "J"):
        err, allowed = (got[k] - ref64[k]).abs().max().item(), M.bound(ref32[k], ref64[k])
        ratios[k] = M.MARGIN * err / allowed if allowed else (0.0 if err == 0 else float("inf"))
    worst = max(ratios, key=ratios.get)
    print("n=%d %s: largest error / allowance unit = %.3f at %s (the margin is %g)" % (n, kind, ratios[worst], worst, M.MARGIN))
    assert ratios[worst] <= M.MARGIN, ratios
    assert torch.equal(_bits(J)[batch[4]], torch.zeros_like(_bits(J)[batch[4]])), "J of a terminal sample is +0"


def test_two_calls_give_the_same_bits_and_nothing_is_read_before_it_is_written():
    n = 2 * C + 1
    batch = _batch(n)
    tr = _trainer()
    L0, J0 = tr.gradients(*batch)
    g0 = tr.grads.clone()
    L1, J1 = tr.gradients(*batch)
    assert torch.equal(tr.grads, g0) and torch.equal(_bits(L0), _bits(L1)) and torch.equal(_bits(J0), _bits(J1))
    for fill in (0x00, 0xFF):                                            # 0xFF bytes: every f32 a NaN
        tr.grads.fill_(fill)
        tr._workspace.fill_(fill)
        L2, J2 = tr.gradients(*batch)
        assert torch.equal(tr.grads, g0) and torch.equal(_bits(L0), _bits(L2)) and torch.equal(_bits(J0), _bits(J2)), fill
    assert not torch.isnan(tr.grads.view(torch.float32)).any()


def _head(blob):
    """The head as an f32 blob holds it: f32[256, 48] (36 policy columns, the value, 11 pads) and its 48 biases."""
    from qtttgym_amd.policy_value import HEAD_COLS, HIDDEN, _matrix
    g = blob.view(torch.float32)
    at = 180 * HIDDEN + 2 * HIDDEN * HIDDEN
    return _matrix(g[at:at + HIDDEN * HEAD_COLS], HIDDEN, HEAD_COLS, torch.float32), g[at + HIDDEN * HEAD_COLS + 3 * HIDDEN:]


def test_an_action_that_is_never_legal_and_the_pads_get_exactly_zero():
    a = 17
    s, pi, mask, v, done = (t.clone() for t in _batch(257))
    mask[:, a] = False
    pi[:, a] = 0
    done |= ~mask.any(1)
    tr = _trainer()
    tr.grads.fill_(0xFF)
    tr.gradients(s, pi, mask, v, done)
    gd = tr.grad_dict()
    wh, bh = _head(tr.grads)
    assert bh.numel() == 48
    for t in (gd["pi_head.1.weight"][a], gd["pi_head.1.bias"][a], wh[:, 37:], bh[37:]):
        assert torch.equal(_bits(t), torch.zeros_like(_bits(t)))                 # +0, not -0 and not tiny
    assert gd["pi_head.1.weight"][a - 1].abs().max() > 0 and wh[:, 36].abs().max() > 0


def test_an_all_done_batch_has_no_policy_term():
    s, pi, mask, v, done = _batch(257)
    tr = _trainer()
    tr.grads.fill_(0xFF)
    L, J = tr.gradients(s, pi, mask, v, torch.ones_like(done))
    gd = tr.grad_dict()
    for t in (gd["pi_head.1.weight"], gd["pi_head.1.bias"], J):
        assert torch.equal(_bits(t), torch.zeros_like(_bits(t)))
    assert gd["V_head.1.weight"].abs().max() > 0 and gd["fc.0.weight"].abs().max() > 0 and (L > 0).any()
    assert not any(torch.isnan(t).any() for t in gd.values())


@pytest.mark.parametrize("n", [1, 65, C + 1])
def test_guard_bytes_after_every_output_stay_untouched(n):
    from qtttgym_amd import _native
    GUARD, batch, tr = 4096, _batch(n), _trainer()
    sizes = {"grads": tr.weights.numel(), "L": 4 * n, "J": 4 * n, "ws": int(_native.lib().qttt_train_workspace_bytes(n))}
    buf = {k: torch.full((b + GUARD,), 0xA5, dtype=torch.uint8, device=DEV) for k, b in sizes.items()}
    tr._call("qttt_train_gradients", *[t.data_ptr() for t in batch], n, tr.weights.data_ptr(), buf["grads"].data_ptr(),
             buf["L"].data_ptr(), buf["J"].data_ptr(), buf["ws"].data_ptr())
    torch.cuda.synchronize()
    for k, b in sizes.items():
        assert bool((buf[k][b:] == 0xA5).all()), k
    L, J = tr.gradients(*batch)                                           # and the call wrote what the Trainer's own call writes
    assert torch.equal(buf["grads"][:sizes["grads"]], tr.grads)
    assert torch.equal(buf["L"][:4 * n], L.view(torch.uint8)) and torch.equal(buf["J"][:4 * n], J.view(torch.uint8))


def test_a_sample_past_the_tail_changes_the_result():
    """n = 65 is checked against the model above: rows 65..127 of the second tile contribute nothing.  A 66th sample does."""
    big = tuple(t.clone() for t in _batch(257))
    big[4][:66] = False
    big[4][:66] |= ~big[2][:66].any(1)
    tr = _trainer()
    tr.gradients(*[t[:65].contiguous() for t in big])
    g65 = tr.grads.clone()
    tr.gradients(*[t[:66].contiguous() for t in big])
    assert not torch.equal(g65, tr.grads)
    tr.gradients(*[t[:65].contiguous() for t in big])
    assert torch.equal(g65, tr.grads)


def test_three_steps_against_the_float64_recurrence():
    """Three AMSGrad steps from zero state on 257 samples.  The expected weights: the float64 model's gradient at the float64
    weights, then the header's five lines in float64.  The allowance: 8 x the distance from that of the same thing carried
    in float32 on the CPU (float32 gradients at float32 weights, float32 recurrence), floor one ulp of the largest weight."""
    batch = _batch(257)
    tr = _trainer()
    a64, a32 = M.Adam(_state_dict("random"), torch.float64), M.Adam(_state_dict("random"), torch.float32)
    vmax_before = tr.vmax.view(torch.float32).clone()
    for t in range(1, 4):
        a64.step(M.gradients(a64.w, batch, torch.float64)[0])
        a32.step(M.gradients(a32.w, batch, torch.float32)[0])
        tr.step(*batch)
        assert tr.step_count == t
        got, ratios = tr.state_dict(), {}
        for k in KEYS:
            err, allowed = (got[k].double().cpu() - a64.w[k]).abs().max().item(), M.bound(a32.w[k], a64.w[k])
            ratios[k] = M.MARGIN * err / allowed
        worst = max(ratios, key=ratios.get)
        print("step %d: largest error / allowance unit = %.3f at %s (the margin is %g)" % (t, ratios[worst], worst, M.MARGIN))
        assert ratios[worst] <= M.MARGIN, (t, ratios)
        vmax = tr.vmax.view(torch.float32).clone()
        assert bool((vmax >= vmax_before).all()) and bool((vmax >= tr.v2.view(torch.float32)).all())
        vmax_before = vmax
        wh, bh = _head(tr.weights)                                       # the pads stay exactly zero
        for pad in (wh[:, 37:], bh[37:]):
            assert torch.equal(_bits(pad), torch.zeros_like(_bits(pad)))


def test_a_bf16_net_is_rewritten_by_the_step():
    from qtttgym_amd import PolicyValueNet
    from qtttgym_amd.policy_value import pack_weights
    net = PolicyValueNet(_state_dict("fixture"), device=DEV, dtype=torch.bfloat16)
    tr = _trainer("random", net=net)
    assert torch.equal(net.blob, pack_weights(tr.state_dict(), torch.bfloat16))          # the trainer's weights from the start
    assert tr.weights.data_ptr() != net.blob.data_ptr()
    for _ in range(2):
        before = net.blob.clone()
        tr.step(*_batch(257))
        assert torch.equal(net.blob, pack_weights(tr.state_dict(), torch.bfloat16))
        assert not torch.equal(net.blob, before)


def test_an_f32_net_shares_the_trainers_weights():
    from qtttgym_amd import PolicyValueNet, VecEnv
    net = PolicyValueNet(_state_dict("fixture"), device=DEV)
    address = net.blob.data_ptr()
    tr = _trainer("random", net=net)
    assert tr.weights.data_ptr() == net.blob.data_ptr() == address
    env = VecEnv(300, device=DEV, seed=5, auto_reset=True)
    env.step_random_many(4)
    before = {k: t.clone() for k, t in env.evaluate(net, rows=("value", "logits")).items()}
    tr.step(*_batch(257))
    assert net.blob.data_ptr() == tr.weights.data_ptr() == address
    out = env.evaluate(net, rows=("value", "logits"))
    fresh = env.evaluate(PolicyValueNet(tr.state_dict(), device=DEV), rows=("value", "logits"))
    for k in out:
        assert torch.equal(_bits(out[k]), _bits(fresh[k])), k
    assert not torch.equal(out["value"], before["value"])


def test_thirty_steps_lower_the_loss():
    batch = _batch(512)
    keep = ~batch[4]
    tr = _trainer()
    L, J = tr.gradients(*batch)
    before = (L.mean() + J[keep].mean()).item()
    for _ in range(30):
        tr.step(*batch)
    L, J = tr.gradients(*batch)
    after = (L.mean() + J[keep].mean()).item()
    print("loss %.6f -> %.6f after 30 steps" % (before, after))
    assert after < before


@pytest.mark.parametrize("extra", [(), ("--replay", "4096", "--batch", "257", "--steps", "2"), ("--dtype", "bf16")])
def test_selfplay_train_example_trains_on_the_device(tmp_path, extra):
    """examples/selfplay_train.py --device-train: two runs (the second searches with the first's step), finite losses, and
    a state dict that the search loads and that is not the initial one."""
    import math
    import os
    import re
    import subprocess
    import sys
    from qtttgym_amd import PolicyValueNet
    from qtttgym_amd.policy_value import SHAPES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = tmp_path / "model.pt"
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "selfplay_train.py"), "--games", "64", "--rollouts", "8",
                          "--sims", "2", "--epochs", "2", "--runs", "2", "--device-train", *extra, "--out", str(out_path)],
                         capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    runs = re.findall(r"run (\d): .*L: (\S+), J: (\S+)", out.stdout)
    assert [r[0] for r in runs] == ["0", "1"], out.stdout
    assert all(math.isfinite(float(x)) for r in runs for x in r[1:]), out.stdout
    sd = torch.load(out_path, map_location="cpu")
    assert {k: tuple(v.shape) for k, v in sd.items()} == SHAPES
    assert all(torch.isfinite(v).all() for v in sd.values())
    PolicyValueNet(sd, device=DEV)

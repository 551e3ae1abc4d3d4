"""step_many(actions) without output buffers with the boards held in registers (step_fused_kernel's output-free ply loop):
asked for with fused=True at any size, and taken by default in the one-round rows of auto_tuning() (csrc/qttt_launch.h:
448 K < n <= 1536 K boards, runs of 16 steps or more, no launch shape named).  Bit for bit against the same steps taken
one by one through step_raw: the state, the returned reward (IEEE bits) and terminated — the last step's —, step_idx, and
one more step_raw afterwards on both environments.  reward / terminated are pre-filled with 7.0 / True, so that a store
that never happened shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOOP_N = (1, 63, 64, 65, 511, 512, 513, 1023, 1025, 5003)
LOOP_T = (1, 2, 3, 63, 64, 65, 129)          # run splitting at 64 plies, the last launch alone stores, prefetch deeper than T
ROUTE_T = (2, 7, 15, 16, 65)                 # below / at the route's shortest run, and a run of two launches
INSIDE = (458752 + 2048, 655360, 1048576, 1572864)
OUTSIDE = (458752, 1572864 + 4096)
ABOVE_2_32 = (1 << 32) + 12345


def _offset_copy(x, lead):
    """the same bytes `lead` bytes into an allocation of their own"""
    buf = torch.empty(x.numel() + lead, dtype=torch.uint8, device="cuda")
    y = buf[lead:].view(x.shape)
    y.copy_(x)
    assert y.data_ptr() % 4 == lead % 4 and y.is_contiguous()
    return y


def _reference(n, steps, seed, auto_reset, off, explicit_bits):
    """T_max + 1 steps of the uniform-legal policy taken one by one, computed ONCE per case: the actions (and the explicit
    collapse bits), and after each T of `steps` the state, the reward bits and terminated; the environment that took them
    is left after step T_max."""
    from qtttgym_amd import VecEnv
    T_max = max(steps)
    rec = VecEnv(n, seed=seed, auto_reset=auto_reset, board_offset=off)
    acts = torch.empty((T_max + 1, n, 2), dtype=torch.uint8, device="cuda")
    bits = None
    if explicit_bits:
        g = torch.Generator(device="cuda").manual_seed(seed + 17)
        bits = torch.randint(0, 2, (T_max + 1, n), dtype=torch.uint8, device="cuda", generator=g)
    snaps = {}
    for t in range(T_max):
        rec.sample_actions(out=acts[t])
        r, tm = rec.step_raw(acts[t], None if bits is None else bits[t])
        if t + 1 in steps:
            snaps[t + 1] = (rec.state.clone(), r.view(torch.int32).clone(), tm.clone())
    rec.sample_actions(out=acts[T_max])
    return acts, bits, snaps


def _check(n, steps, auto_reset, explicit_bits, off=0, fused=False, launch_shape=None, misalign=False):
    from qtttgym_amd import VecEnv
    seed = 2000 + n % 977
    acts, bits, snaps = _reference(n, steps, seed, auto_reset, off, explicit_bits)
    a_in, b_in = acts, bits
    if misalign:
        a_in = _offset_copy(acts, 2)             # one board in: 2-byte but not 4-byte aligned
        if bits is not None:
            b_in = _offset_copy(bits, 1)         # explicit bits from an odd address
    kw = dict(seed=seed, auto_reset=auto_reset, board_offset=off)
    for T in steps:
        tag = (n, T, auto_reset, explicit_bits, off, fused, launch_shape, misalign)
        many = VecEnv(n, launch_shape=launch_shape, **kw)
        many._reward.fill_(7.0)
        many._terminated.fill_(True)
        r, tm = many.step_many(a_in[:T], None if b_in is None else b_in[:T], fused=fused)
        assert r is many._reward and tm is many._terminated and many.step_idx == T, tag
        state, r_bits, term = snaps[T]
        assert torch.equal(many.state, state), tag
        assert torch.equal(r.view(torch.int32), r_bits), tag
        assert torch.equal(tm, term), tag
        # one more step on both: the environments go on alike
        single = VecEnv(n, **kw)
        single.state.copy_(state)
        single.step_idx = T
        r, tm = many.step_raw(acts[T], None if bits is None else bits[T])
        rs, ts = single.step_raw(acts[T], None if bits is None else bits[T])
        assert many.step_idx == single.step_idx == T + 1, tag
        assert torch.equal(many.state, single.state), tag
        assert torch.equal(r.view(torch.int32), rs.view(torch.int32)) and torch.equal(tm, ts), tag


@pytest.mark.parametrize("n", LOOP_N)
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_output_free_loop_equals_single_steps(n, auto_reset, explicit_bits):
    _check(n, LOOP_T, auto_reset, explicit_bits, fused=True)


@pytest.mark.parametrize("n", [1, 65, 513, 5003])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_output_free_loop_board_ids_above_2_pow_32_and_odd_addresses(n, auto_reset, explicit_bits):
    _check(n, LOOP_T, auto_reset, explicit_bits, off=ABOVE_2_32, fused=True)
    _check(n, LOOP_T, auto_reset, explicit_bits, fused=True, misalign=True)


@pytest.mark.parametrize("n", INSIDE + OUTSIDE)
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_default_route_at_its_edges(n, auto_reset, explicit_bits):
    _check(n, ROUTE_T, auto_reset, explicit_bits)


@pytest.mark.parametrize("n", INSIDE)
@pytest.mark.parametrize("variant", ["across_2_pow_32", "shape_named", "actions_one_board_in"])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_default_route_inside_falls_back_or_not_and_agrees(n, variant, auto_reset, explicit_bits):
    if variant == "across_2_pow_32":
        _check(n, ROUTE_T, auto_reset, explicit_bits, off=(1 << 32) - n // 2 - 1)      # the per-step loop, cut at the multiple
    elif variant == "shape_named":
        _check(n, ROUTE_T, auto_reset, explicit_bits, launch_shape=(2, 512))            # the per-step loop in that shape
    else:
        _check(n, ROUTE_T, auto_reset, explicit_bits, misalign=True)


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
@pytest.mark.parametrize("fused", [False, True])
def test_output_buffers_given_every_row_is_filled_as_before(auto_reset, explicit_bits, fused):
    """reward=[T,N] / terminated=[T,N]: every step's outputs are kept — the per-step loop, or (fused) the loop that stores
    every ply, which is the kernel from before the output-free one."""
    from qtttgym_amd import VecEnv
    n, T, seed = 655360, 65, 31
    acts, bits, snaps = _reference(n, (T,), seed, auto_reset, 0, explicit_bits)
    many, single = VecEnv(n, seed=seed, auto_reset=auto_reset), VecEnv(n, seed=seed, auto_reset=auto_reset)
    rew = torch.full((T, n), 7.0, dtype=torch.float32, device="cuda")
    term = torch.ones((T, n), dtype=torch.bool, device="cuda")
    r, tm = many.step_many(acts[:T], None if bits is None else bits[:T], reward=rew, terminated=term, fused=fused)
    assert r is rew and tm is term and many.step_idx == T
    for t in range(T):
        rs, ts = single.step_raw(acts[t], None if bits is None else bits[t])
        assert torch.equal(rew[t].view(torch.int32), rs.view(torch.int32)) and torch.equal(term[t], ts), t
    assert torch.equal(many.state, single.state) and torch.equal(many.state, snaps[T][0])


def test_whole_episodes_against_the_oracle():
    """5 003 boards x 40 steps, fused, no outputs, against the port of the reference (oracle.OracleBoards.replay)."""
    import oracle
    from qtttgym_amd import VecEnv
    n, T, seed = 5003, 40, 77
    rec = VecEnv(n, seed=seed, auto_reset=True)
    acts = torch.empty((T, n, 2), dtype=torch.uint8, device="cuda")
    for t in range(T):
        rec.sample_actions(out=acts[t])
        rec.step_raw(acts[t])
    env = VecEnv(n, seed=seed, auto_reset=True)
    env._reward.fill_(7.0)
    env._terminated.fill_(True)
    r, tm = env.step_many(acts, fused=True)
    a_np = np.ascontiguousarray(acts.cpu().numpy())
    ob = oracle.OracleBoards(n)
    r_or, t_or = ob.replay(a_np.ctypes.data, n, T, seed=seed, step_idx0=0, board_offset=0, auto_reset=True)
    assert np.array_equal(r.cpu().numpy().view(np.uint32), r_or.view(np.uint32))
    assert np.array_equal(tm.cpu().numpy().astype(np.uint8), t_or)
    ex = env.export_boards()
    assert np.array_equal(ex["board"].cpu().numpy(), ob.board)
    assert np.array_equal(ex["moves"].cpu().numpy(), ob.moves)
    assert env.step_idx == T

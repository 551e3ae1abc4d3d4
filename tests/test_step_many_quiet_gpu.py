"""step_many(actions) without output buffers (qttt_step_many, out_stride 0): every step but the last runs through
step_quiet_kernel, which stores the planes and neither reward nor terminated.  Bit for bit against the same steps taken
one by one through step_raw: the state after the run, and the returned reward (IEEE bits) and terminated, which are the
last step's — in every launch shape the library picks or is told, with a ragged tail, with actions whose alignment drops
the launch to one board per lane, and with board ids that cross a multiple of 2^32 inside the batch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T_MAX = 7
STEPS = (1, 2, 7)


def _record(n, T, seed, auto_reset, off, explicit_bits):
    """T steps of the uniform-legal policy: actions u8[T,N,2] and (explicit_bits) the collapse bits u8[T,N] they were
    played with."""
    from qtttgym_amd import VecEnv
    rec = VecEnv(n, seed=seed, auto_reset=auto_reset, board_offset=off)
    acts = torch.empty((T, n, 2), dtype=torch.uint8, device="cuda")
    bits = None
    if explicit_bits:
        g = torch.Generator(device="cuda").manual_seed(seed + 17)
        bits = torch.randint(0, 2, (T, n), dtype=torch.uint8, device="cuda", generator=g)
    for t in range(T):
        rec.sample_actions(out=acts[t])
        rec.step_raw(acts[t], None if bits is None else bits[t])
    return acts, bits


def _check(n, auto_reset, explicit_bits, off=0, launch_shape=None, misalign=False, expect_shape=None):
    from qtttgym_amd import VecEnv, _native
    seed = 1000 + n % 977
    acts, bits = _record(n, T_MAX + 1, seed, auto_reset, off, explicit_bits)
    if expect_shape is not None:
        flags = _native.flag_shape(*launch_shape) if launch_shape else 0
        assert _native.step_launch_shape(n, flags) == expect_shape
    for T in STEPS:
        kw = dict(seed=seed, auto_reset=auto_reset, board_offset=off, launch_shape=launch_shape)
        many, single = VecEnv(n, **kw), VecEnv(n, **kw)
        a_many = acts[:T]
        if misalign:
            # the same actions one board (2 bytes) into an allocation: not 4-byte aligned, so two boards per lane
            # (one u32 of actions per lane) are not possible
            buf = torch.empty(T * n * 2 + 2, dtype=torch.uint8, device="cuda")
            a_many = buf[2:].view(T, n, 2)
            a_many.copy_(acts[:T])
            assert a_many.data_ptr() % 4 == 2 and a_many.is_contiguous()
        # what an earlier step would have left behind must not be what is returned
        many._reward.fill_(7.0)
        many._terminated.fill_(True)
        r, tm = many.step_many(a_many, None if bits is None else bits[:T])
        assert r is many._reward and tm is many._terminated and many.step_idx == T
        for t in range(T):
            rs, ts = single.step_raw(acts[t], None if bits is None else bits[t])
        tag = (n, T, auto_reset, explicit_bits, off, launch_shape, misalign)
        assert torch.equal(many.state, single.state), tag
        assert torch.equal(r.view(torch.int32), rs.view(torch.int32)), tag
        assert torch.equal(tm, ts), tag
        # the step index advanced the same: step T + 1, one launch each
        r, tm = many.step_raw(acts[T], None if bits is None else bits[T])
        rs, ts = single.step_raw(acts[T], None if bits is None else bits[T])
        assert torch.equal(many.state, single.state), tag
        assert torch.equal(r.view(torch.int32), rs.view(torch.int32)) and torch.equal(tm, ts), tag


# one batch size per row of auto_tuning() (csrc/qttt_launch.h), and an odd one with a ragged tail
@pytest.mark.parametrize("n,shape", [(4096, (1, 256)), (458752 + 2048, (1, 1024)), (655360, (2, 512)),
                                     (1048576, (2, 1024)), (1572864 + 4096, (2, 256)), (5003, (1, 256))])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_step_many_without_outputs_equals_single_steps(n, shape, auto_reset, explicit_bits):
    _check(n, auto_reset, explicit_bits, expect_shape=shape)


@pytest.mark.parametrize("launch_shape", [(4, 512), (2, 256), (2, 512), (2, 1024), (1, 512)])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_step_many_without_outputs_forced_shapes_with_ragged_tail(launch_shape, auto_reset, explicit_bits):
    """5003 boards: 1250 lanes of four (or 2501 of two) and a tail that runs one board per lane."""
    _check(5003, auto_reset, explicit_bits, launch_shape=launch_shape, expect_shape=launch_shape)


@pytest.mark.parametrize("n,launch_shape", [(5003, None), (5004, (2, 512)), (5004, (4, 512)), (1048576, None)])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_step_many_without_outputs_actions_offset_by_one_board(n, launch_shape, auto_reset, explicit_bits):
    _check(n, auto_reset, explicit_bits, launch_shape=launch_shape, misalign=True)


@pytest.mark.parametrize("launch_shape", [None, (2, 512), (4, 512)])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_step_many_without_outputs_across_2_pow_32(launch_shape, auto_reset, explicit_bits):
    """Board ids cross a multiple of 2^32 inside the batch: the launch is cut there, an odd number of boards in front."""
    _check(5003, auto_reset, explicit_bits, off=(1 << 32) - 2501, launch_shape=launch_shape)
    _check(5003, auto_reset, explicit_bits, off=(3 << 32) - 1000, launch_shape=launch_shape)


@pytest.mark.parametrize("n", [5003, 655360])
@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("explicit_bits", [False, True])
def test_step_many_with_output_buffers_still_fills_every_row(n, auto_reset, explicit_bits):
    from qtttgym_amd import VecEnv
    T, seed = T_MAX, 31
    acts, bits = _record(n, T, seed, auto_reset, 0, explicit_bits)
    many, single = VecEnv(n, seed=seed, auto_reset=auto_reset), VecEnv(n, seed=seed, auto_reset=auto_reset)
    rew = torch.full((T, n), 7.0, dtype=torch.float32, device="cuda")
    term = torch.ones((T, n), dtype=torch.bool, device="cuda")
    r, tm = many.step_many(acts, bits, reward=rew, terminated=term)
    assert r is rew and tm is term and many.step_idx == T
    for t in range(T):
        rs, ts = single.step_raw(acts[t], None if bits is None else bits[t])
        assert torch.equal(rew[t].view(torch.int32), rs.view(torch.int32)) and torch.equal(term[t], ts), (n, t)
    assert torch.equal(many.state, single.state)


def test_step_many_without_outputs_keeps_its_argument_checks():
    """The steps that store no outputs are checked like the ones that do: QTTT_ERR_NULL -1, _SIZE -2, _ACTION -3 as before."""
    from qtttgym_amd import VecEnv, _native
    n, T = 256, 3
    env = VecEnv(n)
    L = _native.lib()
    s = torch.cuda.current_stream().cuda_stream
    a = torch.zeros((T, n, 2), dtype=torch.uint8, device="cuda")
    r = torch.empty(n, dtype=torch.float32, device="cuda")
    tm = torch.empty(n, dtype=torch.bool, device="cuda")
    st = env.state.data_ptr()
    assert L.qttt_step_many(st, a.data_ptr(), None, 1, 0, 0, 0, None, tm.data_ptr(), 0, n, T, s) == -1
    assert L.qttt_step_many(st, a.data_ptr(), None, 1, 0, 0, 0, r.data_ptr(), None, 0, n, T, s) == -1
    assert L.qttt_step_many(None, a.data_ptr(), None, 1, 0, 0, 0, r.data_ptr(), tm.data_ptr(), 0, n, T, s) == -1
    assert L.qttt_step_many(st, None, None, 1, 0, 0, 0, r.data_ptr(), tm.data_ptr(), 0, n, T, s) == -1
    assert L.qttt_step_many(st, a.data_ptr() + 1, None, 1, 0, 0, 0, r.data_ptr(), tm.data_ptr(), 0, n, T - 1, s) == -3
    assert L.qttt_step_many(st, a.data_ptr(), None, 1, 0, -1, 0, r.data_ptr(), tm.data_ptr(), 0, n, T, s) == -2
    torch.cuda.synchronize()
    assert torch.count_nonzero(env.state).item() == 0          # nothing ran

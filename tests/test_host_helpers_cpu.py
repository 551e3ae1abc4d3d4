"""qtttgym_amd/_host.py: the one tensor check, the allocate-or-check helpers for `out=` arguments and the spec tables
they are driven by — on CPU tensors, with the `meta` device standing in for "another device".  Plus the two refusals
that exist to keep a bad address away from a kernel (VecEnv.from_state, VecEnv.step_many), which are checked here only:
provoking them on a device would be the fault they prevent."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CPU = torch.device("cpu")


def _host():
    from qtttgym_amd import _host
    return _host


def _bad_tensors(dtype, shape):
    """A right tensor's neighbours: wrong dtype, wrong shape, right shape but strided, another device."""
    other = torch.int16 if dtype != torch.int16 else torch.int32
    wide = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=dtype)
    return {"dtype": torch.zeros(shape, dtype=other),
            "shape": torch.zeros(shape[:-1] + (shape[-1] + 1,), dtype=dtype),
            "stride": wide[..., ::2],
            "device": torch.zeros(shape, dtype=dtype, device="meta")}


@pytest.mark.parametrize("dtype,shape", [(torch.uint8, (6, 2)), (torch.float32, (3, 6)), (torch.bool, (4,)),
                                         (torch.int64, (5, 2, 3))])
def test_check_tensor_in_shape_mode_and_in_numel_mode(dtype, shape):
    H = _host()
    good = torch.zeros(shape, dtype=dtype)
    assert H.check_tensor(good, dtype, shape, CPU, "x") is good
    assert H.check_tensor(good, dtype, shape, CPU, "x", numel=True) is good
    bad = _bad_tensors(dtype, shape)
    assert bad["stride"].shape == good.shape and not bad["stride"].is_contiguous()
    for numel in (False, True):
        for why, t in bad.items():
            with pytest.raises(ValueError, match="x must be"):
                H.check_tensor(t, dtype, shape, CPU, "x", numel=numel)
    # numel mode takes any contiguous view of as many elements; shape mode takes the shape alone
    flat = good.reshape(-1)
    assert H.check_tensor(flat, dtype, shape, CPU, "x", numel=True) is flat
    with pytest.raises(ValueError):
        H.check_tensor(flat.reshape(1, -1), dtype, shape, CPU, "x")
    with pytest.raises(ValueError):
        H.check_tensor(torch.zeros(flat.numel() + 1, dtype=dtype), dtype, shape, CPU, "x", numel=True)
    # an empty batch is a tensor like any other
    empty = torch.zeros((0,) + shape[1:], dtype=dtype)
    assert H.check_tensor(empty, dtype, (0,) + shape[1:], CPU, "x") is empty


def test_out_tensor_and_out_tensors_allocate_or_check():
    H = _host()
    t = H.out_tensor(torch.int8, (3,), 5, CPU)
    assert t.dtype == torch.int8 and t.shape == (5, 3) and t.device == CPU
    assert H.out_tensor(torch.int8, (3,), 5, CPU, t) is t
    assert H.out_tensor(torch.uint8, (), 0, CPU).shape == (0,)
    with pytest.raises(ValueError, match="out"):
        H.out_tensor(torch.int8, (3,), 4, CPU, t)
    with pytest.raises(ValueError, match="result"):
        H.out_tensor(torch.int8, (2,), 5, CPU, t, "result")
    assert H.out_tensor(torch.int8, (), 15, CPU, t, numel=True) is t
    specs = ((torch.int8, ()), (torch.uint8, (2,)))
    a, b = H.out_tensors(specs, 7, CPU)
    assert (a.dtype, a.shape, b.dtype, b.shape) == (torch.int8, (7,), torch.uint8, (7, 2))
    assert H.out_tensors(specs, 7, CPU, (a, b)) == (a, b) and H.out_tensors(specs, 7, CPU, [a, b])[1] is b
    with pytest.raises(ValueError, match=r"out\[1\]"):
        H.out_tensors(specs, 7, CPU, (a, b[:-1]))
    with pytest.raises(ValueError, match=r"out\[0\]"):
        H.out_tensors(specs, 7, CPU, (a.to(torch.int16), b))
    with pytest.raises(ValueError, match="out"):
        H.out_tensors(specs, 7, CPU, (a,))
    with pytest.raises(ValueError, match=r"out\[1\]"):
        H.out_tensors(specs, 7, CPU, (a, b.to("meta")))


def test_out_rows_with_optional_and_required_keys():
    H = _host()
    spec = {"a": (torch.int8, ()), "b": (torch.float32, (36,)), "c": (torch.int64, (2,))}
    full = H.out_rows(spec, 4, CPU)
    assert list(full) == ["a", "b", "c"]
    assert [(t.dtype, tuple(t.shape)) for t in full.values()] == [(torch.int8, (4,)), (torch.float32, (4, 36)),
                                                                  (torch.int64, (4, 2))]
    assert list(H.out_rows(spec, 4, CPU, keys=("c", "a"))) == ["c", "a"]
    # the caller's dict: returned as it is, every row optional unless required
    assert H.out_rows(spec, 4, CPU, full) is full
    part = {"b": full["b"]}
    assert H.out_rows(spec, 4, CPU, part) is part and list(part) == ["b"]
    assert H.out_rows(spec, 4, CPU, {"a": None, "b": full["b"]})["a"] is None          # None counts as absent
    with pytest.raises(ValueError, match="'c'"):
        H.out_rows(spec, 4, CPU, part, required=("b", "c"))
    with pytest.raises(ValueError, match="'a'"):
        H.out_rows(spec, 4, CPU, {"a": None, "b": full["b"]}, required=("a",))
    assert H.out_rows(spec, 4, CPU, full, required=spec) is full
    # a wrong row is named
    for why, t in _bad_tensors(torch.float32, (4, 36)).items():
        with pytest.raises(ValueError, match=r"out\['b'\]"):
            H.out_rows(spec, 4, CPU, {"a": full["a"], "b": t})
    # what the spec does not know: ignored, or — strict — refused
    extra = dict(full, child0=object())
    assert H.out_rows(spec, 4, CPU, extra) is extra
    with pytest.raises(ValueError, match="child0"):
        H.out_rows(spec, 4, CPU, extra, strict=True)
    # numel mode reaches the rows
    col = {"a": torch.zeros((4, 1), dtype=torch.int8)}
    assert H.out_rows(spec, 4, CPU, col, numel=True) is col
    with pytest.raises(ValueError):
        H.out_rows(spec, 4, CPU, col)


def test_spec_tables_hold_what_the_docstrings_promise():
    from qtttgym_amd import TreeSearch, VecEnv, vec_env
    u8, i8, i16, i32, i64, f32, f64, b = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.float32,
                                          torch.float64, torch.bool)
    assert VecEnv._EXPORT_ROWS == {"moves": (u8, (9, 2)), "n_moves": (u8, ()), "board": (i8, (9,)), "qmask": (i16, (4,)),
                                   "n_q": (u8, ())}
    assert dict((k, (dt, shp)) for k, dt, shp in VecEnv._EXPORT_SPEC) == VecEnv._EXPORT_ROWS
    assert VecEnv._NODE_ROWS == {"winner": (i8, ()), "terminal": (b, ()), "legal": (i64, ()), "state_key": (i64, ()),
                                 "key": (i64, ())}
    assert VecEnv._EXPAND_ROWS == {"n_children": (u8, ()), "winner": (i8, (2,)), "terminal": (b, (2,)),
                                   "legal": (i64, (2,)), "state_key": (i64, (2,)), "key": (i64, (2,))}
    assert VecEnv._expand_rollout_rows(5) == {"value_sum": (i32, (2,)), "result": (i8, (2, 5))}
    assert VecEnv._EVAL_ROWS == {"value": (f32, ()), "logits": (f32, (36,)), "probs": (f32, (36,))}
    assert VecEnv._LEAF_ROWS == {"value": (f32, ()), "probs": (f32, (36,))}
    assert VecEnv._policy_rows(3) == {"result": (i8, (3,)), "plies": (u8, (3,)), "trace": (u8, (3, 9)),
                                      "value": (f32, ()), "probs": (f32, (36,))}
    assert TreeSearch._ROOT_ROWS == {"N": (i32, (36,)), "W": (f64, (36,)), "Q": (f64, (36,)), "P": (f64, (36,)),
                                     "Ntot": (i32, ()), "choose": (u8, ()), "nodes_used": (i32, ()),
                                     "overflow": (u8, ())}
    # the observation (env.py:19-25,68-85) and the eight tensors of a default step(), in the order they are carved
    assert vec_env._OBS_ROWS == {"q_states_p1": (u8, (5, 2)), "q_states_p1_len": (u8, ()), "q_states_p2": (u8, (4, 2)),
                                 "q_states_p2_len": (u8, ()), "classical": (i8, (9,)), "turn": (u8, ())}
    assert list(vec_env._OBS_ROWS) == list(vec_env._OBS_KEYS)
    assert [(f, dt, shp) for _, f, dt, shp in vec_env._OUTPUTS[:2]] == [("reward", f32, ()), ("terminated", b, ())]
    fields = {name for name, _ in __import__("qtttgym_amd")._native.EnvRecord._fields_}
    assert all(f in fields for _, f, _, _ in vec_env._OUTPUTS) and set(vec_env._OBSERVE_ARGS) <= fields
    assert sorted(vec_env._OBSERVE_ARGS) == sorted(f for _, f, _, _ in vec_env._OUTPUTS[2:])
    n = 1000
    t, base = vec_env._carve_py(n, CPU)
    lay = vec_env._layout(n)
    for k, (key, field, dt, shp) in enumerate(vec_env._OUTPUTS):
        assert t[k].dtype == dt and tuple(t[k].shape) == (n,) + shp and t[k].is_contiguous(), key or field
        assert t[k].data_ptr() - base == lay[k]
    assert lay == (0, 4096, 5120, 15360, 16384, 24576, 25600, 34816, 35840)


def test_resolve_device_and_check_net_without_a_device():
    from qtttgym_amd import _native
    H = _host()
    for who in ("VecEnv", "TreeSearch", "PolicyValueNet"):
        with pytest.raises(_native.QtttNativeError, match=who):
            H.resolve_device("cpu", who)
        with pytest.raises(_native.QtttNativeError):
            H.resolve_device(torch.device("meta"), who)
    if not torch.cuda.is_available():
        with pytest.raises(_native.QtttNativeError, match="no HIP device"):
            H.resolve_device("cuda", "VecEnv")

    class Net:
        device, blob = CPU, torch.zeros(16, dtype=torch.uint8)
    H.check_net(Net(), CPU)
    for bad in (object(), type("NoBlob", (), {"device": CPU})(), type("Elsewhere", (Net,), {"device": torch.device("meta")})()):
        with pytest.raises(ValueError, match="PolicyValueNet"):
            H.check_net(bad, CPU)


def test_from_state_refuses_a_state_that_is_not_a_contiguous_cuda_tensor():
    from qtttgym_amd import VecEnv, _native
    n = 8
    nbytes = int(_native.lib().qttt_state_bytes(n))
    for state in (torch.zeros(nbytes, dtype=torch.uint8), torch.zeros(nbytes, dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError, match="state must be a tensor on a cuda device"):
            VecEnv.from_state(state, n)
    # contiguity, dtype and size are tested before the device type, so a CPU tensor shows that they are
    for state in (torch.zeros(2 * nbytes, dtype=torch.uint8)[::2], torch.zeros(nbytes, dtype=torch.int8),
                  torch.zeros(nbytes + 8, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="state must be a contiguous torch.uint8 tensor"):
            VecEnv.from_state(state, n)
    with pytest.raises(ValueError, match="state"):
        VecEnv.from_state([0] * nbytes, n)


def test_step_many_refuses_outputs_on_another_device():
    """reward / terminated [T,N] of the right dtype and shape on ANOTHER device than the boards used to pass
    validation, and their addresses went to the kernel."""
    from qtttgym_amd import VecEnv
    T, n = 3, 4
    launched = []

    class FakeEnv:                       # what step_many reads before the launch
        num_envs = n
        device = CPU
        state = torch.zeros(64, dtype=torch.uint8)
        _kept_outputs = VecEnv._kept_outputs
        _reward, _terminated = torch.zeros(n), torch.zeros(n, dtype=torch.bool)
        seed = step_idx = board_offset = 0
        _flags = staticmethod(lambda: 0)
        _call = staticmethod(lambda name, *args: launched.append(name))
        _advance = staticmethod(lambda k: None)
    env = FakeEnv()
    actions = torch.zeros((T, n, 2), dtype=torch.uint8)
    reward, terminated = torch.zeros((T, n)), torch.zeros((T, n), dtype=torch.bool)
    assert VecEnv.step_many(env, actions, reward=reward, terminated=terminated) == (reward, terminated)
    assert VecEnv.step_many(env, actions)[0] is env._reward and launched == ["qttt_step_many"] * 2
    for kw, name in ((dict(reward=reward.to("meta"), terminated=terminated), "reward"),
                     (dict(reward=reward, terminated=terminated.to("meta")), "terminated"),
                     (dict(reward=reward.t().contiguous().t(), terminated=terminated), "reward"),
                     (dict(reward=reward, terminated=terminated.to(torch.uint8)), "terminated"),
                     (dict(reward=reward[:2], terminated=terminated), "reward")):
        with pytest.raises(ValueError, match=name):
            VecEnv.step_many(env, actions, **kw)
    with pytest.raises(ValueError, match="together"):
        VecEnv.step_many(env, actions, reward=reward)
    with pytest.raises(ValueError, match="actions"):
        VecEnv.step_many(env, actions.to("meta"), reward=reward, terminated=terminated)
    with pytest.raises(ValueError, match="bits"):
        VecEnv.step_many(env, actions, bits=torch.zeros((T, n), dtype=torch.uint8, device="meta"))
    assert launched == ["qttt_step_many"] * 2

"""PolicyValueNet / qttt_evaluate without a device: the blob size, argument validation, state-dict validation, the
packed layout of include/qttt_nn.h, the C header, and the float64 restatement of nn.Model.forward the GPU tests compare with."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from nn_reference64 import KEYS, forward64, golden_state_dict, load_golden, random_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from qtttgym_amd import _native
    return _native.lib()


def test_nn_weights_bytes_is_host_callable_and_matches_the_packer():
    from qtttgym_amd import _native, policy_value
    L = _lib()
    assert L.qttt_nn_weights_bytes(_native.NN_F32) == 761024
    assert L.qttt_nn_weights_bytes(_native.NN_BF16) == 388288
    for bad in (-1, 2, 7):
        assert L.qttt_nn_weights_bytes(bad) == -1
    for dt, p in ((torch.float32, _native.NN_F32), (torch.bfloat16, _native.NN_BF16)):
        assert policy_value.weights_bytes(dt) == L.qttt_nn_weights_bytes(p)
        assert pack_cpu(random_state_dict(1), dt).numel() == L.qttt_nn_weights_bytes(p)


def test_evaluate_validates_arguments_before_touching_the_device():
    L = _lib()
    st, w, out = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)
    E = L.qttt_evaluate
    assert E(st, w, 0, out, None, None, -1, None) == -2                  # n < 0
    assert E(st, w, 2, out, None, None, 4, None) == -2                   # unknown precision
    assert E(st, w, -1, out, None, None, 0, None) == -2
    assert E(None, None, 0, None, None, None, 0, None) == 0              # n == 0: nothing to do
    assert E(None, w, 0, out, None, None, 4, None) == -1                 # null state
    assert E(st, None, 1, out, None, None, 4, None) == -1                # null weights
    assert E(st, w, 0, None, None, None, 4, None) == -1                  # no output at all
    assert E(st, ctypes.c_void_p(0x20008), 0, out, None, None, 4, None) == -3   # weights not 16-byte aligned
    assert E(st, w, 1, None, ctypes.c_void_p(0x30002), None, 4, None) == -3     # logits not 4-byte aligned
    assert E(st, w, 1, None, None, ctypes.c_void_p(0x30001), 4, None) == -3     # probs not 4-byte aligned


def pack_cpu(sd, dtype):
    from qtttgym_amd.policy_value import pack_weights
    return pack_weights(sd, dtype)


@pytest.mark.parametrize("mutate, what", [
    (lambda sd: sd.pop("fc.2.bias"), "missing key"),
    (lambda sd: sd.__setitem__("fc.0.weight", torch.zeros(128, 180)), "width 128"),
    (lambda sd: sd.__setitem__("fc.4.weight", torch.zeros(256, 255)), "wrong shape"),
    (lambda sd: sd.__setitem__("pi_head.1.bias", torch.zeros(36, dtype=torch.int32)), "integer tensor"),
    (lambda sd: sd.__setitem__("V_head.1.bias", [0.0]), "not a tensor"),
])
def test_state_dict_validation(mutate, what):
    from qtttgym_amd import PolicyValueNet
    sd = random_state_dict(2)
    mutate(sd)
    with pytest.raises(ValueError):
        pack_cpu(sd, torch.float32)
    with pytest.raises(ValueError):
        PolicyValueNet(sd, device="cpu")


def test_bad_dtype_and_cpu_device():
    from qtttgym_amd import PolicyValueNet, _native
    with pytest.raises(ValueError):
        pack_cpu(random_state_dict(3), torch.float16)
    with pytest.raises(ValueError):
        PolicyValueNet(random_state_dict(3), device="cpu", dtype=torch.float64)
    with pytest.raises(_native.QtttNativeError):                         # no CPU fallback
        PolicyValueNet(random_state_dict(3), device="cpu")

    class M(torch.nn.Module):                                            # a module is accepted as the source
        def __init__(self):
            super().__init__()
            self.sd = random_state_dict(4)

        def state_dict(self):
            return self.sd
    with pytest.raises(_native.QtttNativeError):
        PolicyValueNet(M(), device="cpu")


def unpack(blob, dtype):
    """Reads the four matrices B_L[k][c] and the biases back with the offset formulas of include/qttt_nn.h."""
    el = 4 if dtype == torch.float32 else 2
    k1 = 180 if dtype == torch.float32 else 192
    dims = [(k1, 256), (256, 256), (256, 256), (256, 48)]
    nelem = sum(k * c for k, c in dims)
    w = blob[:nelem * el].view(dtype).to(torch.float32).numpy()
    bias = blob[nelem * el:].view(torch.float32).numpy()
    assert bias.size == 816
    mats, start = [], 0
    for K, C in dims:
        k = np.arange(K)[:, None]
        c = np.arange(C)[None, :]
        nc = C // 16
        if dtype == torch.float32:
            off = ((k // 4 * nc + c // 16) * 64 + (k % 4) * 16 + c % 16)
        else:
            off = ((k // 32 * nc + c // 16) * 64 + (k % 32 // 8) * 16 + c % 16) * 8 + k % 8
        assert len(np.unique(off)) == K * C and off.max() == K * C - 1
        mats.append(w[start + off])
        start += K * C
    return mats, bias


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_weights_layout_round_trip(dtype):
    sd = random_state_dict(5)
    mats, bias = unpack(pack_cpu(sd, dtype), dtype)
    conv = (lambda t: t.to(torch.float32)) if dtype == torch.float32 else (lambda t: t.to(torch.bfloat16).to(torch.float32))
    w1 = mats[0]
    assert np.array_equal(w1[:180], conv(sd["fc.0.weight"].t()).numpy())
    assert not w1[180:].any()
    assert np.array_equal(mats[1], conv(sd["fc.2.weight"].t()).numpy())
    assert np.array_equal(mats[2], conv(sd["fc.4.weight"].t()).numpy())
    assert np.array_equal(mats[3][:, :36], conv(sd["pi_head.1.weight"].t()).numpy())
    assert np.array_equal(mats[3][:, 36], conv(sd["V_head.1.weight"][0]).numpy())
    assert not mats[3][:, 37:].any()
    want = np.concatenate([sd["fc.0.bias"], sd["fc.2.bias"], sd["fc.4.bias"], sd["pi_head.1.bias"], sd["V_head.1.bias"],
                           np.zeros(11, np.float32)])
    assert np.array_equal(bias, want)                                    # biases stay f32 in both precisions


def test_float64_restatement_reproduces_the_reference_outputs():
    g = load_golden()
    sd = golden_state_dict(g)
    v, lg, p = forward64(sd, torch.from_numpy(g["vector"]))
    ref_lg, ref_p = torch.from_numpy(g["logits"]).double(), torch.from_numpy(g["probs"]).double()
    assert torch.equal(torch.isneginf(lg), torch.isneginf(ref_lg))
    assert torch.equal(torch.isnan(p), torch.isnan(ref_p))
    fin = torch.isfinite(ref_lg)
    assert (lg[fin] - ref_lg[fin]).abs().max() <= 1e-5
    assert (v - torch.from_numpy(g["value"]).double()).abs().max() <= 1e-5
    ok = ~torch.isnan(ref_p)
    assert (p[ok] - ref_p[ok]).abs().max() <= 1e-5
    # the fixture holds what the issue describes: the 260 parents first, 11 of them terminal with every action masked
    allm = torch.isneginf(ref_lg).all(1)
    assert int(allm[:260].sum()) == 11 and int(allm.sum()) > 11
    assert len(g["value"]) >= 800 and sorted(k for k in g if "." not in k) == sorted(g)
    assert {k.replace(".", "_") for k in KEYS} <= set(g)


def _nn_declared():
    text = open(os.path.join(ROOT, "include", "qttt_nn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(qttt_[a-z0-9_]+)\s*\(", text)))


def test_network_header_symbols_are_bound_exported_and_documented():
    """include/qttt_nn.h is the network's part of the ABI: the binding declares exactly its functions, the library
    exports them, qttt.h includes it, and INTEGRATION.md §2's table names them."""
    from qtttgym_amd import _native
    declared = _nn_declared()
    assert declared == ["qttt_evaluate", "qttt_nn_weights_bytes"]
    assert sorted(_native.NN_SIGNATURES) == declared
    assert not set(declared) & set(_native.SIGNATURES)
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
    assert L.qttt_abi_version() == _native.ABI_VERSION == 6
    assert '#include "qttt_nn.h"' in open(os.path.join(ROOT, "include", "qttt.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all("`%s`" % name in doc for name in declared)


def test_network_header_is_plain_c(tmp_path):
    """qttt.h (and through it qttt_nn.h) compiles as C99 with -pedantic, and the precision codes are the binding's."""
    import subprocess
    from qtttgym_amd import _native
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "qttt.h"\n'
                   'int main(void) {\n'
                   '  int64_t (*wb)(int) = qttt_nn_weights_bytes;\n'
                   '  int (*ev)(const void *, const void *, int, float *, float *, float *, int64_t, void *) = qttt_evaluate;\n'
                   '  printf("%d %d %d", QTTT_NN_F32, QTTT_NN_BF16, (wb != NULL) + (ev != NULL));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-Wno-address",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.dirname(_native.LIB_PATH), "-l:libqttt_hip.so",
                           "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out == [_native.NN_F32, _native.NN_BF16, 2]

"""CPU tests of the training step (include/qttt_train.h, qtttgym_amd.train): the header, the binding table, the workspace
plan, unpack_weights as the inverse of pack_weights, the argument checks (which come before any device work) and the
host plan under the host sanitizers as a stand-alone program.  No GPU."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qttt_train.h")
import train_model as M  # noqa: E402
from nn_reference64 import KEYS, random_state_dict  # noqa: E402

ERR_NULL, ERR_SIZE, ERR_ACTION = -1, -2, -3
NAMES = {"qttt_train_workspace_bytes", "qttt_train_gradients", "qttt_train_adam"}
C = M.CHUNK


def test_header_binding_table_and_docs_agree():
    import __graft_entry__ as entry
    from qtttgym_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(qttt_[a-z0-9_]+)\s*\(", text))
    assert names == set(_native.TRAIN_SIGNATURES) == NAMES
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "TRAIN_SIGNATURES"]
    assert not any(names & set(t) for t in others)
    assert HEADER in entry.HEADERS
    for f in ("qttt_train_kernels.h", "qttt_train_host.h"):
        assert os.path.join(ROOT, "qtttgym_amd", "csrc", f) in entry.HEADERS
    assert re.search(r"#define QTTT_TRAIN_CHUNK %d\b" % C, open(HEADER).read())
    assert _native.TRAIN_CHUNK == C and _native.ABI_VERSION == 6
    L = _native.lib()
    assert L.qttt_abi_version() == 6
    for name in NAMES:
        assert getattr(L, name).argtypes == _native.TRAIN_SIGNATURES[name][1]
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "qttt_train_gradients" in open(os.path.join(ROOT, doc)).read(), doc
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integration for n in NAMES)


def test_header_compiles_alone_and_through_qttt_h(tmp_path):
    src = open(os.path.join(ROOT, "include", "qttt.h")).read()
    assert src.index('#include "qttt_replay.h"') < src.index('#include "qttt_train.h"')
    assert "#define QTTT_ABI_VERSION 6" in src
    uses = ('int64_t (*b)(int64_t) = qttt_train_workspace_bytes;\n'
            'int (*g)(const float *, const double *, const uint8_t *, const float *, const uint8_t *, int64_t, const void *,\n'
            ' void *, float *, float *, void *, void *) = qttt_train_gradients;\n'
            'int (*a)(void *, const void *, void *, void *, void *, int64_t, float, float, float, float, float, void *, void *)\n'
            ' = qttt_train_adam;\n'
            'int main(void) { return (b && g && a && QTTT_TRAIN_CHUNK > 0) ? 0 : 1; }\n')
    for k, head in enumerate(("qttt_train.h", "qttt.h")):
        for lang, cc in (("c", os.environ.get("CC", "gcc")), ("c++", os.environ.get("CXX", "g++"))):
            f = tmp_path / ("use%d.%s" % (k, "c" if lang == "c" else "cpp"))
            f.write_text('#include "%s"\n%s' % (head, uses))
            subprocess.check_call([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(f)])


def test_package_exports_the_trainer():
    import qtttgym_amd
    from qtttgym_amd import Trainer, _native
    assert "Trainer" in qtttgym_amd.__all__
    for method in ("gradients", "step", "state_dict", "grad_dict"):
        assert callable(getattr(Trainer, method))
    with pytest.raises(_native.QtttNativeError):
        Trainer(random_state_dict(1), device="cpu")                  # no CPU path


@pytest.mark.parametrize("n", [1, 63, 64, 65, C - 1, C, C + 1, 2 * C + 1])
def test_workspace_bytes_is_the_plan(n):
    from qtttgym_amd import _native
    assert _native.lib().qttt_train_workspace_bytes(n) == M.workspace_bytes(n)


def test_workspace_bytes_rejects_sizes_out_of_range():
    from qtttgym_amd import _native
    L = _native.lib()
    for bad in (0, -1, -2 ** 40, _native.TRAIN_MAX_SAMPLES + 1):
        assert L.qttt_train_workspace_bytes(bad) == -1
    assert L.qttt_train_workspace_bytes(_native.TRAIN_MAX_SAMPLES) == M.workspace_bytes(_native.TRAIN_MAX_SAMPLES)


def _as_bf16(sd):
    return {k: (t.to(torch.bfloat16).float() if k.endswith("weight") else t.clone()) for k, t in sd.items()}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unpack_is_the_inverse_of_pack(dtype):
    from qtttgym_amd.policy_value import SHAPES, pack_weights, unpack_weights, weights_bytes
    sd = {k: torch.randn(shp, generator=torch.Generator().manual_seed(7 + i)) * 0.3 for i, (k, shp) in enumerate(SHAPES.items())}
    blob = pack_weights(sd, dtype)
    back = unpack_weights(blob, dtype)
    want = sd if dtype == torch.float32 else _as_bf16(sd)
    assert set(back) == set(SHAPES) == set(KEYS)
    for k in SHAPES:
        assert back[k].dtype == torch.float32 and tuple(back[k].shape) == SHAPES[k] and back[k].is_contiguous()
        assert torch.equal(back[k].view(torch.int32), want[k].view(torch.int32)), k
    assert torch.equal(pack_weights(back, dtype), blob)
    assert torch.equal(pack_weights(unpack_weights(blob.view(torch.int16), dtype), dtype), blob)     # any view of the bytes
    with pytest.raises(ValueError):
        unpack_weights(blob[:-4], dtype)
    with pytest.raises(ValueError):
        unpack_weights(blob, torch.float16)
    assert blob.numel() == weights_bytes(dtype)


def _gradients(L, n=1, s=0x10000, pi=0x20000, mask=0x30001, v=0x40000, done=0x50001, weights=0x60000, grads=0x70000,
               Lo=0x80000, Jo=0x90000, ws=0xA0000):
    return L.qttt_train_gradients(s, pi, mask, v, done, n, weights, grads, Lo, Jo, ws, None)


def test_gradients_argument_errors_come_before_any_device_work():
    from qtttgym_amd import _native
    L = _native.lib()
    # the size first, whatever the pointers are
    for n in (0, -1, _native.TRAIN_MAX_SAMPLES + 1):
        assert _gradients(L, n=n) == ERR_SIZE
        assert _gradients(L, n=n, s=None, weights=None, ws=None) == ERR_SIZE
        assert _gradients(L, n=n, s=0x10001, weights=0x60001) == ERR_SIZE
    # then a missing pointer, whatever the alignment of the others; L and J are optional
    for k in ("s", "pi", "mask", "v", "done", "weights", "grads", "ws"):
        assert _gradients(L, **{k: None}) == ERR_NULL, k
        assert _gradients(L, **dict({"s": 0x10001, "weights": 0x60004, "ws": 0xA0010}, **{k: None})) == ERR_NULL, k
    # then alignment: weights and grads 16 bytes, the workspace 256, pi 8, s, v, L and J 4; mask and done take any address
    for k, bad in (("weights", 0x60008), ("grads", 0x70004), ("ws", 0xA0080), ("pi", 0x20004), ("s", 0x10002), ("v", 0x40001),
                   ("Lo", 0x80002), ("Jo", 0x90001)):
        assert _gradients(L, **{k: bad}) == ERR_ACTION, k


def _adam(L, weights=0x10000, grads=0x20000, m=0x30000, v2=0x40000, vmax=0x50000, step=1, bf16=None):
    return L.qttt_train_adam(weights, grads, m, v2, vmax, step, 1e-3, 0.9, 0.999, 1e-8, 1e-3, bf16, None)


def test_adam_argument_errors_come_before_any_device_work():
    from qtttgym_amd import _native
    L = _native.lib()
    for step in (0, -1):
        assert _adam(L, step=step) == ERR_SIZE and _adam(L, step=step, weights=None) == ERR_SIZE
        assert _adam(L, step=step, m=0x30001) == ERR_SIZE
    for k in ("weights", "grads", "m", "v2", "vmax"):
        assert _adam(L, **{k: None}) == ERR_NULL, k
        assert _adam(L, bf16=0x60002, **{k: None}) == ERR_NULL, k
    for k, bad in (("weights", 0x10008), ("grads", 0x20004), ("m", 0x30002), ("v2", 0x40001), ("vmax", 0x50008), ("bf16", 0x60008)):
        assert _adam(L, **{k: bad}) == ERR_ACTION, k


def test_host_plan_under_the_host_sanitizers(tmp_path):
    """tools/train_host_check.cpp, a program of its own over qttt_train_host.h, built with ASan + UBSan and run."""
    exe = str(tmp_path / "train_host_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "qtttgym_amd", "csrc"), os.path.join(ROOT, "tools", "train_host_check.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0 and "train_host_check: ok" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr

#!/usr/bin/env python3
"""Is the device code of two builds of libqttt_hip.so the same?   tools/device_code_diff.py PARENT.so CHANGE.so
Unbundles the gfx950 code object of each library and compares the two byte for byte; when they differ (symbols may
merely have moved), compares per symbol: the set of function symbols, every function's disassembly with addresses and
raw bytes stripped, and every kernel's resource figures from the code object's metadata.  Exit status 0 = same."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), check=True, capture_output=True, text=True).stdout


def code_object(lib, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib)
    tool("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co)
    return co


def functions(co):
    """({every function symbol: kernels and their descriptors}, {kernel: [instruction text]})"""
    syms = {ln.split()[-1] for ln in tool("llvm-readelf", "-s", "--wide", co).splitlines() if " FUNC " in ln or ln.endswith(".kd")}
    names = {s for s in syms if not s.endswith(".kd")}
    out, cur = {}, None
    for ln in tool("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1) in names else None
        elif cur is not None and ln.strip():
            cur.append(re.sub(r"\s*//.*$", "", ln).strip())
    assert set(out) == names, sorted(names ^ set(out))[:5]
    return syms, out


def resources(co):
    """{kernel: figures} from the amdhsa.kernels metadata note (a kernel's own keys are indented by four columns)"""
    out, fig = {}, {}
    for ln in tool("llvm-readelf", "--notes", co).splitlines():
        m = re.match(r"^  [ -] (\.\w+):\s*(\S*)$", ln)
        if ln.startswith("  - "):
            fig = {}
        if m and m.group(1) in FIGURES:
            fig[m.group(1)] = int(m.group(2))
        elif m and m.group(1) == ".symbol":
            out[m.group(2)[:-len(".kd")]] = fig
    for k, v in out.items():
        out[k] = tuple(v[f] for f in FIGURES)
    return out


def main(parent, change):
    with tempfile.TemporaryDirectory() as tmp:
        a, b = code_object(parent, tmp, "parent"), code_object(change, tmp, "change")
        if open(a, "rb").read() == open(b, "rb").read():
            print("gfx950 code objects are byte-identical (%d bytes)" % os.path.getsize(a))
            return 0
        print("gfx950 code objects differ as files (%d / %d bytes): per-symbol comparison" % (os.path.getsize(a), os.path.getsize(b)))
        (sa, fa), (sb, fb), ra, rb = functions(a), functions(b), resources(a), resources(b)
    print("function symbols (kernels + kernel descriptors): parent %d, change %d, only in parent %s, only in change %s"
          % (len(sa), len(sb), sorted(sa - sb), sorted(sb - sa)))
    bad = int(sa != sb)
    # acceptable: the literal of a PC-relative address (s_getpc_b64; s_add_u32 lo, lo, LITERAL) of a __constant__ table
    pcrel = re.compile(r"^s_add_u32 (s\d+), \1, 0x[0-9a-f]+$")
    differing = [s for s in sorted(set(fa) & set(fb)) if fa[s] != fb[s]]
    print("kernels whose instruction text differs: %d of %d" % (len(differing), len(set(fa) & set(fb))))
    for s in differing:
        lines = [i for i, (x, y) in enumerate(zip(fa[s], fb[s])) if x != y]
        ok = len(fa[s]) == len(fb[s]) and all(pcrel.match(fa[s][i]) and pcrel.match(fb[s][i]) and
                                              i > 0 and fa[s][i - 1].startswith("s_getpc_b64") for i in lines)
        print("  %s: %d -> %d instructions, %d differing lines: %s"
              % (s, len(fa[s]), len(fb[s]), len(lines), "PC-relative literals only" if ok else "CODE DIFFERS"))
        for i in lines:
            print("    - %s\n    + %s" % (fa[s][i], fb[s][i]))
        bad += not ok
    print("kernels with metadata: parent %d, change %d" % (len(ra), len(rb)))
    moved = [k for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)]
    print("kernels whose (VGPR, AGPR, SGPR, LDS, scratch) differ: %d" % len(moved))
    for k in moved:
        print("  %s: %s -> %s" % (k, ra.get(k), rb.get(k)))
    bad += len(moved) + (not ra)
    print("RESULT: %s" % ("device code is the parent's" if not bad else "DEVICE CODE CHANGED"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

#!/usr/bin/env python3
"""Folds rocprofv3 --pmc counter_collection.csv files (one pass per counter) into
profiles/pmc_traffic.json, keyed by boards per launch.

    python tools/pmc_summary.py BOARDS fetch_dir write_dir [label] [state_bytes_per_board] [extra_bytes_per_board key_suffix]

extra_bytes_per_board / key_suffix: e.g. `30 gym` for the step kernel that also writes the observation.

FETCH_SIZE / WRITE_SIZE are in KiB; on gfx950 FETCH_SIZE reports half the bytes of a wide
coalesced read (MI355X_MICROARCH.md §HBM), so it is doubled.  Only the step kernel's
dispatches are used.

qttt_step_many without output buffers runs every step but its last through step_quiet_kernel (no reward / terminated
stores).  With PMC_REGION="K,W,R" (bench.py's --steps, --warmup and the `regions` of its JSON line) only the TIMED
dispatches are folded — the last R * (W + K) step dispatches of the process are the R regions, the last K of each are
timed, as in tools/trace_summary.py — and the entry is the mean over them, full and quiet dispatches weighted by their
count (K - 1 quiet + 1 full per region), with the two kinds listed beside it.  Without PMC_REGION every dispatch of
either kind is averaged (the recording pass and the warm-up passes included).

Where step_many takes the register-resident route (no output buffers, 448 K < boards <= 1536 K, K >= 16) the timed region
is ceil(K / 256) dispatches of step_fused_kernel (RESIDENT_MAX_PLIES, csrc/qttt_step_kernels.h): with PMC_KERNEL_FILTER=step_fused_kernel and PMC_STEPS=K every dispatch of
that kernel is a timed one (the warm-up of fewer than 16 steps runs launch per step), their bytes are summed per region and
divided by K, so that the entry stays "bytes per step" like the quiet / full one; its algorithmic figure is the action
stream's 2 B per board-step plus one state round trip (2 x state bytes) and the last ply's 5 B per region."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# which dispatches to fold, e.g. PMC_KERNEL_FILTER="false, true>" for the observation-writing step kernel
KERNEL_FILTER = os.environ.get("PMC_KERNEL_FILTER", "step_kernel")


QUIET_FILTER = "step_quiet_kernel"
STEPS = int(os.environ.get("PMC_STEPS", "0"))
RESIDENT_MAX_PLIES = 256                     # csrc/qttt_step_kernels.h: the plies of one output-free launch
REGION = tuple(int(x) for x in os.environ["PMC_REGION"].split(",")) if os.environ.get("PMC_REGION") else None


def mean_counter(d, name):
    """(mean over the folded dispatches, their number, {kind: (mean, number)}) of one counter"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            quiet = KERNEL_FILTER == "step_kernel" and QUIET_FILTER in r["Kernel_Name"]
            if r["Counter_Name"] == name and (quiet or KERNEL_FILTER in r["Kernel_Name"]):
                rows.append((int(r["Dispatch_Id"]), "quiet" if quiet else "full", float(r["Counter_Value"])))
    rows.sort()
    if STEPS:
        per_region = -(-STEPS // RESIDENT_MAX_PLIES)
        n_regions = len(rows) // per_region
        total = sum(x[2] for x in rows[-n_regions * per_region:])
        return total / (n_regions * STEPS), n_regions * per_region, {}
    if REGION:
        K, W, R = REGION
        tail = rows[-R * (W + K):]
        rows = [x for r in range(R) for x in tail[r * (W + K) + W:(r + 1) * (W + K)]]
    if not rows:
        raise SystemExit("no %s rows for step_kernel under %s" % (name, d))
    kinds = {}
    for kind in ("full", "quiet"):
        v = [x[2] for x in rows if x[1] == kind]
        if v:
            kinds[kind] = (sum(v) / len(v), len(v))
    return sum(x[2] for x in rows) / len(rows), len(rows), kinds


STEP_SOURCES = ("qttt_state.h", "qttt_step_core.h", "qttt_observation.h", "qttt_step_kernels.h")


def step_sources_sha256():
    """Fingerprint of the sources the step kernels are made of: bench.py reports whether the committed traffic figure
    was collected on the build it is running (`roofline.traffic_measured_on_this_build`)."""
    import hashlib
    h = hashlib.sha256()
    for f in STEP_SOURCES:
        h.update(open(os.path.join(ROOT, "qtttgym_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def main():
    boards, fetch_dir, write_dir = sys.argv[1], sys.argv[2], sys.argv[3]
    label = sys.argv[4] if len(sys.argv) > 4 else ""
    state_bytes = int(sys.argv[5]) if len(sys.argv) > 5 else 16
    extra = int(sys.argv[6]) if len(sys.argv) > 6 else 0
    suffix = sys.argv[7] if len(sys.argv) > 7 else ""
    fetch_kib, nf, fetch_kinds = mean_counter(fetch_dir, "FETCH_SIZE")
    write_kib, nw, write_kinds = mean_counter(write_dir, "WRITE_SIZE")
    entry = {
        "FETCH_SIZE_KiB_raw": fetch_kib, "WRITE_SIZE_KiB": write_kib,
        "read_bytes": 2 * fetch_kib * 1024, "write_bytes": write_kib * 1024,
        "hbm_bytes_per_launch": 2 * fetch_kib * 1024 + write_kib * 1024,
        "dispatches": [nf, nw], "label": label, "state_bytes_per_board": state_bytes,
        "algorithmic_bytes_per_launch": (2 * state_bytes + 7 + extra) * int(boards),
        "note": "FETCH_SIZE doubled (gfx950 half-count of wide coalesced reads); separate --pmc passes",
        "step_sources_sha256": step_sources_sha256(),
    }
    if "quiet" in fetch_kinds or "quiet" in write_kinds:
        # the two kinds of dispatch beside their count-weighted mean above; the algorithmic figure likewise
        for kind, out_bytes in (("full", 5), ("quiet", 0)):
            if kind in fetch_kinds and kind in write_kinds:
                (fk, fn), (wk, wn) = fetch_kinds[kind], write_kinds[kind]
                entry[kind] = {"FETCH_SIZE_KiB_raw": fk, "WRITE_SIZE_KiB": wk, "dispatches": [fn, wn],
                               "hbm_bytes_per_launch": 2 * fk * 1024 + wk * 1024,
                               "algorithmic_bytes_per_launch": (2 * state_bytes + 2 + out_bytes + extra) * int(boards)}
        if "full" in entry and "quiet" in entry:
            nq, nfl = entry["quiet"]["dispatches"][1], entry["full"]["dispatches"][1]
            entry["algorithmic_bytes_per_launch"] = (nq * entry["quiet"]["algorithmic_bytes_per_launch"] +
                                                     nfl * entry["full"]["algorithmic_bytes_per_launch"]) / (nq + nfl)
    if STEPS:
        entry["resident_route_steps_per_region"] = STEPS
        entry["algorithmic_bytes_per_launch"] = (2 + (2 * state_bytes + 5) / STEPS) * int(boards)
        entry["note"] += "; step_fused_kernel: bytes per STEP of a region of %d steps in %d dispatches" % (STEPS, -(-STEPS // RESIDENT_MAX_PLIES))
    if REGION:
        entry["timed_region_steps_warmup_regions"] = list(REGION)
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    d = json.load(open(path)) if os.path.exists(path) else {}
    d["%s@%dB%s" % (boards, state_bytes, ("+" + suffix) if suffix else "")] = entry
    json.dump(d, open(path, "w"), indent=1, sort_keys=True)
    print(json.dumps(entry))


if __name__ == "__main__":
    main()

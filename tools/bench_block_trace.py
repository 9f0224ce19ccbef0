#!/usr/bin/env python3
"""Run ON THE GPU BOX: what an attached block trace (WebRtcAecmBatch_SetBlockTrace) costs, and that a launch without one costs
what it did before the trace existed.

For every size in --sizes (default 65536x1280 and 4096x2048, streams x blocks) at 16 kHz it records frames/s (blocks of 64 samples
per second of wall time, launch + synchronise) of the equal-length launch of the batch
    (a) parent     the library given with --parent (a build of the parent commit: tools/ab_build.py from a checkout of it, or a
                   copy of its shipped library), untraced
    (b) untraced   this build, no trace attached
    (c) traced     this build, a stream-major trace attached: 32 bytes of record per block on top of its 384 bytes of audio
Every point -- one size on one library -- runs in a child process of its own under a time limit ($AECM_LIB_PATH names the
library); the first child that fails ends the run.  The libraries are interleaved --passes times; the spread of a figure over the
passes and the repetitions inside them is printed next to it: (b) and (a) are called equal when their ranges overlap, (c) / (b) is
reported as measured.  The form each column ran is named through WebRtcAecmBatch_DescribeLaunch.

    python tools/bench_block_trace.py --parent webrtc_aecm_amd/_lib/ab_parent.so [--sizes 65536x1280,4096x2048] [--reps 4] [--passes 2]

--census PARENT_LIB (no GPU needed): the isa_census fingerprints of every kernel of PARENT_LIB against the same kernel of this
build, and the register / scratch / LDS figures of the kernels this build adds.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
FORMS = {0: "one wavefront per stream (rotation variants)", 1: "one wavefront per stream (priority by phase)", 2: "chunk queue", 3: "pipelined"}


def point(S, T, reps, fs, new):
    """One child: one size on the library $AECM_LIB_PATH names (or the shipped one)."""
    import torch

    import webrtc_aecm_amd as aecm
    from bench import synth_on_device
    device = torch.device("cuda", 0)
    far, near = synth_on_device(torch, S, T * 64, 1234, device)
    out = torch.empty_like(near)
    ptrs = (far.data_ptr(), near.data_ptr(), out.data_ptr(), far.shape[1], 64)
    batch = aecm.AecmBatch(S, fs, cng_mode=1, echo_mode=1, device=0)
    trace = torch.empty((S * T * 32,), dtype=torch.uint8, device=device) if new else None
    torch.cuda.synchronize()

    def run(traced):
        def go():
            if traced:
                batch.set_block_trace(trace.data_ptr(), T, 1)
            elif new:
                batch.clear_block_trace()
            batch.process_device(*ptrs, T)
        return go
    runs = {"untraced": run(False), "traced": run(True)} if new else {"parent": run(False)}
    wall = {k: [] for k in runs}
    for go in runs.values():                                              # warm-up: every form once
        go()
    batch.synchronize()
    for _ in range(reps):
        for name, go in runs.items():
            t0 = time.perf_counter()
            go()
            batch.synchronize()
            wall[name].append(time.perf_counter() - t0)
    forms = {}
    for name in runs:
        if new:
            (batch.set_block_trace(trace.data_ptr(), T, 1) if name == "traced" else batch.clear_block_trace())
        form, detail = batch.describe_launch(T)
        forms[name] = f"{FORMS[form]}" + (f", chunks of {detail}" if form == 2 else f", shape {detail:#x}" if form == 3 else "")
    print("RESULT " + json.dumps({"streams": S, "blocks": T, "frames_per_s": {k: [S * T / t for t in wall[k]] for k in runs}, "forms": forms}), flush=True)
    batch.close()


def census(parent):
    from webrtc_aecm_amd import build, isa_census
    old = isa_census.census_of_text(isa_census.disassemble(Path(parent)))
    new = isa_census.census_of_text(isa_census.disassemble(build.LIB))
    same = sorted(k for k in old if k in new and old[k]["fingerprint"] == new[k]["fingerprint"])
    differ = sorted(k for k in old if k not in new or old[k]["fingerprint"] != new[k]["fingerprint"])
    print(f"kernels of the parent library: {len(old)}; with the same isa_census fingerprint in this build: {len(same)}; missing or different: {len(differ)}")
    for k in differ:
        print(f"  DIFFERENT {k}")
    for k in same:
        print(f"  {old[k]['fingerprint']}  {k}")
    print(f"kernels this build adds: {len(set(new) - set(old))}")
    for k in sorted(set(new) - set(old)):
        print(f"  {new[k]['fingerprint']}  {k}")
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536x1280,4096x2048")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--passes", type=int, default=2, help="interleaved passes over the libraries")
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per point (one child process each)")
    ap.add_argument("--parent", help="a library built from the parent commit, for column (a)")
    ap.add_argument("--census", metavar="PARENT_LIB", help="compare kernel fingerprints with PARENT_LIB (no GPU) and exit")
    ap.add_argument("--point", nargs=3, metavar=("STREAMS", "BLOCKS", "VARIANT"), help="(internal) one size on one library in this process")
    a = ap.parse_args()
    if a.census:
        return census(a.census)
    if a.point:
        point(int(a.point[0]), int(a.point[1]), a.reps, a.fs, a.point[2] == "new")
        return 0
    sizes = [tuple(int(v) for v in x.split("x")) for x in a.sizes.split(",")]
    acc = {}
    for _ in range(a.passes):
        for S, T in sizes:
            for variant in (("parent", "new") if a.parent else ("new",)):
                env = dict(os.environ)
                if variant == "parent":
                    env["AECM_LIB_PATH"] = str(Path(a.parent).resolve())
                cmd = [sys.executable, str(Path(__file__).resolve()), "--point", str(S), str(T), variant, "--reps", str(a.reps), "--fs", str(a.fs)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, env=env)
                except subprocess.TimeoutExpired:
                    print(f"{S} x {T}, {variant}: no result within {a.timeout} s; stopping", flush=True)
                    return 2
                line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
                if r.returncode != 0 or line is None:
                    print(f"{S} x {T}, {variant}: child failed with status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                    return 2
                rec = json.loads(line[7:])
                slot = acc.setdefault((S, T), {"f": {}, "forms": {}})
                for k, v in rec["frames_per_s"].items():
                    slot["f"].setdefault(k, []).extend(v)
                slot["forms"].update(rec["forms"])
    print(f"{a.fs} Hz, {a.passes} interleaved passes x {a.reps} repetitions; M frames/s, min .. max over all of them")
    print(f"{'streams x blocks':>16} {'(a) parent':>18} {'(b) untraced':>18} {'(c) traced':>18}  (c)/(b) best  (c)/(b) median  verdict on (b) against (a)")
    for (S, T), slot in sorted(acc.items()):
        f = slot["f"]
        cell = lambda k: f"{min(f[k]) / 1e6:7.1f} ..{max(f[k]) / 1e6:7.1f} " if k in f else f"{'-':>18}"
        med = lambda k: sorted(f[k])[len(f[k]) // 2]
        verdict = "-"
        if "parent" in f:
            verdict = "ranges overlap" if min(f["untraced"]) <= max(f["parent"]) and min(f["parent"]) <= max(f["untraced"]) else "ranges do NOT overlap"
        print(f"{f'{S} x {T}':>16} {cell('parent')} {cell('untraced')} {cell('traced')}  {max(f['traced']) / max(f['untraced']):12.3f}  "
              f"{med('traced') / med('untraced'):14.3f}  {verdict}", flush=True)
    print("launch forms (WebRtcAecmBatch_DescribeLaunch):")
    for (S, T), slot in sorted(acc.items()):
        for k, label in (("parent", "(a)"), ("untraced", "(b)"), ("traced", "(c)")):
            if k in slot["forms"]:
                print(f"{f'{S} x {T}':>16} {label} {slot['forms'][k]}")
    print("traced bytes per frame: 32 B of record on top of 384 B of audio (2 x 128 B in, 128 B out)")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Run ON THE GPU BOX: what the pipelined form of a launch WITH a clean near-end input (WebRtcAecmBatch_SetCleanPipelining) is worth.

For S in --sizes (default 256, 1 024, 2 048, 3 072, 4 096) and T = --blocks (default 2 048) at 16 kHz it records frames/s
(blocks of 64 samples per second of wall time, launch + synchronise) of the equal-length launch of the batch
    (a) parent      the library given with --parent (a build of the parent commit: tools/ab_build.py, or a copy of its shipped
                    library) with a clean input -- one wavefront per stream
    (b) off         this build with a clean input, the switch off
    (c) on          this build with a clean input, the switch on
    (d) no clean    this build without a clean input under the shipped policy (pipelined: for orientation)
Every point -- one size on one library -- runs in a child process of its own under a time limit ($AECM_LIB_PATH names the
library); the first child that fails ends the run.  The libraries are interleaved --passes times; the spread of a figure over
the passes and the repetitions inside them is printed next to it, and (c) is called faster than (b) only when their ranges do
not overlap.  The kernel each column ran is named through WebRtcAecmBatch_DescribeLaunch.

    python tools/bench_clean_pipelined.py --parent webrtc_aecm_amd/_lib/ab_parent.so [--sizes ...] [--blocks 2048] [--reps 4] [--passes 2]
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


def point(S, T, reps, fs, new):
    """One child: one size on the library $AECM_LIB_PATH names (or the shipped one)."""
    import torch

    import webrtc_aecm_amd as aecm
    from bench import synth_on_device
    from webrtc_aecm_amd import isa_census
    device = torch.device("cuda", 0)
    far, near = synth_on_device(torch, S, T * 64, 1234, device)
    clean = (near.to(torch.int32) * 3 // 4).to(torch.int16)              # (webrtc_aecm_amd.synth.synth_clean, on the device)
    out = torch.empty_like(near)
    torch.cuda.synchronize()
    ptrs = (far.data_ptr(), near.data_ptr(), out.data_ptr(), far.shape[1], 64)
    batch = aecm.AecmBatch(S, fs, cng_mode=1, echo_mode=1, device=0)

    def with_clean(on):
        def run():
            if new:
                batch.set_clean_pipelining(on)
            batch.process_device(*ptrs, T, clean.data_ptr())
        return run
    runs = {"off": with_clean(False), "on": with_clean(True), "no_clean": lambda: batch.process_device(*ptrs, T)} if new else {"parent": with_clean(False)}
    wall = {k: [] for k in runs}
    for run in runs.values():                                             # warm-up: every form once
        run()
    batch.synchronize()
    for _ in range(reps):
        for name, run in runs.items():
            t0 = time.perf_counter()
            run()
            batch.synchronize()
            wall[name].append(time.perf_counter() - t0)
    kernels = {}
    for name in runs:
        if new:
            batch.set_clean_pipelining(name == "on")
        has_clean = name != "no_clean"
        form, detail = batch.describe_launch(T, clean=has_clean)
        if form == 3 and detail & 0x2000:
            kernels[name] = isa_census.block_kernel(3, False, detail & ~0x2000)[1].replace("pipelined_kernel", "pipelined_clean_kernel")
        else:
            kernels[name] = isa_census.block_kernel(form, has_clean, detail)[1]
    print("RESULT " + json.dumps({"streams": S, "blocks": T, "frames_per_s": {k: [S * T / t for t in wall[k]] for k in runs}, "kernels": kernels}), flush=True)
    batch.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,2048,3072,4096")
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--passes", type=int, default=2, help="interleaved passes over the libraries")
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per point (one child process each)")
    ap.add_argument("--parent", help="a library built from the parent commit, for column (a)")
    ap.add_argument("--point", nargs=2, metavar=("STREAMS", "VARIANT"), help="(internal) one size on one library in this process")
    a = ap.parse_args()
    if a.point:
        point(int(a.point[0]), a.blocks, a.reps, a.fs, a.point[1] == "new")
        return 0
    sizes = [int(x) for x in a.sizes.split(",")]
    acc = {}
    for _ in range(a.passes):
        for S in sizes:
            for variant in (("parent", "new") if a.parent else ("new",)):
                env = dict(os.environ)
                if variant == "parent":
                    env["AECM_LIB_PATH"] = str(Path(a.parent).resolve())
                cmd = [sys.executable, str(Path(__file__).resolve()), "--point", str(S), variant, "--blocks", str(a.blocks), "--reps", str(a.reps),
                       "--fs", str(a.fs)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, env=env)
                except subprocess.TimeoutExpired:
                    print(f"{S} streams, {variant}: no result within {a.timeout} s; stopping", flush=True)
                    return 2
                line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
                if r.returncode != 0 or line is None:
                    print(f"{S} streams, {variant}: child failed with status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                    return 2
                rec = json.loads(line[7:])
                slot = acc.setdefault(S, {"f": {}, "kernels": {}})
                for k, v in rec["frames_per_s"].items():
                    slot["f"].setdefault(k, []).extend(v)
                slot["kernels"].update(rec["kernels"])
    print(f"T = {a.blocks} blocks at {a.fs} Hz, {a.passes} interleaved passes x {a.reps} repetitions; M frames/s, min .. max over all of them")
    print(f"{'streams':>7} {'(a) parent, clean':>18} {'(b) off, clean':>18} {'(c) on, clean':>18} {'(d) no clean':>18}  (c)/(b) best  verdict")
    for S, slot in sorted(acc.items()):
        f = slot["f"]
        cell = lambda k: f"{min(f[k]) / 1e6:7.1f} ..{max(f[k]) / 1e6:7.1f} " if k in f else f"{'-':>18}"
        verdict = "on > off" if min(f["on"]) > max(f["off"]) else "on < off" if max(f["on"]) < min(f["off"]) else "on within the spread of off"
        if "parent" in f:
            verdict += "; off = parent" if min(f["off"]) <= max(f["parent"]) and min(f["parent"]) <= max(f["off"]) else "; off != parent"
        print(f"{S:7d} {cell('parent')} {cell('off')} {cell('on')} {cell('no_clean')}  {max(f['on']) / max(f['off']):11.2f}  {verdict}", flush=True)
    print("kernels (WebRtcAecmBatch_DescribeLaunch):")
    for S, slot in sorted(acc.items()):
        for k, label in (("parent", "(a)"), ("off", "(b)"), ("on", "(c)"), ("no_clean", "(d)")):
            if k in slot["kernels"]:
                print(f"{S:7d} {label} {slot['kernels'][k]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

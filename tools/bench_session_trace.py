#!/usr/bin/env python3
"""Run ON THE GPU BOX: what an attached session trace (WebRtcAecmSessions_SetSessionTrace) costs per tick, and that a tick without
one costs what it did before the trace existed.

For every object size in --sessions (default 65536 and 4096) at 16 kHz, ticks of 160 samples through WebRtcAecmSessions_Tick (the
dense tick: planning launch + tick launch, launch + synchronise), it records ms per tick of
    (a) parent     the library given with --parent (a build of the parent commit), untraced
    (b) untraced   this build, no trace attached
    (c) traced     this build, a trace of one record per session attached (ring_ticks = 1): 64 bytes of record per session and tick
Every point -- one column at one size -- runs in a child process of its own under a time limit ($AECM_LIB_PATH names the
library), all by the same loop: a warm-up that takes the sessions out of their start-up phase, then --ticks timed ticks; the first
child that fails ends the run.  The columns are interleaved --passes times, in rotating order.  The spread of a figure over the passes is printed
next to it: (b) and (a) are called equal when their ranges overlap, (c) / (b) is reported as measured.

    python tools/bench_session_trace.py --parent webrtc_aecm_amd/_lib/ab_parent.so [--sessions 65536,4096] [--ticks 1000] [--passes 3]

--census PARENT_LIB (no GPU needed): the isa_census fingerprints of every kernel of PARENT_LIB against the same kernel of this
build, and the kernels this build adds.
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


def point(S, ticks, warmup, fs, column):
    """One child: one column at one size, on the library $AECM_LIB_PATH names (or the shipped one).  Every column runs this same
    loop, so that the columns differ in nothing but the library and the trace."""
    import torch

    import webrtc_aecm_amd as aecm
    from bench import synth_on_device
    device = torch.device("cuda", 0)
    n = 160
    far, near = synth_on_device(torch, S, 8 * n, 1234, device)
    out = torch.empty_like(near)                 # rows of the inputs' stride: the tick takes ONE stream stride for far, near and out
    sb = aecm.AecmSessions(S, fs, 1, 3)
    if column == "traced":
        trace = torch.empty((S * 64,), dtype=torch.uint8, device=device)
        assert sb.set_session_trace(trace.data_ptr(), 1, 1, 1) == 0
    torch.cuda.synchronize()

    def tick(k):
        off = (k % 8) * n * 2
        rc = sb.tick_device(far.data_ptr() + off, near.data_ptr() + off, out.data_ptr() + off, far.shape[1], n, 40)
        assert rc == 0, rc
    for k in range(warmup):                      # (takes the sessions out of their start-up phase, too)
        tick(k)
    ms = []
    for k in range(ticks):
        t0 = time.perf_counter()
        tick(k)                                  # WebRtcAecmSessions_Tick returns when the tick has run
        ms.append((time.perf_counter() - t0) * 1e3)
    if column == "traced":
        assert sb.session_trace_ticks() == warmup + ticks
    print("RESULT " + json.dumps({"sessions": S, "column": column, "ms_per_tick": sorted(ms)[len(ms) // 2], "window_s": sum(ms) / 1e3}), flush=True)
    sb.close()


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
        print(f"  {old[k]['fingerprint']}  {old[k]['n_instructions']:6d}  {k}")
    print(f"kernels this build adds: {len(set(new) - set(old))}")
    for k in sorted(set(new) - set(old)):
        print(f"  {new[k]['fingerprint']}  {new[k]['n_instructions']:6d}  {k}")
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="65536,4096")
    ap.add_argument("--ticks", type=int, default=1000, help="timed ticks per child")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--passes", type=int, default=3, help="interleaved passes over the libraries")
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per point (one child process each)")
    ap.add_argument("--parent", help="a library built from the parent commit, for column (a)")
    ap.add_argument("--census", metavar="PARENT_LIB", help="compare kernel fingerprints with PARENT_LIB (no GPU) and exit")
    ap.add_argument("--point", nargs=2, metavar=("SESSIONS", "COLUMN"), help="(internal) one column at one size in this process")
    a = ap.parse_args()
    if a.census:
        return census(a.census)
    if a.point:
        point(int(a.point[0]), a.ticks, a.warmup, a.fs, a.point[1])
        return 0
    acc = {}
    columns = ("parent", "untraced", "traced") if a.parent else ("untraced", "traced")
    for k in range(a.passes):
        for S in (int(x) for x in a.sessions.split(",")):
            for variant in columns[k % len(columns):] + columns[:k % len(columns)]:      # every column runs first, second and last in turn
                env = dict(os.environ)
                if variant == "parent":
                    env["AECM_LIB_PATH"] = str(Path(a.parent).resolve())
                cmd = [sys.executable, str(Path(__file__).resolve()), "--point", str(S), variant, "--ticks", str(a.ticks), "--warmup", str(a.warmup),
                       "--fs", str(a.fs)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, env=env)
                except subprocess.TimeoutExpired:
                    print(f"{S} sessions, {variant}: no result within {a.timeout} s; stopping", flush=True)
                    return 2
                line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
                if r.returncode != 0 or line is None:
                    print(f"{S} sessions, {variant}: child failed with status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                    return 2
                acc.setdefault(S, {}).setdefault(variant, []).append(json.loads(line[7:])["ms_per_tick"])
    print(f"{a.fs} Hz, ticks of 160 samples, {a.passes} interleaved passes; ms per tick: the median of {a.ticks} ticks per pass, min .. max over the passes")
    print(f"{'sessions':>9} {'(a) parent':>20} {'(b) untraced':>20} {'(c) traced':>20}  (c)/(b) median  verdict on (b) against (a)")
    for S, f in sorted(acc.items(), reverse=True):
        cell = lambda k: f"{min(f[k]):8.4f} ..{max(f[k]):8.4f} " if k in f else f"{'-':>20}"
        med = lambda k: sorted(f[k])[len(f[k]) // 2]
        verdict = "-"
        if "parent" in f:
            verdict = "ranges overlap" if min(f["untraced"]) <= max(f["parent"]) and min(f["parent"]) <= max(f["untraced"]) else "ranges do NOT overlap"
        print(f"{S:>9} {cell('parent')} {cell('untraced')} {cell('traced')}  {med('traced') / med('untraced'):14.3f}  {verdict}", flush=True)
    print("traced bytes per session and tick: 64 B of record on top of 960 B of audio (2 x 320 B in, 320 B out)")
    return 0


if __name__ == "__main__":
    sys.exit(main())

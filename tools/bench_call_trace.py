#!/usr/bin/env python3
"""Run ON THE GPU BOX: what an attached call trace (WebRtcAecmSessions_SetCallTrace) costs a K-call or packet tick.

For every object size in --sessions (default 65536 and 4096), every K in --calls (default 2,3,6) and two workloads --
    calls     a 16 kHz object, ticks of K calls of 160 samples (WebRtcAecmSessions_TickCalls)
    packets   a 16 kHz object in which half of the sessions (a fixed, seeded set) are 8 kHz sessions that make half calls
              (AECM_SESSION_HALF_CALL), ticks of K calls (WebRtcAecmSessions_TickPackets): the mix of profiles/r20_tick_packets.txt
-- it records ms per tick of K call pairs, launch + synchronise per tick (the Device form of either entry point), of
    (a) parent       the library given with --parent (a build of the parent commit): the untraced K-call / packet tick
    (b) parent-K     that library: K ordinary ticks (WebRtcAecmSessions_TickFlags) under SetSessionTrace, each launched and
                     synchronised -- the only way the parent observes those calls; the time is that of all K
    (c) untraced     this build, no trace attached
    (d) call-traced  this build, a call trace of K records per session attached (ring_calls = K): 64 bytes per session and call
Every point -- one column, one workload, one K at one size -- runs in a child process of its own under a time limit
($AECM_LIB_PATH names the library), all by the same loop: a warm-up of at least 40 calls that takes the sessions out of their
start-up phase, then --ticks timed ticks; the first child that fails ends the run.  The columns are interleaved --passes times, in
rotating order; the spread of a figure over the passes is printed next to it.

    python tools/bench_call_trace.py --parent webrtc_aecm_amd/_lib/ab_parent.so [--sessions 65536,4096] [--calls 2,3,6] [--ticks 400]

--static PARENT_LIB (no GPU needed): the isa_census fingerprints of every kernel of PARENT_LIB against the same kernel of this
build, and registers, LDS, scratch and spills of the kernels this build adds next to those of the kernels they twin.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
COLUMNS = ("parent", "parent-K", "untraced", "call-traced")


def point(S, K, workload, ticks, column):
    """One child: one column of one workload, on the library $AECM_LIB_PATH names (or the shipped one)."""
    import numpy as np
    import torch

    import webrtc_aecm_amd as aecm
    fs, n = 16000, 160
    width = 2 * K * n                                   # two ticks of K calls per row
    g = torch.Generator(device="cuda").manual_seed(1)
    far = (torch.randn((S, width), generator=g, device="cuda") * 3000).clamp_(-32768, 32767).to(torch.int16)
    near = (far.roll(37, dims=1) // 3 + (torch.randn((S, width), generator=g, device="cuda") * 200).to(torch.int16))
    out = torch.empty_like(far)
    ms = np.full(S, 40, dtype=np.int16)
    rates = flags = None
    if workload == "packets":
        narrow = np.zeros(S, dtype=bool)
        narrow[np.random.default_rng(7).permutation(S)[:S // 2]] = True
        rates = np.where(narrow, 8000, 16000).astype(np.int32)
        flags = np.where(narrow, aecm.ffi.SESSION_HALF_CALL, 0).astype(np.uint8)
    sb = aecm.AecmSessions(S, fs, 1, 1, rates=rates)
    if column == "call-traced":
        trace = torch.empty((S * K * 64,), dtype=torch.uint8, device="cuda")
        assert sb.set_call_trace(trace.data_ptr(), K, 1, K) == 0
    elif column == "parent-K":
        trace = torch.empty((S * K * 64,), dtype=torch.uint8, device="cuda")
        assert sb.set_session_trace(trace.data_ptr(), K, 1, K) == 0
    torch.cuda.synchronize()
    fn = sb.tick_packets_device if workload == "packets" else sb.tick_calls_device
    zeros = np.zeros(S, dtype=np.uint8)

    def tick(i):
        off = (i % 2) * K * n * 2
        if column == "parent-K":                         # K ordinary ticks; a half-call session's calls lie 160 samples apart here
            for c in range(K):
                o = off + c * n * 2
                rc, _ = sb.tick_device_flags(far.data_ptr() + o, near.data_ptr() + o, out.data_ptr() + o, width, n, ms, zeros if flags is None else flags)
                assert rc == 0, rc
        else:
            rc, _ = fn(far.data_ptr() + off, near.data_ptr() + off, out.data_ptr() + off, width, n, K, ms, flags=flags)
            assert rc == 0, rc
    warm = -(-40 // K)
    for i in range(warm):
        tick(i)
    t = []
    for i in range(ticks):
        t0 = time.perf_counter()
        tick(warm + i)                                   # every entry point used here returns when the tick has run
        t.append((time.perf_counter() - t0) * 1e3)
    if column == "call-traced":
        assert sb.call_trace_calls() == (warm + ticks) * K
    print("RESULT " + json.dumps({"sessions": S, "calls": K, "workload": workload, "column": column, "ms_per_tick": sorted(t)[len(t) // 2]}), flush=True)
    sb.close()


def metadata(lib):
    """{kernel: registers, LDS, scratch, spills} from the code object's notes."""
    from webrtc_aecm_amd import isa_census
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = Path(tmp) / Path(lib).name
        copy.write_bytes(Path(lib).read_bytes())
        subprocess.run([isa_census._tool("llvm-objdump"), "--offloading", str(copy)], check=True, capture_output=True)
        meta = ""
        for obj in sorted(Path(tmp).glob(copy.name + ".*amdgcn*gfx950*")):
            meta += subprocess.run([isa_census._tool("llvm-readelf"), "--notes", str(obj)], check=True, capture_output=True, text=True).stdout
    fields = ("sgpr_count", "vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")
    for block in re.split(r"\n\s*- \.agpr_count:", meta)[1:]:
        out[re.search(r"\.name:\s+(\S+)", block).group(1)] = {f: int(re.search(rf"\.{f}:\s+(\d+)", block).group(1)) for f in fields}
    return out


def static(parent):
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
    added = sorted(set(new) - set(old))
    print(f"kernels this build adds: {len(added)}")
    meta = metadata(build.LIB)
    twins = {"aecm_calls_traced_tick_kernel": "aecm_tick_calls_kernel", "aecm_packets_traced_tick_kernel": "aecm_tick_packets_kernel",
             "aecm_plan_calls_traced_kernel": "aecm_flow_plan_calls_kernel", "aecm_plan_packets_traced_kernel": "aecm_flow_plan_packets_kernel"}
    print(f"  {'kernel':<44} {'VGPRs':>5} {'SGPRs':>5} {'LDS B':>6} {'scratch B':>9} {'SGPR spills':>11} {'VGPR spills':>11} {'instr.':>7} "
          f"{'VMEM':>5} {'SMEM':>5}  fingerprint")

    def row(k):
        m, c = meta[k], new[k]
        short = re.sub(r"^_ZN4aecm\d+", "", k)
        short = re.sub(r"ILb([01])EEE.*", lambda x: f"<clean = {x.group(1)}>", short)
        short = re.sub(r"ENS_.*", "", short)
        print(f"  {short:<44} {m['vgpr_count']:>5} {m['sgpr_count']:>5} {m['group_segment_fixed_size']:>6} {m['private_segment_fixed_size']:>9} "
              f"{m['sgpr_spill_count']:>11} {m['vgpr_spill_count']:>11} {c['n_instructions']:>7} {c['counts']['VMEM']:>5} {c['counts']['SMEM']:>5}  {c['fingerprint']}")
    for k in added:
        row(k)
        name = next(n for n in twins if n in k)
        inst = re.search(r"ILb[01]EEE", k)
        for o in sorted(new):
            if twins[name] in o and (inst is None or inst.group(0) in o):
                row(o)
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="65536,4096")
    ap.add_argument("--calls", default="2,3,6")
    ap.add_argument("--workloads", default="calls,packets")
    ap.add_argument("--ticks", type=int, default=400, help="timed ticks per child")
    ap.add_argument("--passes", type=int, default=3, help="interleaved passes over the columns")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per point (one child process each)")
    ap.add_argument("--parent", help="a library built from the parent commit, for columns (a) and (b)")
    ap.add_argument("--static", metavar="PARENT_LIB", help="compare kernel fingerprints with PARENT_LIB, list the new kernels' resources (no GPU) and exit")
    ap.add_argument("--point", nargs=4, metavar=("SESSIONS", "CALLS", "WORKLOAD", "COLUMN"), help="(internal) one point in this process")
    a = ap.parse_args()
    if a.static:
        return static(a.static)
    if a.point:
        point(int(a.point[0]), int(a.point[1]), a.point[2], a.ticks, a.point[3])
        return 0
    acc = {}
    columns = COLUMNS if a.parent else COLUMNS[2:]
    for k in range(a.passes):
        for S in (int(x) for x in a.sessions.split(",")):
            for workload in a.workloads.split(","):
                for K in (int(x) for x in a.calls.split(",")):
                    for column in columns[k % len(columns):] + columns[:k % len(columns)]:      # every column runs first and last in turn
                        env = dict(os.environ)
                        if column.startswith("parent"):
                            env["AECM_LIB_PATH"] = str(Path(a.parent).resolve())
                        cmd = [sys.executable, str(Path(__file__).resolve()), "--point", str(S), str(K), workload, column, "--ticks", str(a.ticks)]
                        try:
                            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, env=env)
                        except subprocess.TimeoutExpired:
                            print(f"{S} sessions, {workload}, K = {K}, {column}: no result within {a.timeout} s; stopping", flush=True)
                            return 2
                        line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
                        if r.returncode != 0 or line is None:
                            print(f"{S} sessions, {workload}, K = {K}, {column}: child failed with status {r.returncode}; stopping\n{r.stdout[-2000:]}\n"
                                  f"{r.stderr[-2000:]}", flush=True)
                            return 2
                        acc.setdefault((S, workload, K), {}).setdefault(column, []).append(json.loads(line[7:])["ms_per_tick"])
    print(f"16 kHz objects, ticks of K calls of 160 samples (packets: half of the sessions 8 kHz on half calls), Device forms, launch + synchronise per tick;")
    print(f"ms per tick of K call pairs: the median of {a.ticks} ticks per pass, min .. max over {a.passes} interleaved passes")
    print(f"{'sessions':>9} {'workload':>8} {'K':>2} {'(a) parent':>19} {'(b) parent, K ticks':>19} {'(c) untraced':>19} {'(d) call-traced':>19}  (d)/(a)  (d)/(b)  (d)/(c)")
    for (S, workload, K), f in sorted(acc.items(), key=lambda x: (-x[0][0], x[0][1], x[0][2])):
        cell = lambda c: f"{min(f[c]):8.4f} ..{max(f[c]):8.4f}" if c in f else f"{'-':>19}"
        med = lambda c: sorted(f[c])[len(f[c]) // 2]
        ratio = lambda c: f"{med('call-traced') / med(c):7.3f}" if c in f else f"{'-':>7}"
        print(f"{S:>9} {workload:>8} {K:>2} {cell('parent')} {cell('parent-K')} {cell('untraced')} {cell('call-traced')}  {ratio('parent')}  {ratio('parent-K')}  "
              f"{ratio('untraced')}", flush=True)
    print("traced bytes per session and call: 64 B of record on top of 960 B of audio (2 x 320 B in, 320 B out; 480 B for a half call)")
    return 0


if __name__ == "__main__":
    sys.exit(main())

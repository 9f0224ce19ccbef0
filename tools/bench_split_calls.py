#!/usr/bin/env python3
"""K-call ticks with a clean near-end input per session (WebRtcAecmSessions_SetSplitCallTicks), measured ON THE GPU BOX.  Rows for
profiles/r33_split_calls.txt.

For each object size (--streams, default 65536,4096), each K (--calls, default 2,3,6) and each share P of the sessions flagged
AECM_SESSION_NO_CLEAN (--shares, default 25,50,75 per cent; a fixed, seeded random set): device-resident audio, one PACKET of K calls
of 10 ms per session and step, per-session msInSndCardBuf and flags and a clean plane, packets enqueued back to back, one
synchronisation per window.  Every variant is an object of its own that has left its start-up phase under its own flags; the windows
of all variants of one K are interleaved, --repeats rounds, the median is reported and every window is listed.  Variants:
  ordinary_P     baseline (a): K back-to-back ordinary split ticks (WebRtcAecmSessions_TickAsync) of a twin object with the same flags
                 on the same rows -- what a server with both kinds of leg does per packet without the switch
  clean_live     baseline (b): the all-clean K-call tick (WebRtcAecmSessions_TickCallsAsync, nobody flagged; a K-call tick always goes
                 by the live list)
  split_calls_P  WebRtcAecmSessions_TickCallsAsync with the switch on and P per cent of the sessions flagged
The yardstick: split_calls_50 against ordinary_50 and that baseline's own spread (max - min of its windows) at 65 536 sessions.  After
the last window the outputs of split_calls_P and ordinary_P, which have made the same calls, are compared and must be equal.
--resources needs no GPU: registers and scratch of the six new kernels next to their siblings', from the built library.
--quick: one size, K = 2, P = 50 only, one short window per variant."""
import argparse
import json
import re
import subprocess
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

PAIRS = [("aecm_tick_split_calls_kernelILb1E", "aecm_tick_calls_kernelILb1E"), ("aecm_tick_split_calls_kernelILb0E", "aecm_tick_calls_kernelILb0E"),
         ("aecm_tick_split_packets_kernelILb1E", "aecm_tick_packets_kernelILb1E"), ("aecm_tick_split_packets_kernelILb0E", "aecm_tick_packets_kernelILb0E"),
         ("aecm_flow_plan_split_calls_kernelE", "aecm_flow_plan_calls_kernelE"), ("aecm_flow_plan_split_packets_kernelE", "aecm_flow_plan_packets_kernelE")]


def resources():
    """The build's resource report: (sgpr, vgpr, scratch bytes) of each new kernel and of the kernel whose text it shares."""
    from webrtc_aecm_amd import build, isa_census
    with tempfile.TemporaryDirectory() as tmp:
        lib = Path(tmp) / build.LIB.name
        lib.write_bytes(build.build().read_bytes())
        subprocess.run([isa_census._tool("llvm-objdump"), "--offloading", str(lib)], check=True, capture_output=True)
        meta = ""
        for obj in sorted(Path(tmp).glob(lib.name + ".*amdgcn*gfx950*")):
            meta += subprocess.run([isa_census._tool("llvm-readelf"), "--notes", str(obj)], check=True, capture_output=True, text=True).stdout
    found = {}
    for block in re.split(r"\n\s*- \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        found[name] = tuple(int(re.search(rf"\.{f}:\s+(\d+)", block).group(1)) for f in ("sgpr_count", "vgpr_count", "private_segment_fixed_size"))
    for ours, sibling in PAIRS:
        (a, va), = [(k, v) for k, v in found.items() if ours in k]
        (b, vb), = [(k, v) for k, v in found.items() if sibling in k]
        print(json.dumps({"kernel": a, "sgpr_vgpr_scratch": va, "sibling": b, "sibling_sgpr_vgpr_scratch": vb}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="65536,4096")
    ap.add_argument("--calls", default="2,3,6")
    ap.add_argument("--shares", default="25,50,75")
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--window-ms", type=float, default=200.0, help="device work per timed window, roughly: the packets per window are sized by it")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.resources:
        return resources()
    import numpy as np
    import torch

    import webrtc_aecm_amd as aecm
    if not torch.cuda.is_available():
        raise SystemExit("bench_split_calls.py measures on the GPU; no device found")
    NO_CLEAN = aecm.ffi.SESSION_NO_CLEAN
    fs, n = args.fs, args.fs // 100
    shares = [50] if args.quick else [int(x) for x in args.shares.split(",")]
    sizes = [int(x) for x in args.streams.split(",")][:1 if args.quick else None]
    ks = [2] if args.quick else [int(x) for x in args.calls.split(",")]
    for S in sizes:
        ms = np.full(S, 40, dtype=np.int16)
        order = np.random.default_rng(7).permutation(S)
        for K in ks:
            span, period = K * n, 2                      # rows of two packets, used in turn
            g = torch.Generator(device="cuda").manual_seed(1)
            far = (torch.randn((S, span * period), generator=g, device="cuda") * 3000).clamp_(-32768, 32767).to(torch.int16)
            near = (far.roll(37, dims=1) // 3 + (torch.randn((S, span * period), generator=g, device="cuda") * 200).to(torch.int16))
            clean = (near - (torch.randn((S, span * period), generator=g, device="cuda") * 100).to(torch.int16))
            stride = far.shape[1]

            class Variant:
                def __init__(self, name, flags, as_calls, switch=False):
                    self.name, self.flags, self.as_calls = name, flags, as_calls
                    self.sess = aecm.AecmSessions(S, fs, 1, 1)
                    if switch:
                        assert self.sess.set_split_call_ticks(True) == 0
                    self.out = torch.zeros_like(far)
                    self.i = 0
                    self.times = []

                def packets(self, count):
                    for _ in range(count):
                        off = (self.i % period) * span * 2
                        if self.as_calls:
                            rc, _ = self.sess.tick_calls_device(far.data_ptr() + off, near.data_ptr() + off, self.out.data_ptr() + off, stride, n, K, ms,
                                                                clean_ptr=clean.data_ptr() + off, flags=self.flags, asynchronous=True)
                            assert rc == 0, (self.name, rc)
                        else:
                            for c in range(K):
                                at = off + c * n * 2
                                rc = self.sess.tick_async(far.data_ptr() + at, near.data_ptr() + at, self.out.data_ptr() + at, stride, n, 40,
                                                          clean_ptr=clean.data_ptr() + at, ms_per_session=ms, flags=self.flags)
                                assert rc == 0, (self.name, rc)
                        self.i += 1

                def window(self, count):
                    assert self.sess.synchronize() == 0
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    self.packets(count)
                    assert self.sess.synchronize() == 0
                    self.times.append((time.perf_counter() - t0) / count * 1e3)

            none = np.zeros(S, dtype=np.uint8)
            variants = [Variant("clean_live", none, True)]
            for p in shares:
                flags = none.copy()
                flags[order[:(S * p + 50) // 100]] = NO_CLEAN
                variants.append(Variant(f"ordinary_{p}", flags, False))
                variants.append(Variant(f"split_calls_{p}", flags, True, switch=True))
            for v in variants:                                   # through the start-up phase, and every launch shape warmed up
                v.packets(-(-48 // K))
                assert v.sess.synchronize() == 0
            variants[0].window(20)
            per_packet = variants[0].times.pop()
            count = 40 if args.quick else max(20, int(args.window_ms / max(per_packet, 1e-3)))
            for r in range(1 if args.quick else args.repeats):
                for v in variants:
                    v.window(count)
            by_name = {v.name: v for v in variants}
            for p in shares:
                a, b = by_name[f"split_calls_{p}"], by_name[f"ordinary_{p}"]
                assert a.i == b.i and torch.equal(a.out, b.out), ("the K-call split tick and K ordinary split ticks differ", S, K, p)
            live = by_name["clean_live"].times
            rows = []
            for v in variants:
                row = {"variant": v.name, "flagged": int(((v.flags & NO_CLEAN) != 0).sum()), "ms_per_packet": float(np.median(v.times)),
                       "vs_clean_live": float(np.median(v.times) / np.median(live)), "all_ms_per_packet": v.times}
                if v.name.startswith("split_calls_"):
                    base = by_name["ordinary_" + v.name.rsplit("_", 1)[1]].times
                    row["vs_ordinary"] = float(np.median(v.times) / np.median(base))
                    row["ordinary_spread_ms"] = max(base) - min(base)
                    row["gain_ms"] = float(np.median(base) - np.median(v.times))
                rows.append(row)
            line = {"streams": S, "calls": K, "fs": fs, "audio": "device", "async": True, "packets_per_window": count, "windows": len(live), "rows": rows}
            text = json.dumps(line)
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(text + "\n")
            for v in variants:
                v.sess.close()
            del variants, by_name, far, near, clean
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

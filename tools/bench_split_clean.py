#!/usr/bin/env python3
"""Split ticks (AECM_SESSION_NO_CLEAN: a clean near-end input per session), measured ON THE GPU BOX.  Rows for
profiles/r24_split_clean_ticks.txt.

For each object size (--streams, default 65536,4096) and each share P of the sessions flagged AECM_SESSION_NO_CLEAN (--shares,
default 0,25,50,75,100 per cent; a fixed, seeded random set): device-resident audio, WebRtcAecmSessions_TickAsync with per-session
msInSndCardBuf and flags and a clean plane, ticks enqueued back to back, one synchronisation per window.  Every variant is an object
of its own that has left its start-up phase under its own flags; the windows of all variants are interleaved, --repeats rounds, the
median is reported and every window is listed.  Variants:
  clean_live     baseline: the all-clean tick of the same object size sent through the live list (WebRtcAecmSessions_ForceSparseTicks)
                 with the arrays the split rows pass, flags that name nothing
  noclean_live   baseline: the same without a clean plane
  split_P        P per cent of the sessions flagged, as the library ticks it (P = 0: nobody flagged, today's tick; P = 100: everybody,
                 the launches of the tick without a clean input -- neither goes through the live list)
  split_P_fused  the same with the tick launch forced to the fused kernel (WebRtcAecmSessions_SplitCleanTwoLaunches(0))
  split_P_two    ... and forced to two launches, one per list (WebRtcAecmSessions_SplitCleanTwoLaunches(1))
The yardstick: split_50 against clean_live and that baseline's own spread (max - min of its windows) in the same run.  The outputs
of the three forms after the last window are compared and must be equal.
--quick: one size, P = 50 only, one short window per variant -- the run to put under a kernel trace."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="65536,4096")
    ap.add_argument("--shares", default="0,25,50,75,100")
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--window-ms", type=float, default=250.0, help="device work per timed window, roughly: the ticks per window are sized by it")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch

    import webrtc_aecm_amd as aecm
    if not torch.cuda.is_available():
        raise SystemExit("bench_split_clean.py measures on the GPU; no device found")
    NO_CLEAN = aecm.ffi.SESSION_NO_CLEAN
    fs, n = args.fs, args.fs // 100
    shares = [50] if args.quick else [int(x) for x in args.shares.split(",")]
    sizes = [int(x) for x in args.streams.split(",")][:1 if args.quick else None]
    for S in sizes:
        g = torch.Generator(device="cuda").manual_seed(1)
        far = (torch.randn((S, n * 8), generator=g, device="cuda") * 3000).clamp_(-32768, 32767).to(torch.int16)
        near = (far.roll(37, dims=1) // 3 + (torch.randn((S, n * 8), generator=g, device="cuda") * 200).to(torch.int16))
        clean = (near - (torch.randn((S, n * 8), generator=g, device="cuda") * 100).to(torch.int16))
        ms = np.full(S, 40, dtype=np.int16)
        order = np.random.default_rng(7).permutation(S)

        class Variant:
            def __init__(self, name, flags, with_clean, force_sparse=False, two=None):
                self.name, self.flags, self.with_clean = name, flags, with_clean
                self.sess = aecm.AecmSessions(S, fs, 1, 1)
                self.out = torch.empty_like(far)
                if force_sparse:
                    assert self.sess.force_sparse_ticks(True) == 0
                if two is not None:
                    assert self.sess.split_clean_two_launches(two) == 0
                self.i = 0
                self.times = []

            def ticks(self, count):
                for _ in range(count):
                    off = (self.i % 8) * n * 2
                    rc = self.sess.tick_async(far.data_ptr() + off, near.data_ptr() + off, self.out.data_ptr() + off, far.shape[1], n, 40,
                                              clean_ptr=clean.data_ptr() + off if self.with_clean else None, ms_per_session=ms, flags=self.flags)
                    assert rc == 0, (self.name, rc)
                    self.i += 1

            def window(self, count):
                assert self.sess.synchronize() == 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                self.ticks(count)
                assert self.sess.synchronize() == 0
                self.times.append((time.perf_counter() - t0) / count * 1e3)

        none = np.zeros(S, dtype=np.uint8)
        variants = [Variant("clean_live", none, True, force_sparse=True), Variant("noclean_live", none, False, force_sparse=True)]
        for p in shares:
            flags = none.copy()
            flags[order[:(S * p + 50) // 100]] = NO_CLEAN
            variants.append(Variant(f"split_{p}", flags, True))
            if 0 < p < 100:
                variants.append(Variant(f"split_{p}_fused", flags, True, two=False))
                variants.append(Variant(f"split_{p}_two", flags, True, two=True))
        for v in variants:                                   # through the start-up phase, and every launch shape warmed up
            v.ticks(48)
            assert v.sess.synchronize() == 0
        # ticks per window from a first look at the baseline
        variants[0].window(50)
        per_tick = variants[0].times.pop()
        count = 100 if args.quick else max(50, int(args.window_ms / max(per_tick, 1e-3)))
        for r in range(1 if args.quick else args.repeats):
            for v in variants:
                v.window(count)
        by_name = {v.name: v for v in variants}
        for p in shares:
            if 0 < p < 100:
                a = by_name[f"split_{p}"]
                for b in (by_name[f"split_{p}_fused"], by_name[f"split_{p}_two"]):
                    assert a.i == b.i and torch.equal(a.out, b.out), ("the forms' outputs differ", p, b.name)
        base = by_name["clean_live"].times
        line = {"streams": S, "fs": fs, "audio": "device", "async": True, "ticks_per_window": count, "windows": len(base),
                "clean_live_spread_ms": max(base) - min(base),
                "rows": [{"variant": v.name, "flagged": int(((v.flags & NO_CLEAN) != 0).sum()), "ms_per_tick": float(np.median(v.times)),
                          "vs_clean_live": float(np.median(v.times) / np.median(base)), "all_ms_per_tick": v.times} for v in variants]}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
        for v in variants:
            v.sess.close()
        del variants, by_name


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Serving-shaped measurement (run ON THE GPU BOX): S concurrent WebRtcAecm_* sessions on a 10 ms clock
(WebRtcAecmSessions_Tick*).  Reports the time per tick, the bytes that cross the host boundary per second and how many
real-time streams one GPU sustains.  Not the headline metric (bench.py is); rows for BASELINE.md / INTEGRATION.md.

Where the audio lives (--audio):
  device           far / near / out rows in HBM (a media pipeline whose decoder and encoder run on the GPU too)
  host             pageable host memory through WebRtcAecmSessions_TickHost (staged by the library, synchronous)
  host-registered  caller-owned host buffers registered once (WebRtcAecmBatch_RegisterHostBuffer): the tick kernel reads
                   and writes them in place over the link -- no copies at all
  host-staged      pinned host buffers, three slots in flight: upload of tick t + 1, tick t and download of tick t - 1
                   overlap on three HIP streams, ordered by events only (WebRtcAecmSessions_TickAsync's wait / done hooks;
                   reference call shape: main.cc:112-145 -- far and near frames in, one output frame out per 10 ms)
A tick moves 2 x n x 2 bytes in and n x 2 bytes out per session (n = 160 at 16 kHz): 63 MB per tick of 65 536 sessions.

--occupancy P[,P...]: sparse ticks (AECM_SESSION_IDLE).  For each P a fixed, seeded random set of ceil(P x S) sessions is live and
the others sit out every tick; device-resident audio, WebRtcAecmSessions_TickAsync with per-session msInSndCardBuf and flags,
ticks enqueued back to back.  Printed next to the dense tick of the same object size (the same call without a flags array,
--repeats times: its spread is the yardstick for every difference).  P = 1.0 is a tick forced through the live list and the
sparse tick kernel with nobody idle (WebRtcAecmSessions_ForceSparseTicks): what the indirection itself costs.

--mixed P[,P...]: one object per clock, not per rate.  For each P an object of rate 16 000 in which a fixed, seeded random P % of the
sessions are 8 kHz sessions (WebRtcAecmSessions_InitRates) that make a half call (AECM_SESSION_HALF_CALL: 10 ms = 80 samples) in
every 160-sample tick, the rest 16 kHz / 160; device-resident audio, TickAsync with per-session msInSndCardBuf and flags.  Printed
next to (a) the all-16 kHz object of the same size without a flags array -- and once more with the arrays the mixed rows pass, flags
that name nothing --, and (d) what a user without mixed objects does for the
50 % case: two objects of S / 2 sessions, one 8 kHz / 80 and one 16 kHz / 160, ticked back to back.  --repeats times each.

--calls K[,K...]: ticks of K call pairs (WebRtcAecmSessions_TickCallsAsync: a 20 .. 60 ms packet interval on 10 ms calls in one
planning and one tick launch).  For each K, in one process and interleaved (K-call object, twin, K-call object, twin, ...,
--repeats rounds): one K-call tick of an object against K back-to-back WebRtcAecmSessions_TickAsync ticks of a twin object on the
same rows; device-resident audio, per-session msInSndCardBuf and flags.  With --occupancy P (a fraction, or per cent when > 1) a
fixed, seeded random share of the sessions is live and the others sit out every tick.  Printed: ms per K-call tick, ms per K
ordinary ticks, the ratio (< 1: the K-call tick is cheaper).

--packets K[,K...] [--mixed P[,P...]]: packet ticks (WebRtcAecmSessions_TickPacketsAsync: one packet of K 10 ms calls per session,
every session at its own rate and call size, rows packed).  For each P (per cent of the sessions that are 8 kHz sessions making half
calls in a 16 kHz object ticking 160; default 0) and each K, by --calls' interleaved, median-of-repeats method: one packet tick of
an object against K back-to-back WebRtcAecmSessions_TickAsync ticks flagged AECM_SESSION_HALF_CALL of a twin object of the same
rates.  P = 0 is a uniform object without half flags: the routing falls back to the K-call tick's launches (compare with --calls).
Outputs are compared at P = 0 only (with half calls the twin's rows are laid out differently; tests/test_gpu_tick_packets.py
compares those).
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--classes", type=int, default=1,
                    help="distinct msInSndCardBuf values among the sessions (> 1: WebRtcAecmSessions_TickPerSession, one value per session)")
    ap.add_argument("--audio", choices=["device", "host", "host-registered", "host-staged"], default="device")
    ap.add_argument("--host", action="store_true", help="= --audio host")
    ap.add_argument("--pinned", action="store_true", help="= --audio host-registered")
    ap.add_argument("--async", dest="asynchronous", action="store_true",
                    help="WebRtcAecmSessions_TickAsync: ticks are enqueued back to back, one synchronisation at the end (host-staged always is)")
    ap.add_argument("--occupancy", default="", help="P[,P...]: share of the sessions that is live; the others are idle every tick (see above)")
    ap.add_argument("--mixed", default="", help="P[,P...]: per cent of the sessions that are 8 kHz half-call sessions in a 16 kHz object (see above)")
    ap.add_argument("--repeats", type=int, default=3, help="--occupancy / --mixed / --calls: measurements per column (the median is reported, all are listed)")
    ap.add_argument("--calls", default="", help="K[,K...]: a tick of K call pairs against K back-to-back ticks of a twin object (see above)")
    ap.add_argument("--packets", default="", help="K[,K...]: a packet tick of K calls per session against K back-to-back ticks of a twin object; with --mixed P[,P...] (see above)")
    args = ap.parse_args()
    if args.packets:
        return packets_sweep(args)
    if args.calls:
        return calls_sweep(args)
    if args.occupancy:
        return occupancy_sweep(args)
    if args.mixed:
        return mixed_sweep(args)
    if args.host:
        args.audio = "host"
    if args.pinned:
        args.audio = "host-registered"
    import numpy as np
    import torch

    import webrtc_aecm_amd as aecm
    S, fs = args.streams, args.fs
    n = fs // 100                                     # one 10 ms tick
    g = torch.Generator(device="cuda").manual_seed(1)
    far = (torch.randn((S, n * 8), generator=g, device="cuda") * 3000).clamp_(-32768, 32767).to(torch.int16)
    near = (far.roll(37, dims=1) // 3 + (torch.randn((S, n * 8), generator=g, device="cuda") * 200).to(torch.int16))
    out = torch.empty_like(far)                       # Tick() uses ONE row stride for far, near and out
    sess = aecm.AecmSessions(S, fs, 1, 1)
    lib = aecm.load()
    torch.cuda.synchronize()
    ms = (40 + (np.arange(S) % args.classes)).astype(np.int16)          # distinct values in [40, 40 + classes)

    if args.audio in ("host", "host-registered"):
        hfar = np.ascontiguousarray(far.cpu().numpy()[:, :n])
        hnear = np.ascontiguousarray(near.cpu().numpy()[:, :n])
    if args.audio == "host-registered":
        hout = np.zeros_like(hnear)
        pf, pn, po = (aecm.register_host_buffer(a) for a in (hfar, hnear, hout))
    if args.audio == "host-staged":
        K = 3
        hfar_t, hnear_t = far[:, :n].contiguous().cpu().pin_memory(), near[:, :n].contiguous().cpu().pin_memory()
        hout_t = [torch.zeros((S, n), dtype=torch.int16).pin_memory() for _ in range(K)]
        dfar = [torch.zeros((S, n), dtype=torch.int16, device="cuda") for _ in range(K)]
        dnear = [torch.zeros_like(dfar[0]) for _ in range(K)]
        dout = [torch.zeros_like(dfar[0]) for _ in range(K)]
        upload, download = torch.cuda.Stream(), torch.cuda.Stream()
        ready = [torch.cuda.Event() for _ in range(K)]
        done = [torch.cuda.Event() for _ in range(K)]
        consumed = [None] * K
        for e in done:                                # torch creates the hipEvent_t at the first record; the tick re-records it
            e.record(download)
        torch.cuda.synchronize()

    def tick(i):
        if args.audio == "host-staged":
            k = i % K
            with torch.cuda.stream(upload):           # tick i's rows: host -> slot k, once the download of the tick that last used the slot is through
                if consumed[k] is not None:
                    upload.wait_event(consumed[k])
                dfar[k].copy_(hfar_t, non_blocking=True)
                dnear[k].copy_(hnear_t, non_blocking=True)
                ready[k].record(upload)
            rc = lib.WebRtcAecmSessions_TickAsync(sess.h, dfar[k].data_ptr(), dnear[k].data_ptr(), None, dout[k].data_ptr(), n, n, 40, None, None, None,
                                                  ready[k].cuda_event, done[k].cuda_event)
            assert rc == 0, rc
            with torch.cuda.stream(download):
                download.wait_event(done[k])
                hout_t[k].copy_(dout[k], non_blocking=True)
                consumed[k] = torch.cuda.Event()
                consumed[k].record(download)
            return
        if args.audio == "host-registered":
            rc = sess.tick_async(pf, pn, po, n, n, 40) if args.asynchronous else sess.tick_device(pf, pn, po, n, n, 40)
            assert rc == 0, rc
            return
        if args.audio == "host":
            rc = sess.tick_host_per_session(hfar, hnear, ms)[0] if args.classes > 1 else sess.tick_host(hfar, hnear, 40)[0]
            assert rc == 0, rc
            return
        off = (i % 8) * n * 2
        if args.asynchronous:
            rc = sess.tick_async(far.data_ptr() + off, near.data_ptr() + off, out.data_ptr(), far.shape[1], n, 40,
                                 ms_per_session=ms if args.classes > 1 else None)
        elif args.classes > 1:
            rc = sess.tick_device_per_session(far.data_ptr() + off, near.data_ptr() + off, out.data_ptr(), far.shape[1], n, ms)
        else:
            rc = sess.tick_device(far.data_ptr() + off, near.data_ptr() + off, out.data_ptr(), far.shape[1], n, 40)
        assert rc == 0, rc
    for i in range(40):                               # through the start-up phase
        tick(i)
    assert sess.synchronize() == 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.ticks):
        tick(40 + i)
    assert sess.synchronize() == 0
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.ticks
    blocks_per_tick = n / 64.0
    boundary_bytes = 0 if args.audio == "device" else 3 * S * n * 2
    desc = aecm.describe_tick(S, aecm.device_info(0)[1])
    print(json.dumps({"streams": S, "fs": fs, "audio": args.audio, "async": bool(args.asynchronous or args.audio == "host-staged"),
                      "ms_per_tick": dt * 1e3, "frames_per_s": S * blocks_per_tick / dt, "realtime_streams_per_gpu": int(S * 0.010 / dt),
                      "MB_over_the_boundary_per_tick": boundary_bytes / 1e6, "GBps_over_the_boundary": boundary_bytes / dt / 1e9,
                      "tick_workgroup_rounds": desc["rounds_x1000"] / 1000.0}))


def occupancy_sweep(args):
    import math

    import numpy as np
    import torch

    import webrtc_aecm_amd as aecm
    S, fs = args.streams, args.fs
    n = fs // 100
    g = torch.Generator(device="cuda").manual_seed(1)
    far = (torch.randn((S, n * 8), generator=g, device="cuda") * 3000).clamp_(-32768, 32767).to(torch.int16)
    near = (far.roll(37, dims=1) // 3 + (torch.randn((S, n * 8), generator=g, device="cuda") * 200).to(torch.int16))
    out = torch.empty_like(far)
    ms = np.full(S, 40, dtype=np.int16)
    cus = aecm.device_info(0)[1]

    def measure(flags, force_sparse):
        """ms per tick, args.repeats times, on a fresh object that has left its start-up phase under the same flags."""
        sess = aecm.AecmSessions(S, fs, 1, 1)
        if force_sparse:
            assert sess.force_sparse_ticks(True) == 0

        def tick(i):
            off = (i % 8) * n * 2
            rc = sess.tick_async(far.data_ptr() + off, near.data_ptr() + off, out.data_ptr(), far.shape[1], n, 40, ms_per_session=ms, flags=flags)
            assert rc == 0, rc
        for i in range(40):
            tick(i)
        times = []
        for r in range(args.repeats):
            assert sess.synchronize() == 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.ticks):
                tick(40 + i)
            assert sess.synchronize() == 0
            times.append((time.perf_counter() - t0) / args.ticks * 1e3)
        sess.close()
        return times

    dense = measure(None, False)
    rows = []
    for p in [float(x) for x in args.occupancy.split(",")]:
        live = min(S, math.ceil(p * S))
        flags = np.full(S, aecm.ffi.SESSION_IDLE, dtype=np.uint8)
        flags[np.random.default_rng(7).permutation(S)[:live]] = 0
        times = measure(flags, force_sparse=live == S)
        rows.append({"occupancy": p, "live": live, "ms_per_tick": float(np.median(times)), "all_ms_per_tick": times,
                     "tick_workgroup_rounds": aecm.describe_tick_live(S, live, cus)["rounds_x1000"] / 1000.0,
                     "forced_sparse": live == S})
    print(json.dumps({"streams": S, "fs": fs, "audio": "device", "async": True, "ticks": args.ticks,
                      "dense_ms_per_tick": float(np.median(dense)), "dense_all_ms_per_tick": dense,
                      "dense_tick_workgroup_rounds": aecm.describe_tick(S, cus)["rounds_x1000"] / 1000.0, "sparse": rows}))


def calls_sweep(args):
    import math

    import numpy as np
    import torch

    import webrtc_aecm_amd as aecm
    S, fs = args.streams, args.fs
    n = fs // 100
    ks = [int(x) for x in args.calls.split(",")]
    width = n * max(ks) * 2                           # two packet intervals of the largest K per row
    g = torch.Generator(device="cuda").manual_seed(1)
    far = (torch.randn((S, width), generator=g, device="cuda") * 3000).clamp_(-32768, 32767).to(torch.int16)
    near = (far.roll(37, dims=1) // 3 + (torch.randn((S, width), generator=g, device="cuda") * 200).to(torch.int16))
    out_a, out_b = torch.empty_like(far), torch.empty_like(far)
    ms = np.full(S, 40, dtype=np.int16)
    p = float(args.occupancy) if args.occupancy else 1.0
    p = p / 100.0 if p > 1.0 else p
    live = min(S, math.ceil(p * S))
    flags = None
    if live < S:
        flags = np.full(S, aecm.ffi.SESSION_IDLE, dtype=np.uint8)
        flags[np.random.default_rng(7).permutation(S)[:live]] = 0
    rows = []
    for K in ks:
        a, b = aecm.AecmSessions(S, fs, 1, 1), aecm.AecmSessions(S, fs, 1, 1)

        def tick_a(i):
            off = (i % 2) * K * n * 2
            rc, _ = a.tick_calls_device(far.data_ptr() + off, near.data_ptr() + off, out_a.data_ptr() + off, width, n, K, ms, flags=flags, asynchronous=True)
            assert rc == 0, rc

        def tick_b(i):
            for c in range(K):
                off = ((i % 2) * K + c) * n * 2
                rc = b.tick_async(far.data_ptr() + off, near.data_ptr() + off, out_b.data_ptr() + off, width, n, 40, ms_per_session=ms, flags=flags)
                assert rc == 0, rc
        warm = -(-40 // K)                            # both through the start-up phase, on the same calls
        for i in range(warm):
            tick_a(i)
            tick_b(i)
        times = {"a": [], "b": []}
        at = warm
        for r in range(args.repeats):
            for key, obj, tick in (("a", a, tick_a), ("b", b, tick_b)):
                assert a.synchronize() == 0 and b.synchronize() == 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.ticks):
                    tick(at + i)
                assert obj.synchronize() == 0
                times[key].append((time.perf_counter() - t0) / args.ticks * 1e3)
            at += args.ticks
        assert a.synchronize() == 0 and b.synchronize() == 0
        same = bool(torch.equal(out_a[:, :2 * K * n], out_b[:, :2 * K * n])) if live == S else None      # (idle rows are never written)
        ta, tb = float(np.median(times["a"])), float(np.median(times["b"]))
        rows.append({"calls": K, "ms_per_k_call_tick": ta, "ms_per_k_ticks": tb, "ratio": ta / tb, "all_k_call": times["a"], "all_k_ticks": times["b"],
                     "outputs_equal": same})
        a.close(), b.close()
    print(json.dumps({"streams": S, "fs": fs, "n": n, "audio": "device", "async": True, "ticks": args.ticks, "live": live, "rows": rows}))


def packets_sweep(args):
    import numpy as np
    import torch

    import webrtc_aecm_amd as aecm
    S, fs, n = args.streams, 16000, 160
    ks = [int(x) for x in args.packets.split(",")]
    width = n * max(ks) * 2                           # two packets of the largest K per row
    g = torch.Generator(device="cuda").manual_seed(1)
    far = (torch.randn((S, width), generator=g, device="cuda") * 3000).clamp_(-32768, 32767).to(torch.int16)
    near = (far.roll(37, dims=1) // 3 + (torch.randn((S, width), generator=g, device="cuda") * 200).to(torch.int16))
    out_a, out_b = torch.empty_like(far), torch.empty_like(far)
    ms = np.full(S, 40, dtype=np.int16)
    rows = []
    for p in [float(x) for x in (args.mixed or "0").split(",")]:
        narrow = np.zeros(S, dtype=bool)
        narrow[np.random.default_rng(7).permutation(S)[:int(round(p / 100 * S))]] = True
        rates = np.where(narrow, 8000, 16000).astype(np.int32)
        flags = np.where(narrow, aecm.ffi.SESSION_HALF_CALL, 0).astype(np.uint8) if narrow.any() else None
        for K in ks:
            a, b = (aecm.AecmSessions(S, fs, 1, 1, rates=rates if narrow.any() else None) for _ in range(2))

            def tick_a(i):
                off = (i % 2) * K * n * 2
                rc, _ = a.tick_packets_device(far.data_ptr() + off, near.data_ptr() + off, out_a.data_ptr() + off, width, n, K, ms, flags=flags, asynchronous=True)
                assert rc == 0, rc

            def tick_b(i):
                for c in range(K):
                    off = ((i % 2) * K + c) * n * 2
                    rc = b.tick_async(far.data_ptr() + off, near.data_ptr() + off, out_b.data_ptr() + off, width, n, 40, ms_per_session=ms, flags=flags)
                    assert rc == 0, rc
            warm = -(-40 // K)                        # both through the start-up phase, on the same number of calls
            for i in range(warm):
                tick_a(i)
                tick_b(i)
            times = {"a": [], "b": []}
            at = warm
            for r in range(args.repeats):
                for key, obj, tick in (("a", a, tick_a), ("b", b, tick_b)):
                    assert a.synchronize() == 0 and b.synchronize() == 0
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(args.ticks):
                        tick(at + i)
                    assert obj.synchronize() == 0
                    times[key].append((time.perf_counter() - t0) / args.ticks * 1e3)
                at += args.ticks
            assert a.synchronize() == 0 and b.synchronize() == 0
            same = bool(torch.equal(out_a[:, :2 * K * n], out_b[:, :2 * K * n])) if not narrow.any() else None
            ta, tb = float(np.median(times["a"])), float(np.median(times["b"]))
            rows.append({"mixed_percent": p, "narrowband": int(narrow.sum()), "calls": K, "ms_per_packet_tick": ta, "ms_per_k_ticks": tb, "ratio": ta / tb,
                         "all_packet": times["a"], "all_k_ticks": times["b"], "outputs_equal": same})
            a.close(), b.close()
    print(json.dumps({"streams": S, "fs": fs, "n": n, "audio": "device", "async": True, "ticks": args.ticks, "rows": rows}))


def mixed_sweep(args):
    import numpy as np
    import torch

    import webrtc_aecm_amd as aecm
    S, n = args.streams, 160
    g = torch.Generator(device="cuda").manual_seed(1)
    far = (torch.randn((S, n * 8), generator=g, device="cuda") * 3000).clamp_(-32768, 32767).to(torch.int16)
    near = (far.roll(37, dims=1) // 3 + (torch.randn((S, n * 8), generator=g, device="cuda") * 200).to(torch.int16))
    out = torch.empty_like(far)

    def measure(objects):
        """ms per tick of the clock, args.repeats times: objects = [(sessions, first row, samples per tick, ms or None, flags or None)],
        ticked back to back, each past its start-up phase under the same arguments."""
        def tick(i):
            for sess, row, k, ms, flags in objects:
                off = row * far.shape[1] * 2 + (i % 8) * k * 2
                rc = sess.tick_async(far.data_ptr() + off, near.data_ptr() + off, out.data_ptr() + row * far.shape[1] * 2, far.shape[1], k, 40,
                                     ms_per_session=ms, flags=flags)
                assert rc == 0, rc
        for i in range(40):
            tick(i)
        times = []
        for r in range(args.repeats):
            for o in objects:
                assert o[0].synchronize() == 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.ticks):
                tick(40 + i)
            for o in objects:
                assert o[0].synchronize() == 0
            times.append((time.perf_counter() - t0) / args.ticks * 1e3)
        for o in objects:
            o[0].close()
        return times

    row = lambda name, times, **kw: dict(case=name, ms_per_tick=float(np.median(times)), all_ms_per_tick=times, **kw)
    rows = [row("uniform 16 kHz / 160, no flags", measure([(aecm.AecmSessions(S, 16000, 1, 1), 0, 160, None, None)]))]
    # the same uniform object handed the arrays the mixed rows hand over (msInSndCardBuf per session, flags that name nothing): what
    # the host's passes over them and the two pinned copies cost -- the launches are those of the row above
    rows.append(row("uniform 16 kHz / 160, ms and flags arrays", measure([(aecm.AecmSessions(S, 16000, 1, 1), 0, 160, np.full(S, 40, dtype=np.int16),
                                                                          np.zeros(S, dtype=np.uint8))])))
    for p in [float(x) for x in args.mixed.split(",")]:
        narrow = np.zeros(S, dtype=bool)
        narrow[np.random.default_rng(7).permutation(S)[:int(round(p / 100 * S))]] = True
        rates = np.where(narrow, 8000, 16000).astype(np.int32)
        flags = np.where(narrow, aecm.ffi.SESSION_HALF_CALL, 0).astype(np.uint8)
        sess = aecm.AecmSessions(S, 16000, 1, 1, rates=rates)
        rows.append(row(f"mixed {p:g} % 8 kHz half calls", measure([(sess, 0, 160, np.full(S, 40, dtype=np.int16), flags)]), narrowband=int(narrow.sum())))
    half = S // 2
    rows.append(row("two objects of S / 2: 8 kHz / 80 + 16 kHz / 160", measure([(aecm.AecmSessions(half, 8000, 1, 1), 0, 80, None, None),
                                                                               (aecm.AecmSessions(S - half, 16000, 1, 1), half, 160, None, None)])))
    print(json.dumps({"streams": S, "audio": "device", "async": True, "ticks": args.ticks, "rows": rows}))


if __name__ == "__main__":
    main()

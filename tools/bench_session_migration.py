#!/usr/bin/env python3
"""Bulk session snapshots (WebRtcAecmSessions_ExportSessions / ImportSessions and their *Device forms) against the loop of
single-session calls -- the only way to drain, rebalance or checkpoint an object before there was a bulk form.  Writes
profiles/r18_session_migration.txt:

  1. static check: `python -m webrtc_aecm_amd.isa_census --all` of this tree's library against the parent commit's
     (--parent-lib: a libaecm_mi355x.so built from the parent with webrtc_aecm_amd/build.py) -- every kernel that existed before
     keeps its fingerprint;
  2. milliseconds to export and to import 256, 4 096 and 65 536 sessions of a 65 536-session object after 40 ticks, in three
     forms -- device memory, host memory (staged, 256 snapshots per copy), a registered host buffer (the kernels write it in place) --
     and, at 256 and 4 096 sessions, the loop of ExportSession / ImportSession calls on the same object.

No ratio is claimed in advance; where no GPU is present the second section says so."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def static_check(parent_lib):
    from webrtc_aecm_amd import build, isa_census
    ours = isa_census.census_of_text(isa_census.disassemble(build.build()))
    lines = ["1. Static check: every kernel that existed before this change against the parent commit's library", ""]
    if parent_lib is None:
        return lines + ["not compared: no parent library was given (--parent-lib)", ""], None
    theirs = isa_census.census_of_text(isa_census.disassemble(parent_lib))
    changed = [k for k in theirs if k not in ours or ours[k]["fingerprint"] != theirs[k]["fingerprint"]]
    new = sorted(k for k in ours if k not in theirs)
    lines += ["python -m webrtc_aecm_amd.isa_census --all on both libraries (sha256 of the disassembled instruction stream, first 16 hex digits).",
              f"{len(theirs)} kernels in the parent's library, {len(ours)} in this one; {len(theirs) - len(changed)} of the parent's keep their fingerprint, "
              f"{len(changed)} changed or missing, {len(new)} new.", ""]
    lines.append(f"{'kernel':100s} {'parent':>16s} {'this tree':>16s} {'instr':>6s}")
    for k in sorted(theirs):
        mine = ours.get(k)
        verdict = "MISSING" if mine is None else "equal" if mine["fingerprint"] == theirs[k]["fingerprint"] else "CHANGED"
        lines.append(f"{k[:100]:100s} {theirs[k]['fingerprint']:>16s} {(mine or {}).get('fingerprint', '-'):>16s} {theirs[k]['n_instructions']:6d}  {verdict}")
    for k in new:
        lines.append(f"{k[:100]:100s} {'-':>16s} {ours[k]['fingerprint']:>16s} {ours[k]['n_instructions']:6d}  new")
    lines.append("")
    return lines, not changed


def timed(fn, repeats):
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def measure(total, counts, loop_counts, repeats):
    import torch

    import webrtc_aecm_amd as aecm
    fs, frame = 16000, 160
    size = aecm.load().WebRtcAecmSessions_session_size_bytes()
    g = torch.Generator(device="cuda").manual_seed(1)
    f = (torch.randn((total, frame * 8), generator=g, device="cuda") * 3000).clamp_(-32768, 32767).to(torch.int16)
    d = (f.roll(37, dims=1) // 3 + (torch.randn((total, frame * 8), generator=g, device="cuda") * 200).to(torch.int16))
    o = torch.empty_like(f)
    a = aecm.AecmSessions(total, fs, 1, 3)
    b = aecm.AecmSessions(total, fs, 1, 3)
    torch.cuda.synchronize()
    for i in range(40):
        off = (i % 8) * frame * 2
        assert a.tick_device(f.data_ptr() + off, d.data_ptr() + off, o.data_ptr(), f.shape[1], frame, 40) == 0
    del f, d, o
    dev = torch.empty(max(counts) * size, dtype=torch.uint8, device="cuda")
    host = np.empty(max(counts) * size, dtype=np.uint8)
    pinned = np.empty(max(counts) * size, dtype=np.uint8)
    alias = aecm.ffi.register_host_buffer(pinned)
    torch.cuda.synchronize()
    lib = a.lib
    rows = []
    for count in counts:
        n = count * size
        # every export before the import of the same form: the imports read what the exports wrote
        forms = (
            ("device memory", lambda: lib.WebRtcAecmSessions_ExportSessionsDevice(a.h, None, count, dev.data_ptr(), n),
             lambda: lib.WebRtcAecmSessions_ImportSessionsDevice(b.h, None, count, dev.data_ptr(), n, 0)),
            ("host memory (staged)", lambda: lib.WebRtcAecmSessions_ExportSessions(a.h, None, count, host.ctypes.data, n),
             lambda: lib.WebRtcAecmSessions_ImportSessions(b.h, None, count, host.ctypes.data, n, 0)),
            ("registered host buffer", lambda: lib.WebRtcAecmSessions_ExportSessionsDevice(a.h, None, count, alias, n),
             lambda: lib.WebRtcAecmSessions_ImportSessionsDevice(b.h, None, count, alias, n, 0)),
        )
        for name, export, imp in forms:
            def checked(call):
                def run():
                    rc = call()
                    assert rc == 0, (name, count, rc)
                return run
            checked(export)()                                  # warm-up: the grow-only buffers
            e = timed(checked(export), repeats)
            checked(imp)()
            i = timed(checked(imp), repeats)
            rows.append((count, name, e, i))
            print(count, name, e, i, file=sys.stderr, flush=True)
        if count in loop_counts:
            base = host.ctypes.data

            def export_loop():
                for k in range(count):
                    assert lib.WebRtcAecmSessions_ExportSession(a.h, k, base + k * size, size) == 0

            def import_loop():
                for k in range(count):
                    assert lib.WebRtcAecmSessions_ImportSession(b.h, k, base + k * size, size) == 0
            e = timed(export_loop, 1)
            i = timed(import_loop, 1)
            rows.append((count, "loop of ExportSession / ImportSession", e, i))
            print(count, "loop", e, i, file=sys.stderr, flush=True)
    # the bulk form wrote what the loop writes
    assert lib.WebRtcAecmSessions_ExportSessions(a.h, None, 256, host.ctypes.data, 256 * size) == 0
    for k in (0, 255):
        rc, snap = a.export_session(k)
        assert rc == 0 and snap == host[k * size:(k + 1) * size].tobytes()
    aecm.ffi.unregister_host_buffer(pinned)
    dev_name, cus, _ = aecm.device_info(0)
    name = f"{dev_name} ({cus} CUs)"
    a.close(), b.close()
    return rows, name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libaecm_mi355x.so built from the parent commit (static check)")
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--counts", default="256,4096,65536")
    ap.add_argument("--loop-counts", default="256,4096")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-measure", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r18_session_migration.txt"))
    args = ap.parse_args()
    title = "Bulk session snapshots: export and import of a list of sessions, gathered on the device"
    lines = [title, "=" * len(title), ""]
    static, kept = static_check(args.parent_lib)
    lines += static
    lines += ["2. Export and import of the first N sessions of a %d-session object (16 kHz, 160-sample ticks) after 40 ticks, ms per call" % args.sessions, ""]
    measured = None
    if not args.no_measure:
        try:
            import torch
            have_gpu = torch.cuda.is_available()
        except ImportError:
            have_gpu = False
        if have_gpu:
            counts = [int(c) for c in args.counts.split(",") if int(c) <= args.sessions]
            measured, device = measure(args.sessions, counts, [int(c) for c in args.loop_counts.split(",")], args.repeats)
            lines += [f"Measured on {device}: tools/bench_session_migration.py --repeats {args.repeats}; median (min .. max) of the repeats, the loops once.",
                      "Import goes into a second object of the same size; every call returns when its work is done.", ""]
            lines.append(f"{'sessions':>8s}  {'form':40s} {'export ms':>32s} {'import ms':>32s}")
            for count, name, e, i in measured:
                fmt = lambda t: f"{t[0]:10.3f} ({t[1]:.3f} .. {t[2]:.3f})"
                lines.append(f"{count:8d}  {name:40s} {fmt(e):>32s} {fmt(i):>32s}")
            lines.append("")
    if measured is None:
        lines += ["not yet measured on hardware", ""]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines))
    print(json.dumps({"out": args.out, "pre_existing_kernels_keep_their_fingerprints": kept,
                      "rows": [[c, n, e[0], i[0]] for c, n, e, i in (measured or [])]}))
    return 0 if kept in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())

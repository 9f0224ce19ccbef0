#!/usr/bin/env python3
"""Run ON THE GPU BOX: what a ragged launch (WebRtcAecmBatch_ProcessBlocksRagged) is worth.

For S = 65 536 and 8 192 streams, T = 1 280 blocks and three length distributions --
    equal               every stream T blocks
    uniform[T/4, T]     lengths spread evenly between a quarter and the whole of the longest
    one_long            every stream T/8 blocks but 1 % of them T
-- it times, interleaved, REPS repetitions each of
    (a) ragged          the ragged launch of the batch
    (b) padded          the equal-length launch of the same batch, every stream run to T (what a caller had to do before)
    (c) equal work      an equal-length launch of T' = sum of the lengths / S blocks: the same useful work without raggedness
and prints useful frames/s = sum of the lengths / wall time for each, with the min-max spread over the repetitions.  Wall time
is a host clock around launch + synchronise (the ragged launch's plan building and upload are part of it); the library's own
kernel time (HIP events) is printed next to it.  The gate the tool reports (exit 1 when missed): on uniform and one_long every
repetition of (a) is faster than every repetition of (b).

Every point runs in a child process of its own under a time limit; the first child that fails ends the run.

    python tools/bench_ragged.py [--sizes 65536,8192] [--blocks 1280] [--reps 5] [--timeout 300]

--pipelined: what the pipelined form of a ragged launch the chip holds at once (WebRtcAecmBatch_SetRaggedPipelining) is worth.
For S in --sizes (default 256, 1 024, 2 048, 3 072, 4 096 and two non-multiples of the CU count), T = --blocks (default 2 048 here)
and the distributions uniform and one_long (1 % of the streams 8 x the common length) it records useful frames/s of
    (a) parent      the library given with --parent (a build of the parent commit: tools/ab_build.py or a copy of its shipped
                    library under webrtc_aecm_amd/_lib/) running the same ragged launch -- one wavefront per stream
    (b) off         this build with the switch off
    (c) on          this build with the switch on
    (d) equal       this build's equal-length pipelined launch of the same total work (sum of the lengths / S blocks per stream)
(tools/ab.sh, the usual way to interleave two builds, times bench.py, and bench.py issues equal-length launches only; so this tool
does the interleaving itself, the same way: one child process per library, $AECM_LIB_PATH naming the library.)
(a) and (b, c, d) run in child processes of their own, interleaved --passes times; the spread of a figure over the passes and the
repetitions inside them is printed next to it, and (c) is called faster than (a) only when their ranges do not overlap.

    python tools/bench_ragged.py --pipelined --parent webrtc_aecm_amd/_lib/ab_parent.so [--sizes ...] [--blocks 2048] [--reps 4] [--passes 2]

--pipelined --clean: the same sweep for ragged launches WITH a clean near-end input (WebRtcAecmBatch_SetRaggedCleanPipelining).
(a), (b) and (c) run the ragged launch with a clean input -- the parent's library, this build with the new switch off, this build
with it on -- and (d) is this build's ragged launch of the same lengths WITHOUT a clean input with WebRtcAecmBatch_SetRaggedPipelining on:
what the third transform and the wider hand-over cost.  (b) runs in a child of its own that does exactly what (a)'s child does -- the
one launch, back to back -- so that the two columns differ in the library alone; (c) and (d) alternate in a third child.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
DISTRIBUTIONS = ("equal", "uniform", "one_long")


def lengths(dist, S, T, seed=1):
    import numpy as np
    rs = np.random.RandomState(seed)
    if dist == "equal":
        return np.full(S, T, dtype=np.int32)
    if dist == "uniform":
        lens = rs.randint(T // 4, T + 1, size=S).astype(np.int32)
        lens[0] = T
        return lens
    lens = np.full(S, T // 8, dtype=np.int32)
    lens[rs.choice(S, size=max(1, S // 100), replace=False)] = T
    return lens


def point(S, T, dist, reps, fs):
    import numpy as np
    import torch

    import webrtc_aecm_amd as aecm
    from bench import synth_on_device
    device = torch.device("cuda", 0)
    far, near = synth_on_device(torch, S, T * 64, 1234, device)
    out = torch.empty_like(near)
    stride = far.shape[1]
    lens = lengths(dist, S, T)
    total = int(lens.sum())
    t_equal = max(1, total // S)
    batch = aecm.AecmBatch(S, fs, cng_mode=1, echo_mode=1, device=0)
    ptrs = (far.data_ptr(), near.data_ptr(), out.data_ptr(), stride, 64)
    runs = {"ragged": lambda: batch.process_ragged_device(*ptrs, T, lens),
            "padded": lambda: batch.process_device(*ptrs, T),
            "equal_work": lambda: batch.process_device(*ptrs, t_equal)}
    wall = {k: [] for k in runs}
    kernel = {k: [] for k in runs}
    for name, run in runs.items():                      # warm-up: every shape once
        run()
    batch.synchronize()
    for _ in range(reps):
        for name, run in runs.items():
            batch.reset_timers()
            t0 = time.perf_counter()
            run()
            batch.synchronize()
            wall[name].append(time.perf_counter() - t0)
            kernel[name].append(batch.timers()[0] / 1e3)
    d = batch.describe_ragged_launch(lens)
    useful = {"ragged": total, "padded": total, "equal_work": S * t_equal}
    rec = {"streams": S, "blocks": T, "dist": dist, "sum_blocks": total, "padded_blocks": S * T, "equal_work_blocks_per_stream": t_equal,
           "form": d["form"], "chunk_blocks": d["chunk_blocks"], "items": d["items"],
           "wall_s": wall, "kernel_s": kernel,
           "useful_frames_per_s": {k: [useful[k] / t for t in wall[k]] for k in runs}}
    rec["ragged_faster_than_padded_every_rep"] = max(wall["ragged"]) < min(wall["padded"])
    print("RESULT " + json.dumps(rec), flush=True)
    batch.close()


def pipelined_point(S, T, reps, fs, with_switch, clean=False, column="parent"):
    """One child: both distributions at one size on the library $AECM_LIB_PATH names (or the shipped one)."""
    import torch

    import webrtc_aecm_amd as aecm
    from bench import synth_on_device
    device = torch.device("cuda", 0)
    far, near = synth_on_device(torch, S, T * 64, 1234, device)
    out = torch.empty_like(near)
    ptrs = (far.data_ptr(), near.data_ptr(), out.data_ptr(), far.shape[1], 64)
    # (--clean) the clean input: 3/4 of the near end, as webrtc_aecm_amd.synth.synth_clean makes it
    clean_ptr = None
    if clean:
        near_clean = ((near.to(torch.int32) * 3) >> 2).to(torch.int16)
        clean_ptr = near_clean.data_ptr()
        torch.cuda.synchronize()
    for dist in ("uniform", "one_long"):
        lens = lengths(dist, S, T)
        total = int(lens.sum())
        t_equal = max(1, total // S)
        batch = aecm.AecmBatch(S, fs, cng_mode=1, echo_mode=1, device=0)
        runs = {}
        if with_switch and clean:
            def on():
                batch.set_ragged_clean_pipelining(True)
                batch.process_ragged_device(*ptrs, T, lens, clean_ptr)

            def equal():                                  # column (d) of the clean sweep: the same lengths without a clean input, pipelined
                batch.set_ragged_pipelining(True)
                batch.process_ragged_device(*ptrs, T, lens)
            runs = {"on": on, "equal": equal}
        elif with_switch:
            def on():
                batch.set_ragged_pipelining(True)
                batch.process_ragged_device(*ptrs, T, lens)

            def off():
                batch.set_ragged_pipelining(False)
                batch.process_ragged_device(*ptrs, T, lens)
            runs = {"off": off, "on": on, "equal": lambda: batch.process_device(*ptrs, t_equal)}
        else:
            runs = {column: lambda: batch.process_ragged_device(*ptrs, T, lens, clean_ptr)}      # (the switches at their defaults: off)
        wall = {k: [] for k in runs}
        for run in runs.values():
            run()
        batch.synchronize()
        for _ in range(reps):
            for name, run in runs.items():
                t0 = time.perf_counter()
                run()
                batch.synchronize()
                wall[name].append(time.perf_counter() - t0)
        useful = {k: (S * t_equal if k == "equal" and not clean else total) for k in runs}
        rec = {"streams": S, "blocks": T, "dist": dist, "sum_blocks": total, "frames_per_s": {k: [useful[k] / t for t in wall[k]] for k in runs}}
        if with_switch:
            if clean:
                batch.set_ragged_clean_pipelining(True)
            else:
                batch.set_ragged_pipelining(True)
            d = batch.describe_ragged_launch(lens, clean)
            rec.update(form_on=d["form"], shape_on=d["shape"], workgroups_on=d["workgroups"], evenness_on=d["cu_load_evenness_x1000"])
        print("RESULT " + json.dumps(rec), flush=True)
        batch.close()


def pipelined_main(a):
    import os
    sizes = [int(x) for x in (a.sizes if a.sizes != "65536,8192" else "256,1024,1030,2048,3072,3000,4096").split(",")]
    T = a.blocks if a.blocks != 1280 else 2048
    acc = {}
    for p in range(a.passes):
        for S in sizes:
            # (--clean: column (b) from a child shaped like (a)'s, on this build)
            for variant in (("parent",) if a.parent else ()) + (("off", "new") if a.clean else ("new",)):
                env = dict(os.environ)
                if variant == "parent":
                    env["AECM_LIB_PATH"] = str(Path(a.parent).resolve())
                cmd = [sys.executable, str(Path(__file__).resolve()), "--pipelined-point", str(S), variant, "--blocks", str(T), "--reps", str(a.reps), "--fs", str(a.fs)]
                if a.clean:
                    cmd.append("--clean")
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, env=env)
                except subprocess.TimeoutExpired:
                    print(f"{S} streams, {variant}: no result within {a.timeout} s; stopping", flush=True)
                    return 2
                lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                if r.returncode != 0 or len(lines) != 2:
                    print(f"{S} streams, {variant}: child failed with status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                    return 2
                for line in lines:
                    rec = json.loads(line[7:])
                    slot = acc.setdefault((S, rec["dist"]), {"sum_blocks": rec["sum_blocks"], "f": {}})
                    for k, v in rec["frames_per_s"].items():
                        slot["f"].setdefault(k, []).extend(v)
                    slot.update({k: rec[k] for k in ("form_on", "shape_on", "workgroups_on", "evenness_on") if k in rec})
    print(f"T = {T} blocks, {a.passes} interleaved passes x {a.reps} repetitions; M useful frames/s, min .. max over all of them")
    if a.clean:
        print("every column but (d) with a clean near-end input; (d): the same lengths without one, SetRaggedPipelining on")
    print(f"{'streams':>7} {'dist':>8} {'(a) parent':>17} {'(b) off':>17} {'(c) on':>17} {'(d) no clean' if a.clean else '(d) equal':>17}  form/shape/wgs/evenness  verdict")
    for (S, dist), slot in sorted(acc.items()):
        f = slot["f"]
        cell = lambda k: f"{min(f[k]) / 1e6:7.1f} ..{max(f[k]) / 1e6:7.1f}" if k in f else f"{'-':>17}"
        verdict = ""
        if "parent" in f:
            verdict = "on > parent" if min(f["on"]) > max(f["parent"]) else "on < parent" if max(f["on"]) < min(f["parent"]) else "within the spread"
            verdict += "; off = parent" if min(f["off"]) <= max(f["parent"]) and min(f["parent"]) <= max(f["off"]) else "; off != parent"
        print(f"{S:7d} {dist:>8} {cell('parent')} {cell('off')} {cell('on')} {cell('equal')}  {slot.get('form_on')}/{slot.get('shape_on', 0):#x}/{slot.get('workgroups_on')}/{slot.get('evenness_on')}  {verdict}",
              flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,8192")
    ap.add_argument("--blocks", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per point (one child process each)")
    ap.add_argument("--point", nargs=2, metavar=("STREAMS", "DIST"), help="(internal) run one point in this process")
    ap.add_argument("--pipelined", action="store_true", help="the sweep of the ragged pipelined form (see the module text)")
    ap.add_argument("--parent", help="--pipelined: a library built from the parent commit, for column (a)")
    ap.add_argument("--clean", action="store_true", help="--pipelined: the sweep with a clean near-end input and WebRtcAecmBatch_SetRaggedCleanPipelining")
    ap.add_argument("--passes", type=int, default=2, help="--pipelined: interleaved passes over the libraries")
    ap.add_argument("--pipelined-point", nargs=2, metavar=("STREAMS", "VARIANT"), help="(internal) one size on one library in this process")
    a = ap.parse_args()
    if a.pipelined_point:
        pipelined_point(int(a.pipelined_point[0]), a.blocks, a.reps, a.fs, a.pipelined_point[1] == "new", a.clean, a.pipelined_point[1])
        return 0
    if a.pipelined:
        return pipelined_main(a)
    if a.point:
        point(int(a.point[0]), a.blocks, a.point[1], a.reps, a.fs)
        return 0
    missed = []
    for S in (int(x) for x in a.sizes.split(",")):
        for dist in DISTRIBUTIONS:
            cmd = [sys.executable, str(Path(__file__).resolve()), "--point", str(S), dist, "--blocks", str(a.blocks), "--reps", str(a.reps), "--fs", str(a.fs)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(f"{S} streams, {dist}: no result within {a.timeout} s; stopping", flush=True)
                return 2
            line = next((l for l in r.stdout.splitlines() if l.startswith("RESULT ")), None)
            if r.returncode != 0 or line is None:
                print(f"{S} streams, {dist}: child failed with status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                return 2
            rec = json.loads(line[7:])
            mf = {k: [f / 1e6 for f in v] for k, v in rec["useful_frames_per_s"].items()}
            print(f"{S:6d} streams x {a.blocks} blocks, {dist:8s}: sum {rec['sum_blocks']} blocks = {rec['sum_blocks'] / rec['padded_blocks']:.1%} of the padded launch; "
                  f"ragged launch form {rec['form']}, chunk {rec['chunk_blocks']}, {rec['items']} items")
            for k, label in (("ragged", "(a) ragged    "), ("padded", "(b) padded    "), ("equal_work", "(c) equal work")):
                w, kt = rec["wall_s"][k], rec["kernel_s"][k]
                print(f"    {label}  useful {min(mf[k]):7.1f} .. {max(mf[k]):7.1f} M frames/s   wall {min(w) * 1e3:7.2f} .. {max(w) * 1e3:7.2f} ms   "
                      f"kernel {min(kt) * 1e3:7.2f} .. {max(kt) * 1e3:7.2f} ms   ({len(w)} repetitions)")
            best = {k: max(mf[k]) for k in mf}
            print(f"    ragged / equal work (best repetitions): {best['ragged'] / best['equal_work']:.3f};  ragged / padded: {best['ragged'] / best['padded']:.2f}x;  "
                  f"every ragged repetition faster than every padded one: {rec['ragged_faster_than_padded_every_rep']}", flush=True)
            if dist != "equal" and not rec["ragged_faster_than_padded_every_rep"]:
                missed.append((S, dist))
    print("GATE " + ("met: on uniform and one_long every ragged repetition beat every padded repetition" if not missed else f"MISSED at {missed}"))
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())

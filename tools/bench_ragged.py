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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,8192")
    ap.add_argument("--blocks", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per point (one child process each)")
    ap.add_argument("--point", nargs=2, metavar=("STREAMS", "DIST"), help="(internal) run one point in this process")
    a = ap.parse_args()
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

#!/usr/bin/env python3
"""Which decisions of the session wrapper has a set of inputs taken one way only -- and which only ever uniformly within a wavefront?

The sibling of tools/decision_coverage.py for webrtc_aecm_amd/csrc/aecm_flow_plan.h (FlowTick, FlowStartup, FlowEstBufDelay,
FlowDelayComp, FlowMoveFarReadPtr, FlowFarendCall, FlowBurstBegin, FlowResync, FlowMoveNear, FlowTickMixed / Calls / Packets,
FlowPacketCallSize, FlowLiveSlot).  Builds the host harness tests/sim/sim_flowcov.cpp with -O0 --coverage into a library of its own under
tests/_build/flowcov/, drives whole objects of sessions through it in a child python process (the counters are written when it
exits) the way the planning kernels drive them -- one lane per session, planned by the host's own planner (aecm_tick_plan.h), which takes a tick to the dense,
sparse, mixed, K-call or packets planner, far-end bursts in between -- and reads `gcov -b -c --json-format`.  Every run is a parity
run: the plans, executed as the tick kernels execute them, must move the sample tags SessionFlow<T> moves.

  --inputs existing   the call patterns today's CPU flow fuzz and session GPU tests feed: helpers.call_pattern (uniform objects of both
                      rates and call sizes, with and without bursts; per-session patterns as corpus_sessions.plan lays them out), the
                      sparse, mixed, K-call and packets golden patterns, the counter-wrap run of the flow fuzz (33 100 calls of 80
                      samples at 16 kHz, then 160), single sessions on random patterns like the fuzz's.  Not restated: re-initialisation
                      events (helpers.reconfiguration_events re-create a session: its wrapper starts over)
  --inputs corpus     tests/flow_corpus.py, every entry-point family
  --without NAME      leave a corpus scenario out (to see which decisions depend on it)

What counts.  Branch decisions as in decision_coverage.py: a pair of branch edges gcov reports on a source line of one of the functions
above; loop-condition lines (for / while / do) are left out.  FlowMin / FlowMax / FlowAsShort are shared by every clamp site and
excluded as functions: each clamp site is a decision marker instead.  Markers: aecm_flow_plan.h marks every decision with
AECM_FLOW_MARK(id, outcome) (nothing in any other build); the harness records the outcomes per tick and session.  A marker decision is
ONE-WAY when no session ever took one of its sides, and NEVER DIVERGENT when it went both ways but in no launch did two different
sessions of one wavefront -- 64 consecutive session ids from a multiple of 64, the mapping of all five planners -- take different
sides (any evaluation of a lane in the launch counts).  The burst kernel runs one wavefront per session: its decisions (BB_*, and the
FC_* / DC_* / MRP_* evaluations made inside it) cannot diverge there; the same decisions do when a tick's planner makes them.  In
place of the two data-dependent loops' conditions, the trip counts that occurred: blocks per frame (1 or 2), and calls per launch and
lane that the call loop left with `continue` (the start-up phase).
"""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import json
import os
import re
import shutil
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "webrtc_aecm_amd" / "csrc"
OUT = ROOT / "tests" / "_build" / "flowcov"
SRC = ROOT / "tests" / "sim" / "sim_flowcov.cpp"
DEPS = [SRC, CSRC / "aecm_flow_plan.h", CSRC / "aecm_flow_clean.h", CSRC / "aecm_tick_plan.h", CSRC / "aecm_session_flow.h", CSRC / "aecm_state.h"]
FLOW_FUNCTIONS = {"FlowTick", "FlowStartup", "FlowEstBufDelay", "FlowDelayComp", "FlowMoveFarReadPtr", "FlowFarendCall", "FlowBurstBegin", "FlowResync",
                  "FlowMoveNear", "FlowTickMixed", "FlowTickCalls", "FlowTickPackets", "FlowPacketCallSize", "FlowLiveSlot"}
WAVE = 64
SHARDS = 10                                     # child processes of a measurement (each runs every tenth object)
# evaluated once per iteration of a constant loop with a wave-uniform operand (FlowLiveSlot: w < wave, the lane's wavefront within its
# workgroup): every lane of a wavefront takes the same side in every evaluation, so "any evaluation counts" would call it divergent
UNIFORM_PER_EVALUATION = ("LS_WAVE_BEFORE",)


def tools_missing(coverage=True):
    return [t for t in (("g++", "gcov") if coverage else ("g++",)) if shutil.which(t) is None]


def lib_path(coverage):
    return OUT / ("cov" if coverage else "plain") / "libaecm_flowcov.so"


def build(coverage=True):
    so = lib_path(coverage)
    if so.exists() and all(so.stat().st_mtime >= p.stat().st_mtime for p in DEPS):
        return so
    shutil.rmtree(so.parent, ignore_errors=True)
    so.parent.mkdir(parents=True)
    flags = ["-std=c++17", "-fwrapv", "-fPIC", f"-I{CSRC}"] + (["-O0", "--coverage", "-fprofile-update=atomic"] if coverage else ["-O2"])
    obj = so.parent / "sim_flowcov.o"
    subprocess.check_call(["g++", *flags, "-c", str(SRC), "-o", str(obj)])
    tmp = so.with_suffix(f".{os.getpid()}.tmp")
    subprocess.check_call(["g++", *(["--coverage"] if coverage else []), "-shared", str(obj), "-o", str(tmp)])
    os.replace(tmp, so)
    return so


def family_names():
    """The kernel families of a tick by number: the one list, AECM_TICK_FAMILIES of aecm_tick_plan.h (TickFamily), read from the source."""
    line = re.search(r"^#define AECM_TICK_FAMILIES\(X\)(.*)$", (CSRC / "aecm_tick_plan.h").read_text(), re.M).group(1)
    return tuple(re.findall(r"X\((\w+)\)", line))


KERNELS = family_names()


class Harness:
    def __init__(self, coverage=False):
        self.lib = l = C.CDLL(str(build(coverage)))
        l.flowcov_decision_name.restype = C.c_char_p
        l.flowcov_run.restype = C.c_int64
        self.D, self.F = l.flowcov_decisions(), l.flowcov_fields()
        self.names = [l.flowcov_decision_name(i).decode() for i in range(self.D)]

    def run(self, sch):
        """A schedule (tests/flow_corpus.py: schedule()) through the harness.  Returns dict(first_difference (-1: none), detail, start[S, 32],
        regs[T, S, F], marks[T, 2, S, D] uint8 ([:, 0] the planning launches, [:, 1] the burst launches before them), kernels[T], continues[T, S])."""
        T, S = sch["flags"].shape
        a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)
        kind = a(np.full(T, sch["kind"]) if np.ndim(sch["kind"]) == 0 else sch["kind"], np.int32)
        n_t = a(np.full(T, sch["n"]) if np.ndim(sch["n"]) == 0 else sch["n"], np.int32)
        calls = a(np.full(T, sch["K"]) if np.ndim(sch["K"]) == 0 else sch["K"], np.int32)
        blen = a(np.full(T, sch.get("burst_len", 80)), np.int32)
        z = lambda k, dt: a(sch[k] if k in sch else np.zeros(S), dt)
        rates, flags, ms, burst = a(sch["rates"], np.int32), a(sch["flags"], np.uint8), a(sch["ms"], np.int16), a(sch.get("burst", np.zeros((T, S))), np.uint8)
        preroll, preroll_ms, far_off, frm_off = z("preroll", np.int32), a(sch.get("preroll_ms", np.full(S, 40)), np.int16), z("far_off", np.uint32), z("frm_off", np.uint32)
        start = np.zeros((S, 32), np.int32)
        regs = np.zeros((T, S, self.F), np.int32)
        marks = np.zeros((T, 2, S, self.D), np.uint8)
        kernels = np.zeros(T, np.int32)
        cont = np.zeros((T, S), np.uint8)
        detail = np.zeros(2, np.int64)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        first = self.lib.flowcov_run(S, T, int(sch["fs"]), int(bool(sch.get("force"))), p(rates), p(kind), p(n_t), p(calls), p(flags), p(ms), p(burst), p(blen),
                                     p(preroll), p(preroll_ms), p(far_off), p(frm_off), p(start), p(regs), p(marks), p(kernels), p(cont), p(detail))
        return dict(first_difference=int(first), detail=[int(x) for x in detail], start=start, regs=regs, marks=marks, kernels=kernels, continues=cont)


# ---- the record of outcomes -----------------------------------------------------------------------------------------------------
PLANNERS = tuple(k for k in KERNELS if k not in ("nothing", "split"))      # (the harness passes no clean plane: no split tick)


def tally(res, K):        # K[T]: call pairs per tick and session (an ordinary tick: 1, though a split tick makes two)
    """Per launch kind of one run (the five planners, and "burst": aecm_buffer_farend_kernel) and per decision: lane-launches that went
    false, that went true, and whether some launch had two different sessions of one wavefront on different sides.  Also the call
    loop's trip counts as (calls per launch, continues)."""
    out = {}
    for name in PLANNERS + ("burst",):
        if name == "burst":
            m = res["marks"][:, 1]
        else:
            m = res["marks"][res["kernels"] == KERNELS.index(name), 0]
        if not m.any():
            continue
        T, S, D = m.shape
        went_f, went_t = (m & 1) != 0, (m & 2) != 0
        pad = (-S) % WAVE
        wf = np.pad(went_f, ((0, 0), (0, pad), (0, 0))).reshape(T, -1, WAVE, D)
        wt = np.pad(went_t, ((0, 0), (0, pad), (0, 0))).reshape(T, -1, WAVE, D)
        cf, ct, both = wf.sum(axis=2), wt.sum(axis=2), (wf & wt).sum(axis=2)
        div = (cf >= 1) & (ct >= 1) & ~((cf == 1) & (ct == 1) & (both == 1))      # (one lane that took both sides alone is no divergence)
        if name == "burst":
            div[:] = False                                                        # one wavefront per session: nothing diverges
        out[name] = dict(false=went_f.sum(axis=(0, 1)), true=went_t.sum(axis=(0, 1)), divergent=div.any(axis=(0, 1)))
    live = res["marks"][:, 0].any(axis=2)
    t, s = np.nonzero(live)
    return out, sorted({(int(k), int(c)) for k, c in zip(K[t], res["continues"][t, s])})


def merge(tallies, names):
    """{launch kind: {decision: dict(false, true, divergent)}} over runs; "all": the sum, divergent in some planner."""
    acc = {k: {n: dict(false=0, true=0, divergent=False) for n in names} for k in PLANNERS + ("burst", "all")}
    loops = set()
    for per_kernel, trips in tallies:
        loops |= set(map(tuple, trips))
        for kernel, t in per_kernel.items():
            for i, n in enumerate(names):
                for dst in (acc[kernel][n], acc["all"][n]):
                    dst["false"] += int(t["false"][i])
                    dst["true"] += int(t["true"][i])
                    dst["divergent"] = dst["divergent"] or (bool(t["divergent"][i]) and n not in UNIFORM_PER_EVALUATION)
    return acc, sorted(loops)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def corpus_schedules(without=()):
    sys.path[:0] = [str(ROOT / "tests")]
    from flow_corpus import schedules
    return schedules(tuple(without))


def existing_schedules():
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import calls_helpers as ch
    import mixed_helpers as mh
    import packets_helpers as ph
    import sparse_helpers as sh
    from helpers import call_pattern
    NO_FAREND = 1
    out = []

    def uniform(name, fs, n, S, T, seed, bursts=False, per_session=False):
        flags, ms, burst = np.zeros((T, S), np.uint8), np.zeros((T, S), np.int16), np.zeros((T, S), np.uint8)
        for s in range(S):
            m, far = call_pattern(seed + 10 * s if per_session else seed, T, bursts=bursts)
            ms[:, s] = m
            flags[:, s] = np.where(far == 0, NO_FAREND, 0)
            burst[:, s] = np.maximum(far.astype(int) - 1, 0)
        out.append(dict(family=name, fs=fs, n=n, K=1, kind=0, force=False, rates=np.full(S, fs), flags=flags, ms=ms, burst=burst, burst_len=n))
    for fs, n in ((16000, 160), (8000, 80), (16000, 80), (8000, 160)):
        uniform(f"call_pattern fs{fs} f{n}", fs, n, 8, 500, 7)
    uniform("call_pattern bursts fs16000", 16000, 160, 8, 300, 15, bursts=True)
    uniform("call_pattern bursts fs8000", 8000, 80, 8, 300, 16, bursts=True)
    uniform("call_pattern per session fs16000", 16000, 160, 24, 1400, 0, per_session=True)
    uniform("call_pattern per session fs8000", 8000, 80, 24, 1400, 0, per_session=True)
    for name, (fs, n, seed) in sh.GOLDEN_CASES.items():
        flags, ms = sh.golden_pattern(fs, n, seed)
        out.append(dict(family=name, fs=fs, n=n, K=1, kind=0, force=False, rates=np.full(flags.shape[1], fs), flags=flags, ms=ms))
        out.append(dict(family=name + " forced", fs=fs, n=n, K=1, kind=0, force=True, rates=np.full(flags.shape[1], fs), flags=flags & ~np.uint8(4), ms=ms))
    for name, (seed, idle_p, bursts) in mh.GOLDEN_CASES.items():
        flags, ms = mh.mixed_pattern(seed, idle_p=idle_p)
        flags[3, 6] = 4                                                  # (the refused byte of that run belongs to a session that idles)
        out.append(dict(family=name, fs=mh.OBJECT_FS, n=160, K=1, kind=0, force=False, rates=mh.RATES, flags=flags, ms=ms,
                        burst=mh.burst_pattern(seed) if bursts else np.zeros(flags.shape, np.uint8), burst_len=80))
    for name, (fs, n, K, seed) in ch.GOLDEN_CASES.items():
        flags, ms = ch.golden_pattern(n, K, seed)
        out.append(dict(family=name, fs=fs, n=n, K=K, kind=1, force=False, rates=np.full(flags.shape[1], fs), flags=flags & np.uint8(5), ms=ms))
    for name, (fs, n, K, seed) in ph.GOLDEN_CASES.items():
        flags, ms = ph.golden_pattern(K, seed)
        out.append(dict(family=name, fs=fs, n=n, K=K, kind=2, force=False, rates=mh.RATES, flags=flags, ms=ms))
    # the flow fuzz: its counter-wrap run, and single sessions on random patterns
    T = 33300
    out.append(dict(family="fuzz counter wrap", fs=16000, n=np.where(np.arange(T) < 33100, 80, 160), K=1, kind=0, force=False, rates=np.full(1, 16000),
                    flags=np.zeros((T, 1), np.uint8), ms=(40 + np.arange(T) % 3).astype(np.int16)[:, None]))
    for k, fs in enumerate((16000, 8000, 16000, 8000)):
        rng = np.random.default_rng(50 + k)
        T, n = 2000, 160 if fs == 16000 or k == 3 else 80
        flags = ((rng.random((T, 1)) < 0.25) * 1 + (rng.random((T, 1)) < 0.3) * (2 if n == 160 else 0)).astype(np.uint8)
        ms = rng.integers(0, 501, (T, 1)).astype(np.int16) if k < 2 else np.where((np.arange(T) // 200) % 2, 480, 10).astype(np.int16)[:, None]
        ms[rng.random((T, 1)) < 0.03] = -300
        out.append(dict(family=f"fuzz-like single session {k}", fs=fs, n=n, K=1, kind=0, force=False, rates=np.full(1, fs), flags=flags, ms=ms))
    return out


def child(args):
    h = Harness(coverage=True)
    schedules = corpus_schedules(args.without) if args.inputs == "corpus" else existing_schedules()
    schedules = schedules[args.shard::args.shards]            # (the parent runs several children: gcov merges their counters)
    tallies, runs = [], []

    def one(sch):
        t0 = time.thread_time()
        res = h.run(sch)
        T = sch["flags"].shape[0]
        tl = tally(res, np.where(np.broadcast_to(sch["kind"], T) != 0, np.broadcast_to(sch["K"], T), 1))
        div = set()
        for t in tl[0].values():
            div |= {n for i, n in enumerate(h.names) if t["divergent"][i] and n not in UNIFORM_PER_EVALUATION}
        T, S = sch["flags"].shape
        return tl, dict(family=sch["family"], sessions=S, ticks=T, first_difference=res["first_difference"], detail=res["detail"],
                         kernels={KERNELS[k]: int((res["kernels"] == k).sum()) for k in range(len(KERNELS)) if (res["kernels"] == k).any()},
                         divergent=sorted(div), seconds=round(time.thread_time() - t0, 2))
    for sch in schedules:
        tl, run = one(sch)
        tallies.append(tl)
        runs.append(run)
    acc, loops = merge(tallies, h.names)
    Path(args.result).write_text(json.dumps(dict(runs=runs, kernels=acc, call_loop=loops)))


# ---- gcov -----------------------------------------------------------------------------------------------------------------------
_LOOP = re.compile(r"^(\}\s*)?(for|while|do)\b")


def _base_name(demangled):
    out, depth = [], 0
    for ch in demangled:
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif depth == 0:
            if ch == "(":
                break
            out.append(ch)
    return "".join(out).strip().split(" ")[-1].replace("aecm::", "")


def branch_decisions():
    """{key: [count of one edge, of the other]} of the Flow* functions, summed over template instantiations; keys as decision_coverage.py's:
    file|function|stripped source text|occurrence of the text in the function|branch pair.  Also {key: line number}."""
    d = lib_path(True).parent
    acc = {}
    for gcno in sorted(d.glob("*.gcno")):
        raw = subprocess.run(["gcov", "-b", "-c", "-m", "--json-format", "--stdout", str(gcno)], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
        doc = json.loads(gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw)
        for f in doc["files"]:
            if Path(f["file"]).name != "aecm_flow_plan.h":
                continue
            demangled = {fn["name"]: fn.get("demangled_name", fn["name"]) for fn in f.get("functions", [])}
            for ln in f["lines"]:
                br = [b for b in ln.get("branches", []) if not b.get("throw")]
                fn = _base_name(demangled.get(ln.get("function_name", ""), ln.get("function_name", "")))
                if len(br) < 2 or fn not in FLOW_FUNCTIONS:
                    continue
                counts = acc.setdefault((ln["line_number"], fn), [0] * len(br))
                if len(counts) == len(br):
                    for i, b in enumerate(br):
                        counts[i] += b["count"]
    source = (CSRC / "aecm_flow_plan.h").read_text().splitlines()
    out, lines, seen = {}, {}, {}
    for (line, fn), counts in sorted(acc.items()):
        text = " ".join(source[line - 1].split("//")[0].split())
        if _LOOP.match(text) or "AECM_FLOW_MARK" in text:
            continue
        occ = seen[fn, text] = seen.get((fn, text), -1) + 1
        for pair in range(0, len(counts), 2):
            key = f"aecm_flow_plan.h|{fn}|{text}|{occ}|{pair // 2}"
            out[key] = counts[pair:pair + 2] if pair + 2 <= len(counts) else counts[pair:] + [0]
            lines[key] = line
    return out, lines


def unmarked_lines(lines):
    """Source lines with a branch decision and no AECM_FLOW_MARK within the twelve lines above them (a decision somebody added without
    its marker would be invisible to the divergence record)."""
    source = (CSRC / "aecm_flow_plan.h").read_text().splitlines()
    return sorted({ln for ln in lines.values() if not any("AECM_FLOW_MARK" in source[k] for k in range(max(0, ln - 13), ln - 1))})


def measure(inputs, without=()):
    """Build, run the inputs in a child process, read the counters and the child's outcome record.  Returns dict(run, branches {key: counts},
    markers {name: false, true, divergent}, call_loop, lines)."""
    build(True)
    for g in lib_path(True).parent.glob("*.gcda"):
        g.unlink()
    shards = min(SHARDS, os.cpu_count() or 1)
    t0 = time.time()

    def shard(k):
        result = OUT / f"result_{os.getpid()}_{k}.json"
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--inputs", inputs, "--result", str(result), "--shard", str(k), "--shards", str(shards)]
        for w in without:
            cmd += ["--without", w]
        subprocess.check_call(cmd, cwd=ROOT)
        part = json.loads(result.read_text())
        result.unlink()
        return part
    with ThreadPoolExecutor(max_workers=shards) as ex:
        parts = list(ex.map(shard, range(shards)))
    run = dict(runs=[r for k in range(max(len(p["runs"]) for p in parts)) for p in parts if k < len(p["runs"]) for r in [p["runs"][k]]],
               call_loop=sorted({tuple(x) for p in parts for x in p["call_loop"]}), kernels={})
    for p in parts:                                        # counts add up, divergence in any run counts
        for kernel, dec in p["kernels"].items():
            for n, v in dec.items():
                cur = run["kernels"].setdefault(kernel, {}).setdefault(n, dict(false=0, true=0, divergent=False))
                cur["false"] += v["false"]
                cur["true"] += v["true"]
                cur["divergent"] = cur["divergent"] or v["divergent"]
    run["markers"] = run["kernels"]["all"]
    run["wall_seconds"] = time.time() - t0
    branches, lines = branch_decisions()
    return dict(run=run, branches=branches, markers=run["markers"], kernels=run["kernels"], call_loop=run["call_loop"], lines=lines)


def one_way_branches(rep):
    return sorted(k for k, v in rep["branches"].items() if min(v) == 0)


def one_way_markers(rep):
    return sorted(n for n, v in rep["markers"].items() if min(v["false"], v["true"]) == 0)


def never_divergent(rep):
    return sorted(n for n, v in rep["markers"].items() if min(v["false"], v["true"]) > 0 and not v["divergent"])


def undiverged_by_planner(rep):
    """{decision: [planners that evaluate it and never had it diverge within a wavefront, each with the reason's kind: "never true",
    "never false" or "uniform"]} -- the per-planner form of the never-divergent set: every planner is a compilation of its own."""
    out = {}
    for k in PLANNERS:
        for n, v in rep["kernels"][k].items():
            if v["false"] + v["true"] > 0 and not v["divergent"]:
                out.setdefault(n, []).append(f"{k}: {'never true' if v['true'] == 0 else 'never false' if v['false'] == 0 else 'uniform'}")
    return out


def format_report(title, rep):
    run = rep["run"]
    bad = [r for r in run["runs"] if r["first_difference"] != -1]
    lines = [f"== {title}: {len(run['runs'])} objects, wall {run['wall_seconds']:.0f} s; harness against SessionFlow<T> (tags of every block, output "
             f"sample, return code; the live lists): {'all equal' if not bad else bad}"]
    for r in run["runs"]:
        lines.append(f"   {r['family']:<36} {r['sessions']:>4} sessions {r['ticks']:>6} ticks  launches {r['kernels']}  decisions divergent within a wavefront: {len(r['divergent'])}")
    ob, om, nd = one_way_branches(rep), one_way_markers(rep), never_divergent(rep)
    lines.append(f"-- flow decisions: {len(rep['branches'])} branch decisions (gcov), {len(rep['markers'])} marked decisions")
    lines.append(f"-- one-way or never evaluated: {len(ob)} branch decisions, {len(om)} marked decisions")
    for k in ob:
        lines.append(f"   {rep['branches'][k][0]:>9} {rep['branches'][k][1]:>9}  {k}")
    for n in om:
        lines.append(f"   {rep['markers'][n]['false']:>9} {rep['markers'][n]['true']:>9}  marker {n}")
    lines.append(f"-- both ways, never divergent within a wavefront: {len(nd)} marked decisions")
    for n in nd:
        lines.append(f"   {rep['markers'][n]['false']:>9} {rep['markers'][n]['true']:>9}  marker {n}")
    ub = undiverged_by_planner(rep)
    lines.append(f"-- per planner (each is a compilation of its own): decisions a planner evaluates but never divergently: {sum(len(v) for v in ub.values())} (decision, planner) pairs")
    for n in sorted(ub):
        lines.append(f"   {n:<24} {'; '.join(ub[n])}")
    tb = rep["markers"]["T_TWO_BLOCKS"]
    lines.append(f"-- loops: blocks per frame: 1 x {tb['false']}, 2 x {tb['true']} (lane-launches); calls a lane's call loop left with `continue`, as "
                 f"(calls per launch, continues): {[tuple(x) for x in rep['call_loop']]}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--inputs", choices=("existing", "corpus"), default="corpus")
    ap.add_argument("--without", action="append", default=[])
    ap.add_argument("--json", help="write the one-way and never-divergent sets here (the form of tests/flow_allowlist.json, reasons empty)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--result", help=argparse.SUPPRESS)
    ap.add_argument("--shard", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--shards", type=int, default=1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if tools_missing():
        sys.exit(f"missing: {tools_missing()}")
    rep = measure(args.inputs, args.without)
    print(format_report(f"--inputs {args.inputs}" + "".join(f" --without {w}" for w in args.without), rep))
    if rep["lines"] and unmarked_lines(rep["lines"]):
        print(f"!! decisions without a marker at aecm_flow_plan.h lines {unmarked_lines(rep['lines'])}")
    if args.json:
        Path(args.json).write_text(json.dumps(dict(one_way=[dict(key=k, reason="") for k in one_way_branches(rep) + ["marker " + n for n in one_way_markers(rep)]],
                                                   never_divergent=[dict(key="marker " + n, reason="") for n in never_divergent(rep)]), indent=1) + "\n")


if __name__ == "__main__":
    main()

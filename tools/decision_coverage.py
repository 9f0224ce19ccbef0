#!/usr/bin/env python3
"""Which conditionals of the block path has a set of inputs taken one way only?

Builds oracle/aecm_oracle.c and the lane simulator's block DSP (tests/sim/sim_lib.cpp over webrtc_aecm_amd/csrc/aecm_wave.h and
aecm_ops.h) with -O0 --coverage into libraries of their own under tests/_build/cov/, runs the inputs through them in a child
python process (the counters are written when it exits), reads `gcov -b -c --json-format` and reports every conditional that
went one way only, or was never evaluated.  The child also compares every simulator run with the oracle, outputs and digests,
so a coverage run is a parity run.

  --inputs existing   what the GPU block tests feed today (helpers.adversarial_cases, the 64 x 2 048 block-parity streams of
                      both rates, the lean mix, the hostile clean kinds, the control case, the golden block vectors); the
                      simulator gets a sample of the long synth streams (--sim-sample, 10 of 64 per rate)
  --inputs corpus     tests/block_corpus.py
  --without NAME      leave a corpus case out (to see which decisions depend on it)

Families.  The kernel source is instantiated per kernel family with different compile-time gates; the simulator has three of
these instantiations, each built and counted apart:
  plain   BlockEngine<SimWave, false>, lean forms off (one wavefront per stream, pipelined, ragged, tick kernels)
  lean    BlockEngine<SimWave, false>, lean forms on (-DAECM_LEAN_POLICY_DEFAULT=1: the chunk queue)
  clean   BlockEngine<SimWave, true> (every kernel with a clean input), fed the inputs that carry one
The role split (tests/sim/sim_roles.cpp) runs the same BlockEngine members stage by stage and the tick bodies are simulated on
sample tags without the DSP (tests/sim/sim_calls.cpp), so neither adds a decision of aecm_wave.h; they are not built here.

What counts.  A decision is a pair of branch edges gcov reports on a source line (a line with `a && b` has two).  Edges of
exceptions, lines with `if constexpr`, loop conditions (for / while / do lines) and the precondition audits of aecm_ops.h
(`if (...) aecm_*_violation(...)`: assertions, which the checked build counts on the device) are left out.  Vector selects
(W::select, per-lane arithmetic) are no branches on the CPU either: gcov cannot see them, the parity of outputs and digests
is what checks them.  Counts are summed over template instantiations.  Keys are (file, function, stripped source text,
occurrence of that text in the function, branch pair): they survive edits that move lines.
"""
from __future__ import annotations

import argparse
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

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "webrtc_aecm_amd" / "csrc"
COV = ROOT / "tests" / "_build" / "cov"
FAMILIES = ("plain", "lean", "clean")
SIM_FLAGS = ["-O0", "--coverage", "-fprofile-update=atomic", "-std=c++17", "-fwrapv", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
             f"-I{CSRC}", f"-I{ROOT / 'tests' / 'sim'}"]
SIM_SOURCES = [ROOT / "tests" / "sim" / "sim_lib.cpp", CSRC / "aecm_host_state.cpp"]
SIM_DEPS = SIM_SOURCES + [ROOT / "tests" / "sim" / "wave_sim.h", ROOT / "tests" / "sim" / "sim_stream.h", CSRC / "aecm_wave.h", CSRC / "aecm_ops.h",
                          CSRC / "aecm_state.h", CSRC / "aecm_host_state.h", CSRC / "aecm_tables.h"]
ORACLE_SRC = ROOT / "oracle" / "aecm_oracle.c"
# the oracle's functions that aecm_oracle_process_block never reaches (lifetime, configuration, digest, the stream loop, the state
# image door -- tests/test_state_injection.py pins that one word for word)
ORACLE_NOT_BLOCK_PATH = {"aecm_oracle_create", "aecm_oracle_free", "aecm_oracle_init", "aecm_oracle_set_config", "aecm_oracle_control",
                         "aecm_oracle_init_echo_path", "aecm_oracle_get_echo_path", "aecm_oracle_digest", "aecm_oracle_get_stats",
                         "aecm_oracle_process_stream", "fnv_step", "hash_bytes", "aecm_oracle_import_image", "aecm_oracle_export_image", "bitrev6"}
KERNEL_FILES = ("aecm_wave.h", "aecm_ops.h")


def tools_missing():
    return [t for t in ("gcc", "g++", "gcov") if shutil.which(t) is None]


def lib_path(family):
    return COV / family / ("libaecm_cov_oracle.so" if family == "oracle" else f"libaecm_cov_sim_{family}.so")


def build(verbose=False):
    """tests/_build/cov/<family>/: objects, .gcno and the library of each family.  Rebuilt when a source is newer."""
    def one(family):
        so, d = lib_path(family), COV / family
        deps = [ORACLE_SRC, ORACLE_SRC.with_suffix(".h"), ROOT / "oracle" / "aecm_oracle_tables.h"] if family == "oracle" else SIM_DEPS
        if so.exists() and all(so.stat().st_mtime >= p.stat().st_mtime for p in deps + [Path(__file__)]):
            return
        shutil.rmtree(d, ignore_errors=True)
        d.mkdir(parents=True)
        if family == "oracle":
            obj = d / "aecm_oracle.o"
            subprocess.check_call(["gcc", "-O0", "--coverage", "-fprofile-update=atomic", "-std=c11", "-fPIC", "-fwrapv", "-c", str(ORACLE_SRC), "-o", str(obj)])
            subprocess.check_call(["gcc", "--coverage", "-shared", str(obj), "-o", str(so)])
            return
        flags = SIM_FLAGS + [f"-DAECM_LEAN_POLICY_DEFAULT={1 if family == 'lean' else 0}"]
        objs = []
        for src in SIM_SOURCES:
            objs.append(str(d / (src.name + ".o")))
            subprocess.check_call(["g++", *flags, "-c", str(src), "-o", objs[-1]])
        subprocess.check_call(["g++", "--coverage", "-shared", *objs, "-o", str(so)])
    t0 = time.time()
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(one, ("oracle",) + FAMILIES))
    if verbose:
        print(f"coverage libraries built in {time.time() - t0:.1f} s", file=sys.stderr)


# ---- the child: run the inputs, compare simulator and oracle ------------------------------------------------------------------
def _inputs(which, without, sim_sample):
    """[(case dict, run on the simulator too)]"""
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import numpy as np
    if which == "corpus":
        from block_corpus import corpus_cases
        return [(c, True) for c in corpus_cases(without=tuple(without))]
    from helpers import adversarial_cases, adversarial_clean_cases, golden_files, stream_config
    from webrtc_aecm_amd.synth import synth_pair
    cases = []

    def add(name, far, near, fs, cng, em, sim=True, **kw):
        cases.append((dict(dict(name=name, far=far, near=near, fs=fs, cng=cng, echo_mode=em, clean=None, path=None, control=None), **kw), sim))
    for it, c in enumerate(adversarial_cases()):
        add(f"adversarial{it}", c["far"], c["near"], c["fs"], c["cng"], c["echo_mode"], path=c["path"])
    for fs in (16000, 8000):
        for s in range(64):
            far, near = synth_pair(1000 + s, 2048, fs)
            add(f"parity{fs}_{s}", far, near, fs, *stream_config(s), sim=s < sim_sample)
    import test_gpu_lean_block as L
    for fs in (16000, 8000):
        cfg, far, near = L._mix(fs)
        for s in range(L.S):
            add(f"leanmix{fs}_{s}", far[s].copy(), near[s].copy(), fs, *cfg[s])
    for k, c in enumerate(adversarial_clean_cases(1100)):
        add(f"hostile_clean{k}", c["far"], c["near"], c["fs"], c["cng"], c["echo_mode"], path=c["path"], clean=c["clean"])
    for s in (5, 6, 7, 8):
        far, near = synth_pair(s, 800, 16000)
        add(f"control{s}", far, near, 16000, 1, 3, control=(7, 0))
    for f in golden_files("block_"):
        g = np.load(f)
        far, near = synth_pair(int(g["seed"]), int(g["n_blocks"]), int(g["fs"]), str(g["profile"]) or None)
        add(f.stem, far, near, int(g["fs"]), int(g["cng"]), int(g["echo_mode"]))
    return cases


def child(args):
    import ctypes as C

    import numpy as np
    i16p = np.ctypeslib.ndpointer(dtype=np.int16, flags="C_CONTIGUOUS")
    u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
    cases = _inputs(args.inputs, args.without, args.sim_sample)
    orc = C.CDLL(str(lib_path("oracle")))
    orc.aecm_oracle_create.restype = C.c_void_p
    for fn, at in (("aecm_oracle_free", [C.c_void_p]), ("aecm_oracle_init", [C.c_void_p, C.c_int]), ("aecm_oracle_set_config", [C.c_void_p, C.c_int, C.c_int]),
                   ("aecm_oracle_control", [C.c_void_p, C.c_int, C.c_int]), ("aecm_oracle_init_echo_path", [C.c_void_p, i16p]),
                   ("aecm_oracle_process_block", [C.c_void_p, i16p, i16p, C.c_void_p, i16p]),
                   ("aecm_oracle_process_stream", [C.c_void_p, i16p, i16p, i16p, C.c_size_t]), ("aecm_oracle_digest", [C.c_void_p, u32p])):
        getattr(orc, fn).argtypes = at
    sims = {}
    for fam in FAMILIES:
        l = C.CDLL(str(lib_path(fam)))
        l.sim_create.restype = C.c_void_p
        l.sim_create.argtypes = [C.c_int, C.c_int, C.c_int]
        l.sim_free.argtypes = [C.c_void_p]
        l.sim_control.argtypes = [C.c_void_p, C.c_int, C.c_int]
        l.sim_set_echo_path.argtypes = [C.c_void_p, i16p]
        l.sim_process.argtypes = [C.c_void_p, i16p, i16p, C.c_void_p, i16p, C.c_int]
        l.sim_digest.argtypes = [C.c_void_p, u32p]
        sims[fam] = l

    def run_oracle(c):
        h = orc.aecm_oracle_create()
        assert orc.aecm_oracle_init(h, c["fs"]) == 0 and orc.aecm_oracle_set_config(h, c["cng"], c["echo_mode"]) == 0
        if c["path"] is not None:
            orc.aecm_oracle_init_echo_path(h, np.ascontiguousarray(c["path"]))
        if c["control"] is not None:
            orc.aecm_oracle_control(h, *c["control"])
        far, near = np.ascontiguousarray(c["far"]), np.ascontiguousarray(c["near"])
        out = np.empty_like(near)
        if c["clean"] is None:
            orc.aecm_oracle_process_stream(h, far, near, out, near.size // 64)
        else:
            clean = np.ascontiguousarray(c["clean"])
            for b in range(near.size // 64):
                sl = slice(b * 64, (b + 1) * 64)
                orc.aecm_oracle_process_block(h, far[sl], near[sl], clean[sl].ctypes.data_as(C.c_void_p), out[sl])
        d = np.zeros(24, np.uint32)
        orc.aecm_oracle_digest(h, d)
        orc.aecm_oracle_free(h)
        return out, d

    def run_sim(l, c, launches):
        h = l.sim_create(c["fs"], c["cng"], c["echo_mode"])
        assert h
        if c["path"] is not None:
            l.sim_set_echo_path(h, np.ascontiguousarray(c["path"]))
        if c["control"] is not None:
            l.sim_control(h, *c["control"])
        far, near = np.ascontiguousarray(c["far"]), np.ascontiguousarray(c["near"])
        clean = None if c["clean"] is None else np.ascontiguousarray(c["clean"])
        out = np.empty_like(near)
        n = near.size // 64
        step = -(-n // launches)
        for b in range(0, n, step):                       # several launches: the state goes through store_state / load_state
            e = min(n, b + step)
            l.sim_process(h, far[b * 64:e * 64], near[b * 64:e * 64], None if clean is None else clean[b * 64:e * 64].ctypes.data_as(C.c_void_p),
                          out[b * 64:e * 64], e - b)
        d = np.zeros(24, np.uint32)
        l.sim_digest(h, d)
        l.sim_free(h)
        return out, d

    jobs = []
    for k, (c, sim) in enumerate(cases):
        jobs.append(("oracle", k))
        if sim:
            jobs.extend((fam, k) for fam in (("clean",) if c["clean"] is not None else ("plain", "lean")))
    seconds = {f: 0.0 for f in ("oracle",) + FAMILIES}
    blocks = {f: 0 for f in ("oracle",) + FAMILIES}

    def do(job):
        fam, k = job
        c = cases[k][0]
        t0 = time.thread_time()
        res = run_oracle(c) if fam == "oracle" else run_sim(sims[fam], c, 1 + k % 3)
        return fam, k, res, time.thread_time() - t0
    results = {}
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 2)) as ex:
        for fam, k, res, dt in ex.map(do, jobs):
            results[fam, k] = res
            seconds[fam] += dt
            blocks[fam] += cases[k][0]["near"].size // 64
    mismatches = []
    for (fam, k), (out, d) in results.items():
        if fam == "oracle":
            continue
        eo, ed = results["oracle", k]
        if not np.array_equal(out, eo):
            mismatches.append(dict(case=cases[k][0]["name"], family=fam, first_block=int(np.nonzero(out != eo)[0][0]) // 64))
        elif not np.array_equal(d, ed):
            mismatches.append(dict(case=cases[k][0]["name"], family=fam, digest_words=[int(i) for i in np.nonzero(d != ed)[0]]))
    Path(args.result).write_text(json.dumps(dict(cases=[c["name"] for c, _ in cases], cpu_seconds=seconds, blocks=blocks, mismatches=mismatches,
                                                 sim_runs=sum(1 for f, _ in results if f != "oracle"))))


# ---- gcov ---------------------------------------------------------------------------------------------------------------------
_ENGINE = re.compile(r"BlockEngine<aecm::SimWave, (true|false)>")
_AUDIT = re.compile(r"\baecm_\w+_violation\(")      # aecm_ops.h: precondition audits of the checked build, assertions and no decisions
_LOOP = re.compile(r"^(\}\s*)?(for|while|do)\b")


def _base_name(demangled):
    """aecm::BlockEngine<SimWave, false>::noise_bin<int, true>(...) -> BlockEngine::noise_bin"""
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
    name = "".join(out).strip().split(" ")[-1]
    return name.replace("aecm::", "").replace("(anonymous namespace)::", "")


def _gcov(family):
    d = COV / family
    res = []
    for gcno in sorted(d.glob("*.gcno")):
        p = subprocess.run(["gcov", "-b", "-c", "-m", "--json-format", "--stdout", str(gcno)], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        raw = p.stdout
        res.append(json.loads(gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw))
    return res


def decisions(family):
    """{key: [count of the one edge, count of the other]} of a family's block path, summed over instantiations."""
    acc = {}            # (file, line, function) -> list of branch counts
    for doc in _gcov(family):
        for f in doc["files"]:
            name = Path(f["file"]).name
            if family == "oracle":
                if name != "aecm_oracle.c":
                    continue
            elif name not in KERNEL_FILES:
                continue
            demangled = {fn["name"]: fn.get("demangled_name", fn["name"]) for fn in f.get("functions", [])}
            for ln in f["lines"]:
                br = [b for b in ln.get("branches", []) if not b.get("throw")]
                if len(br) < 2:
                    continue
                full = demangled.get(ln.get("function_name", ""), ln.get("function_name", ""))
                inst = _ENGINE.search(full)
                if inst and (inst.group(1) == "true") != (family == "clean"):
                    continue            # the library holds both BlockEngine<SimWave, kHasClean>: a family counts its own
                fn = _base_name(full)
                if family == "oracle" and fn in ORACLE_NOT_BLOCK_PATH:
                    continue
                counts = acc.setdefault((name, ln["line_number"], fn), [0] * len(br))
                if len(counts) == len(br):
                    for i, b in enumerate(br):
                        counts[i] += b["count"]
    sources = {"aecm_oracle.c": ORACLE_SRC.read_text().splitlines(), **{k: (CSRC / k).read_text().splitlines() for k in KERNEL_FILES}}
    out, seen = {}, {}
    for (name, line, fn), counts in sorted(acc.items()):
        text = " ".join(sources[name][line - 1].split("//")[0].split("/*")[0].split())
        if "if constexpr" in text or _LOOP.match(text) or _AUDIT.search(text):
            continue
        occ = seen[name, fn, text] = seen.get((name, fn, text), -1) + 1
        for pair in range(0, len(counts), 2):
            out[f"{name}|{fn}|{text}|{occ}|{pair // 2}"] = counts[pair:pair + 2] if pair + 2 <= len(counts) else counts[pair:] + [0]
    return out


def split_key(key):
    """(file, function, source text, occurrence, branch pair) of a key; the text may hold '|' itself."""
    name, fn, rest = key.split("|", 2)
    text, occ, pair = rest.rsplit("|", 2)
    return name, fn, text, int(occ), int(pair)


def one_way(dec):
    return {k: v for k, v in dec.items() if min(v) == 0}


def measure(inputs, without=(), sim_sample=10, verbose=False):
    """Build, run the inputs in a child process, read the counters.  Returns a dict: per family the decisions and the one-way
    ones, `kernel` = the three simulator families summed, the child's parity result and CPU seconds."""
    build(verbose)
    for fam in ("oracle",) + FAMILIES:
        for g in (COV / fam).glob("*.gcda"):
            g.unlink()
    result = COV / f"result_{os.getpid()}.json"
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--inputs", inputs, "--result", str(result), "--sim-sample", str(sim_sample)]
    for w in without:
        cmd += ["--without", w]
    t0 = time.time()
    subprocess.check_call(cmd, cwd=ROOT)
    run = json.loads(result.read_text())
    result.unlink()
    run["wall_seconds"] = time.time() - t0
    rep = dict(run=run, families={})
    for fam in ("oracle",) + FAMILIES:
        rep["families"][fam] = decisions(fam)
    kernel = {}
    for fam in FAMILIES:
        for k, v in rep["families"][fam].items():
            cur = kernel.setdefault(k, [0, 0])
            cur[0] += v[0]
            cur[1] += v[1]
    rep["kernel"] = kernel
    return rep


def one_way_entries(rep):
    """{key: sorted families in which the decision is one-way} -- the form of tests/decision_allowlist.json."""
    out = {}
    for fam in ("oracle",) + FAMILIES:
        for k in one_way(rep["families"][fam]):
            out.setdefault(k, []).append(fam)
    return out


def format_report(title, rep):
    run = rep["run"]
    lines = [f"== {title}: {len(run['cases'])} inputs, {run['sim_runs']} simulator runs, wall {run['wall_seconds']:.0f} s", "   CPU seconds / blocks per library: " +
             ", ".join(f"{f} {run['cpu_seconds'][f]:.0f} s / {run['blocks'][f]}" for f in ("oracle",) + FAMILIES),
             f"   simulator against oracle (outputs and digests): {'all equal' if not run['mismatches'] else run['mismatches']}"]
    for fam in ("oracle",) + FAMILIES:
        dec = rep["families"][fam]
        ow = one_way(dec)
        lines.append(f"-- {fam}: {len(dec)} decisions, {len(ow)} one-way")
        for k, v in ow.items():
            lines.append(f"   {v[0]:>9} {v[1]:>9}  {k}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--inputs", choices=("existing", "corpus"), default="corpus")
    ap.add_argument("--without", action="append", default=[])
    ap.add_argument("--sim-sample", type=int, default=10)
    ap.add_argument("--json", help="write the one-way entries here (the form of tests/decision_allowlist.json, reasons empty)")
    ap.add_argument("--counts", help="write every decision's counts per family here (JSON)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--result", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if tools_missing():
        sys.exit(f"missing: {tools_missing()}")
    rep = measure(args.inputs, args.without, args.sim_sample, verbose=True)
    print(format_report(f"--inputs {args.inputs}" + "".join(f" --without {w}" for w in args.without), rep))
    if args.json:
        Path(args.json).write_text(json.dumps([dict(key=k, families=f, reason="") for k, f in one_way_entries(rep).items()], indent=1) + "\n")
    if args.counts:
        Path(args.counts).write_text(json.dumps(rep["families"], indent=0))


if __name__ == "__main__":
    main()

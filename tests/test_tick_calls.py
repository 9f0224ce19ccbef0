"""Ticks of K call pairs (WebRtcAecmSessions_TickCalls) without a GPU: the index domain (aecm_flow_plan.h: FlowTickCalls) and the
sample movement of the two new kernels on sample tags (tests/sim/sim_calls.cpp), the public interface, the build of the new
units and the golden runs.  The GPU side: tests/test_gpu_tick_calls.py."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import calls_helpers as ch
import calls_sim
import sparse_helpers as sh

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"


def test_k_call_ticks_equal_k_calls_of_the_wrapper_on_sample_tags():
    """40 seeds x 1 500 ticks at both rates, n in {80, 160} in stretches, K drawn per tick from 1 .. 6, mixed with ordinary ticks
    (split calls too), underruns, bursts (also into idle ticks), idle stretches longer than the ring, ticks nobody makes, wrapping
    counters and msInSndCardBuf jumps that move the read pointer: every block input and every output sample carries the tag
    SessionFlow<T>, called K times, gives it; the state words equal those of the device model of ordinary ticks, ticked K times,
    after every tick (lag arithmetic with calls * n included); FlowStateDefect accepts every state, those between two calls too.
    And each case the kernel has to get right occurred."""
    total = dict.fromkeys(calls_sim.DETAIL, 0)
    for seed in range(40):
        for fs in (8000, 16000):
            tick, d = calls_sim.fuzz(seed, fs, 1500, 0xffffff00 if seed % 3 == 2 else 0)
            assert tick == -1, (seed, fs, tick, d)
            for k, v in d.items():
                total[k] = max(total[k], v) if k == "longest_idle_samples" else total[k] + v
    assert total["calls_ticks"] > 40000 and total["ordinary_ticks"] > 20000 and total["bursts"] > 5000 and total["blocks"] > 300000
    for case in ("nondirect_later", "spill_later", "startup_end_later", "stuffing_later", "no_block_calls", "nobody_ticks", "resyncs"):
        assert total[case] > 0, case
    assert total["longest_idle_samples"] > 8192


def test_lag_of_idle_k_call_ticks_is_that_of_the_single_ticks():
    for ticks, K, n in ((1, 2, 160), (7, 3, 80), (100, 6, 160), (5000, 5, 80), (40960, 6, 160)):
        lag, single = calls_sim.lag_after(ticks, K, n)
        assert lag == single == (ticks * K * n) % 40960 and lag % 80 == 0


def test_the_spill_recipe_of_the_gpu_test_spills_inside_a_tick():
    """calls_helpers.SPILL_RECIPE: the replay row moves at a call c > 0 of a K-call tick, it is row 1, and the recipe's K-call
    ticks reach it.  (With ONE ordinary tick ahead of the K-call ticks no row is ever spilled: the session is still in its
    start-up phase, farendOld[1] is the zeroed row.)"""
    r = ch.SPILL_RECIPE
    got = calls_sim.spill_recipe(r["fs"], r["pre_ticks"], r["calls"])
    assert got is not None and got["call"] > 0 and got["row"] == 1 and got["tick"] < r["k_ticks"], got
    assert calls_sim.spill_recipe(r["fs"], 1, r["calls"]) is None


def test_simulator_runs_stand_alone_under_sanitizers(tmp_path):
    """tests/sim/sim_calls.cpp has a main of its own: built with AddressSanitizer and UndefinedBehaviorSanitizer into a program
    and run, on the CPU."""
    exe = tmp_path / "sim_calls_san"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-fwrapv",
                           f"-I{ROOT / 'webrtc_aecm_amd' / 'csrc'}", str(ROOT / "tests" / "sim" / "sim_calls.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr[-2000:])


def test_symbols_are_declared_exported_and_bound():
    import webrtc_aecm_amd as aecm
    from webrtc_aecm_amd import build, ffi
    names = ["WebRtcAecmSessions_TickCalls", "WebRtcAecmSessions_TickCallsHost", "WebRtcAecmSessions_TickCallsAsync"]
    header = (ROOT / "include" / "aecm_batch.h").read_text()
    lib = ctypes.CDLL(str(build.build()))
    bound = aecm.load()
    for name in names:
        assert re.search(rf"\bint32_t {name}\(", header) and name in ffi.SESSIONS_SYMBOLS and hasattr(lib, name)
        assert len(getattr(bound, name).argtypes) == (14 if name.endswith("Async") else 12)
    assert "enum { AECM_SESSION_MAX_TICK_CALLS = 6 }" in header and ffi.SESSION_MAX_TICK_CALLS == 6
    assert hasattr(aecm.AecmSessions, "tick_calls_host") and hasattr(aecm.AecmSessions, "tick_calls_device")
    # what can be asked without a device: no object, no call
    for name in names:
        args = [None, None, None, None, None, 160, 160, 2, 40, None, None, None] + ([None, None] if name.endswith("Async") else [])
        assert getattr(bound, name)(*args) == -1


def test_new_units_are_built_like_the_others(tmp_path):
    """Both recipes list the two units; the tick kernel's unit gets the flags aecm_kernels.hip gets, the planning kernel's unit --
    one lane per session, divergent branches -- none of its own; both instantiations of the tick kernel and the planning kernel
    are in the code object, under names the dense tick kernel's pattern does not match; registers and scratch of the tick kernel
    (the code object's metadata) admit the 7 waves per SIMD it is built for, with at most a few spilled dwords."""
    from webrtc_aecm_amd import build, isa_census
    tick, plan = "aecm_tick_calls_kernels.hip", "aecm_tick_calls_plan_kernels.hip"
    assert tick in build.KERNEL_SOURCES and plan in build.KERNEL_SOURCES
    assert build.SOURCE_FLAGS[tick] == build.SOURCE_FLAGS["aecm_kernels.hip"] and plan not in build.SOURCE_FLAGS
    cmake = (ROOT / "CMakeLists.txt").read_text()
    assert tick in cmake and plan in cmake
    ours = isa_census.census_of_text(isa_census.disassemble(build.build()))
    for clean in (0, 1):
        assert len([k for k in ours if re.search(rf"aecm_tick_calls_kernelILb{clean}EEE", k)]) == 1
        assert len([k for k in ours if re.search(rf"aecm_tick_flow_kernelILb{clean}E", k)]) == 1
    assert len([k for k in ours if "aecm_flow_plan_calls_kernel" in k]) == 1
    lib = tmp_path / build.LIB.name
    lib.write_bytes(build.LIB.read_bytes())
    subprocess.run([isa_census._tool("llvm-objdump"), "--offloading", str(lib)], check=True, capture_output=True)
    meta = ""
    for obj in sorted(tmp_path.glob(lib.name + ".*amdgcn*gfx950*")):
        meta += subprocess.run([isa_census._tool("llvm-readelf"), "--notes", str(obj)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for block in re.split(r"\n\s*- \.agpr_count:", meta)[1:]:
        if "aecm_tick_calls_kernel" not in re.search(r"\.name:\s+(\S+)", block).group(1):
            continue
        sgpr, vgpr, scratch = (int(re.search(rf"\.{f}:\s+(\d+)", block).group(1)) for f in ("sgpr_count", "vgpr_count", "private_segment_fixed_size"))
        assert min(8, 512 // (-(-vgpr // 8) * 8), 800 // (-(-sgpr // 16) * 16 + 16)) >= 7 and scratch <= 16, (sgpr, vgpr, scratch)
        seen += 1
    assert seen == 2


@pytest.mark.parametrize("name", sorted(ch.GOLDEN_CASES))
def test_golden_runs_are_what_their_recipe_says(name):
    """tests/golden/sesscalls_*.npz (tools/gen_golden.py; run on the GPU by tests/test_gpu_tick_calls.py): 9 sessions x 48 calls,
    arrays only, the pattern the recipe gives, zeros and code 0 where a session sat out; where the unmodified reference is built,
    its instances -- K pairs per tick in order, not called in idle ticks -- give exactly the stored outputs, codes and echo paths."""
    from oracle import pyoracle
    path = GOLDEN / f"{name}.npz"
    assert path.stat().st_size < 150 * 1024
    g = np.load(path, allow_pickle=False)
    fs, n, K, seed = ch.GOLDEN_CASES[name]
    assert (int(g["fs"]), int(g["frame"]), int(g["calls"]), int(g["seed"])) == (fs, n, K, seed)
    flags, ms = ch.golden_pattern(n, K, seed)
    T = ch.GOLDEN_CALLS // K
    assert np.array_equal(g["flags"], flags) and np.array_equal(g["ms"], ms) and flags.shape == (T, ch.GOLDEN_S)
    assert not (flags & (sh.SPLIT_CALLS | 8)).any()
    idle = (flags & sh.IDLE) != 0
    out = g["out"].reshape(ch.GOLDEN_S, T, K * n)
    assert g["out"].dtype == np.int16 and not out[idle.T].any() and not g["codes"][idle].any() and out[~idle.T].any()
    assert 0.1 < idle.mean() < 0.35 and 12100 in g["codes"] and g["paths"].shape == (ch.GOLDEN_S, 65)
    if pyoracle.have_reference():
        far, near, _ = sh.signals(seed, ch.GOLDEN_S, ch.GOLDEN_CALLS * n, fs)
        eout, ecodes, refs = ch.run_reference(lambda: pyoracle.RefSession(fs, 1, 3), ch.calls_ops(K, n, flags, ms), ch.Feed(far, near))
        assert np.array_equal(eout, g["out"]) and np.array_equal(ecodes, g["codes"])
        assert np.array_equal(np.stack([r.get_echo_path()[1] for r in refs]), g["paths"])
        # and K ordinary calls per tick are the same calls: the per-call driver of the sparse tests on the expanded pattern
        f2, m2 = ch.per_call(K, flags, ms)
        sout, scodes, _ = sh.drive_reference(lambda: pyoracle.RefSession(fs, 1, 3), fs, f2, m2, np.full(T * K, n), far, near)
        assert np.array_equal(sout, g["out"]) and np.array_equal(scodes.reshape(T, K, -1).max(axis=1), g["codes"])

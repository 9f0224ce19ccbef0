"""Packet ticks (WebRtcAecmSessions_TickPackets) without a GPU: the index domain (aecm_flow_plan.h: FlowTickPackets) and the sample
movement of the two new kernels on sample tags (tests/sim/sim_packets.cpp), the public interface, the build of the new units, the
kernels that must not have moved, and the golden runs.  The GPU side: tests/test_gpu_tick_packets.py."""
import ctypes
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import calls_helpers as ch
import mixed_helpers as mh
import packets_helpers as ph
import packets_sim

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
NAMES = ["WebRtcAecmSessions_TickPackets", "WebRtcAecmSessions_TickPacketsHost", "WebRtcAecmSessions_TickPacketsAsync"]


def test_packet_ticks_equal_k_calls_at_the_sessions_rate_and_size_on_sample_tags():
    """24 seeds x 1 000 ticks of objects of both own rates holding sessions of both rates, 8 seeds of uniform objects (where a packet
    tick without half flags takes the K-call tick's launches): packet ticks (K = 1 .. 6, half flags per session in stretches),
    ordinary ticks (half and split calls), bursts, idle stretches longer than the ring, ticks nobody makes, wrapping start
    positions.  Every block input and every output sample carries the tag SessionFlow<T> gives when called K times at the session's
    rate and size; after every tick the flow words except F_NEAR_LAG equal those of the device model of ordinary mixed ticks ticked
    K times on re-laid rows, and the snapshot models of the two are equal; FlowStateDefect accepts every state, those between two
    calls too.  And each case the kernels have to get right occurred."""
    total = dict.fromkeys(packets_sim.DETAIL, 0)
    for seed in range(32):
        tick, d = packets_sim.fuzz(seed, 6, 1000, packets_sim.MIXED_RATES if seed < 24 else packets_sim.UNIFORM)
        assert tick == -1, (seed, tick, d)
        for k, v in d.items():
            total[k] = max(total[k], v) if k == "longest_idle_samples" else total[k] + v
    assert total["packet_ticks"] > 10000 and total["ordinary_ticks"] > 5000 and total["calls_shaped_ticks"] > 2000 and total["bursts"] > 5000
    assert total["blocks"] > 300000 and total["half_packets"] > 10000 and total["full_8k_packets"] > 1000
    for case in ("half_spill_later", "startup_end_later", "resync_after_idle", "half_and_full", "nondirect_later", "no_block_calls", "nobody_ticks"):
        assert total[case] > 0, case
    assert total["longest_idle_samples"] > 8192


def test_lag_of_half_call_packets():
    """After T all-half packet ticks of K calls a session lies (T K 80) mod 40 960 behind the object."""
    for ticks, K in ((1, 2), (7, 3), (100, 6), (5000, 5), (40960, 6)):
        lag = packets_sim.lag_after(ticks, K)
        assert lag == (ticks * K * 80) % 40960 and lag % 80 == 0


def test_the_spill_recipe_of_the_gpu_test_spills_inside_a_packet():
    """calls_helpers.SPILL_RECIPE on an 8 kHz session making half calls: the replay row moves at a call c > 0 of a packet, it is row 1,
    and the recipe's packets reach it."""
    r = ch.SPILL_RECIPE
    got = packets_sim.spill_recipe(8000, r["pre_ticks"], r["calls"])
    assert got is not None and got["call"] > 0 and got["row"] == 1 and got["tick"] < r["k_ticks"], got
    assert packets_sim.spill_recipe(8000, 1, r["calls"]) is None


def test_simulator_runs_stand_alone_under_sanitizers(tmp_path):
    """tests/sim/sim_packets.cpp has a main of its own: built with AddressSanitizer and UndefinedBehaviorSanitizer into a program
    and run, on the CPU."""
    exe = packets_sim.standalone(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr[-2000:])


def test_symbols_are_declared_exported_and_bound():
    import webrtc_aecm_amd as aecm
    from webrtc_aecm_amd import build, ffi
    header = (ROOT / "include" / "aecm_batch.h").read_text()
    lib = ctypes.CDLL(str(build.build()))
    bound = aecm.load()
    for name in NAMES:
        assert re.search(rf"\bint32_t {name}\(", header) and name in ffi.SESSIONS_SYMBOLS and hasattr(lib, name)
        assert len(getattr(bound, name).argtypes) == (14 if name.endswith("Async") else 12)
    assert hasattr(aecm.AecmSessions, "tick_packets_host") and hasattr(aecm.AecmSessions, "tick_packets_device")
    assert "left for later" not in header
    # what can be asked without a device: no object, no call
    for name in NAMES:
        args = [None, None, None, None, None, 320, 160, 2, 40, None, None, None] + ([None, None] if name.endswith("Async") else [])
        assert getattr(bound, name)(*args) == -1


def _kernel_metadata(tmp_path):
    """{kernel name: (sgpr, vgpr, scratch bytes)} of the shipped library's gfx950 code object."""
    from webrtc_aecm_amd import build, isa_census
    lib = tmp_path / build.LIB.name
    lib.write_bytes(build.build().read_bytes())
    subprocess.run([isa_census._tool("llvm-objdump"), "--offloading", str(lib)], check=True, capture_output=True)
    meta = ""
    for obj in sorted(tmp_path.glob(lib.name + ".*amdgcn*gfx950*")):
        meta += subprocess.run([isa_census._tool("llvm-readelf"), "--notes", str(obj)], check=True, capture_output=True, text=True).stdout
    found = {}
    for block in re.split(r"\n\s*- \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        found[name] = tuple(int(re.search(rf"\.{f}:\s+(\d+)", block).group(1)) for f in ("sgpr_count", "vgpr_count", "private_segment_fixed_size"))
    return found


def test_new_units_are_built_like_their_siblings(tmp_path):
    """Both recipes list the two new units; the tick kernel's unit gets the flags aecm_tick_calls_kernels.hip gets, the planning
    kernel's unit -- one lane per session -- none of its own; both instantiations of the tick kernel and the planning kernel are in
    the code object; registers admit the 7 waves per SIMD the kernel is built for; its scratch exceeds that of
    aecm_tick_calls_kernel<clean> of the same build by at most 16 bytes (two more wave-uniform values, which should stay scalar)."""
    from webrtc_aecm_amd import build, isa_census
    tick, plan = "aecm_tick_packets_kernels.hip", "aecm_tick_packets_plan_kernels.hip"
    assert tick in build.KERNEL_SOURCES and plan in build.KERNEL_SOURCES
    assert build.SOURCE_FLAGS[tick] == build.SOURCE_FLAGS["aecm_tick_calls_kernels.hip"] and plan not in build.SOURCE_FLAGS
    cmake = (ROOT / "CMakeLists.txt").read_text()
    assert tick in cmake and plan in cmake
    ours = isa_census.census_of_text(isa_census.disassemble(build.build()))
    for clean in (0, 1):
        assert len([k for k in ours if re.search(rf"aecm_tick_packets_kernelILb{clean}EEE", k)]) == 1
    assert len([k for k in ours if "aecm_flow_plan_packets_kernel" in k]) == 1
    meta = _kernel_metadata(tmp_path)
    for clean in (0, 1):
        (name, (sgpr, vgpr, scratch)), = [(k, v) for k, v in meta.items() if f"aecm_tick_packets_kernelILb{clean}E" in k]
        (_, (_, _, calls_scratch)), = [(k, v) for k, v in meta.items() if f"aecm_tick_calls_kernelILb{clean}E" in k]
        print(name, "sgpr", sgpr, "vgpr", vgpr, "scratch", scratch, "aecm_tick_calls_kernel scratch", calls_scratch)
        assert min(8, 512 // (-(-vgpr // 8) * 8), 800 // (-(-sgpr // 16) * 16 + 16)) >= 7, (sgpr, vgpr)
        assert scratch <= calls_scratch + 16, (scratch, calls_scratch)


def test_k_call_kernels_are_the_kernels_they_were():
    """The packet tick lives in units of its own; the K-call tick's two kernel instantiations and its planning kernel must stay,
    instruction for instruction and operand for operand, those of the commit before (isa_census fingerprints; the mechanism of
    tests/golden/tick_dense_fingerprints.json, and like it a yardstick for one compiler: re-record after a compiler upgrade or a
    deliberate change of those kernels with `python -m webrtc_aecm_amd.isa_census --all`)."""
    from webrtc_aecm_amd import build, isa_census
    recorded = json.loads((GOLDEN / "tick_calls_fingerprints.json").read_text())
    ours = isa_census.census_of_text(isa_census.disassemble(build.build()))
    assert sorted(recorded["kernels"]) == ["plan", "tick_clean", "tick_noclean"]
    for key, want in recorded["kernels"].items():
        got = ours[want["symbol"]]
        assert (got["fingerprint"], got["n_instructions"]) == (want["fingerprint"], want["n_instructions"]), (key, recorded["compiler"])


@pytest.mark.parametrize("name", sorted(ph.GOLDEN_CASES))
def test_golden_runs_are_what_their_recipe_says(name):
    """tests/golden/sesspackets_*.npz (tools/gen_golden.py; run on the GPU by tests/test_gpu_tick_packets.py): the 9 sessions and
    rates of the mixed run x 48 calls in packets of K, arrays only, the pattern the recipe gives, zeros and code 0 where a session
    sat out and behind a half-call session's K * 80 samples; where the unmodified reference is built, its instances -- at per-session
    rates, K calls of the session's size per packet -- give exactly the stored outputs, codes and echo paths."""
    from oracle import pyoracle
    path = GOLDEN / f"{name}.npz"
    assert path.stat().st_size < 150 * 1024
    g = np.load(path, allow_pickle=False)
    fs, n, K, seed = ph.GOLDEN_CASES[name]
    assert (int(g["fs"]), int(g["frame"]), int(g["calls"]), int(g["seed"])) == (fs, n, K, seed) and np.array_equal(g["rates"], mh.RATES)
    assert sorted(g.files) == sorted(["seed", "fs", "frame", "calls", "rates", "flags", "ms", "out", "codes", "paths"])
    flags, ms = ph.golden_pattern(K, seed)
    T = ph.GOLDEN_CALLS // K
    assert np.array_equal(g["flags"], flags) and np.array_equal(g["ms"], ms) and flags.shape == (T, mh.S9)
    idle, half = (flags & ph.IDLE) != 0, (flags & ph.HALF_CALL) != 0
    assert not (flags & ph.SPLIT_CALLS).any() and half[:, list(mh.ALWAYS_HALF)].all() and not half[:, [0, 5, 6, 8]].any()
    assert 0 < half[:, mh.SOMETIMES_HALF].sum() < T and mh.RATES[8] == 8000
    out = g["out"].reshape(mh.S9, T, K * n)
    assert g["out"].dtype == np.int16 and not out[idle.T].any() and not g["codes"][idle].any() and out[~idle.T].any()
    assert not out[half.T][:, K * 80:].any() and out[(half & ~idle).T][:, :K * 80].any()
    assert 0.1 < idle.mean() < 0.35 and 12100 in g["codes"] and g["paths"].shape == (mh.S9, 65)
    if pyoracle.have_reference():
        far, near, _ = mh.signals(seed, mh.RATES, ph.GOLDEN_CALLS * n)
        eout, ecodes, refs = ph.run_reference(lambda rate: pyoracle.RefSession(rate, 1, 3), mh.RATES, ph.packets_ops(K, n, flags, ms), ph.Feed(far, near))
        assert np.array_equal(eout, g["out"]) and np.array_equal(ecodes, g["codes"])
        assert np.array_equal(np.stack([r.get_echo_path()[1] for r in refs]), g["paths"])

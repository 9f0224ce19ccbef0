"""The call trace without a device (include/aecm_batch.h: WebRtcAecmSessions_SetCallTrace): one AecmSessionTrace record per session
and call pair from the K-call and packet ticks, byte for byte what K ordinary ticks under a session trace write.

  - the interface: header, bindings, the unchanged 64-byte struct;
  - the planner (aecm_tick_plan.h: TickObject): the per-call mode accepts ticks of several calls and counts call slots, the two
    traces exclude each other, the per-tick mode refuses what it refused;
  - the records of the CPU double (tests/sim/sim_call_trace.cpp, tests/call_trace_sim.py -- the planning kernels' text with the
    trace's sink, the K-call loop with the body's hook, on the lane simulator) against an untraced-form twin: an object that makes
    the same calls as K ordinary ticks under the per-tick trace, whose wrapper words and core digest after every tick give every
    field by the header's table (session_trace_helpers.header_record, trace_helpers.records_of_digests), and whose buffer must be
    the same bytes;
  - the build: both recipes list the new units, every new kernel is in the code object once per instantiation, the untraced
    kernels keep their fingerprints, the new tick kernels keep the occupancy of the kernels they twin.
The device side is tests/test_gpu_call_trace.py."""
import re
import subprocess

import numpy as np
import pytest

import call_trace_sim as cs
import session_trace_helpers as sh
import trace_helpers as th
import webrtc_aecm_amd as aecm
from helpers import GOLDEN
from webrtc_aecm_amd import ffi

ROOT = GOLDEN.parent.parent
DT = ffi.SESSION_TRACE_DTYPE
GUARD = 2      # guard records on either side of every trace buffer


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_record_size():
    lib = aecm.load()
    header = (ROOT / "include" / "aecm_batch.h").read_text()
    assert re.search(r"\bint32_t WebRtcAecmSessions_SetCallTrace\(AecmSessions \*s, void \*trace_dev, int64_t session_stride, int64_t call_stride, "
                     r"int32_t ring_calls\);", header)
    assert re.search(r"\bint32_t WebRtcAecmSessions_GetCallTraceCalls\(AecmSessions \*s, int64_t \*calls\);", header)
    for name in ("WebRtcAecmSessions_SetCallTrace", "WebRtcAecmSessions_GetCallTraceCalls"):
        assert name in ffi.SESSIONS_SYMBOLS and hasattr(lib, name), name
    assert len(lib.WebRtcAecmSessions_SetCallTrace.argtypes) == 5 and len(lib.WebRtcAecmSessions_GetCallTraceCalls.argtypes) == 2
    for name in ("set_call_trace", "clear_call_trace", "call_trace_calls"):
        assert callable(getattr(aecm.AecmSessions, name))
    assert aecm.session_trace_size_bytes() == 64 == DT.itemsize      # the struct is the session trace's, unchanged
    # what can be asked without a device: no object
    assert lib.WebRtcAecmSessions_SetCallTrace(None, None, 1, 1, 1) == ffi.AECM_BAD_PARAMETER_ERROR
    assert lib.WebRtcAecmSessions_GetCallTraceCalls(None, None) == ffi.AECM_BAD_PARAMETER_ERROR


# ---- the planner -----------------------------------------------------------------------------------------------------------------
def _object(S=4, blocks=64, fs=16000, rates=None, seed=5):
    rs = np.random.RandomState(seed)
    far = rs.randint(-6000, 6000, (S, blocks * 64)).astype(np.int16)
    near = (far // 2 + rs.randint(-300, 300, far.shape)).astype(np.int16)
    return cs.SimSessions(far, near, fs=fs, rates=rates)


def test_per_call_mode_accepts_several_calls_and_counts_call_slots():
    S = 4
    o = _object(S)
    buf = cs.trace_buffer(S * 64)
    assert o.count(cs.PER_CALL) == 0
    assert o.tick(40, calls=2)[0] == 0 and o.count(cs.PER_CALL) == 0                 # nothing attached: nothing counts
    assert o.attach(cs.PER_CALL, buf, 64, 1, 64) == 0 and o.count(cs.PER_CALL) == 0
    want = 0
    for packets in (False, True):
        for calls in (2, 3, 6):
            rc, family, _ = o.tick(40, calls=calls, packets=packets, n=80)
            want += calls
            assert rc == 0 and family == 4 and o.count(cs.PER_CALL) == want, (packets, calls)      # `calls`: a uniform object's packet tick is one
    assert o.tick(40)[0] == 0 and o.count(cs.PER_CALL) == want + 1                   # an ordinary tick: one slot
    want += 1
    idle = np.full(S, cs.IDLE, dtype=np.uint8)
    pos = o.near_pos
    rc, family, _ = o.tick(40, flags=idle, calls=3, n=80)
    assert rc == 0 and family == 0 and o.count(cs.PER_CALL) == want + 3 and o.near_pos == pos + 240      # nobody calls: it still counts
    want += 3
    # refused ticks: neither the count nor the position
    pos = o.near_pos
    assert o.tick(40, n=81, calls=2)[0] == cs.BAD_PARAMETER
    assert o.tick(40, calls=7)[0] == cs.BAD_PARAMETER
    assert o.tick(40, flags=np.full(S, cs.SPLIT_CALLS, dtype=np.uint8), calls=2)[0] == cs.BAD_PARAMETER
    assert o.tick(40, flags=np.full(S, cs.HALF_CALL, dtype=np.uint8), calls=2)[0] == cs.BAD_PARAMETER        # half calls: packet ticks only
    assert o.count(cs.PER_CALL) == want and o.near_pos == pos
    assert o.count(cs.PER_TICK) == 0                                                # the session trace's count is its own
    assert o.attach(cs.PER_CALL, buf, 64, 1, 64) == 0 and o.count(cs.PER_CALL) == 0   # attaching again starts at 0
    assert o.attach(cs.PER_CALL, None, 0, 0, 0) == 0
    assert o.tick(40, calls=2, n=80)[0] == 0 and o.count(cs.PER_CALL) == 0


def test_the_two_traces_exclude_each_other_and_the_per_tick_mode_refuses_as_before():
    S = 3
    o = _object(S)
    a, b = cs.trace_buffer(S * 8), cs.trace_buffer(S * 8)
    assert o.attach(cs.PER_TICK, a, 8, 1, 8) == 0
    assert o.attach(cs.PER_CALL, b, 8, 1, 8) == cs.BAD_PARAMETER                     # ... and the attached one stays attached:
    pos = o.near_pos
    for packets in (False, True):
        for calls in (2, 3, 6):
            assert o.tick(40, calls=calls, packets=packets)[0] == cs.UNSUPPORTED
            assert o.tick(40, calls=calls, packets=packets, n=80)[0] == cs.UNSUPPORTED
    assert o.count(cs.PER_TICK) == 0 and o.near_pos == pos
    assert o.tick(40)[0] == 0 and o.count(cs.PER_TICK) == 1 and o.count(cs.PER_CALL) == 0
    assert o.attach(cs.PER_CALL, None, 0, 0, 0) == 0 and o.count(cs.PER_TICK) == 1   # NULL detaches only its own kind
    assert o.tick(40, calls=2)[0] == cs.UNSUPPORTED
    assert o.attach(cs.PER_TICK, None, 0, 0, 0) == 0
    assert o.attach(cs.PER_CALL, b, 8, 1, 8) == 0
    assert o.attach(cs.PER_TICK, a, 8, 1, 8) == cs.BAD_PARAMETER
    assert o.tick(40, calls=2, n=80)[0] == 0 and o.count(cs.PER_CALL) == 2 and o.count(cs.PER_TICK) == 0
    assert o.attach(cs.PER_TICK, None, 0, 0, 0) == 0 and o.count(cs.PER_CALL) == 2   # likewise
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert o.attach(cs.PER_CALL, b, *bad) == cs.BAD_PARAMETER and o.count(cs.PER_CALL) == 2
    assert o.attach(cs.PER_CALL, b, 8, 1, 8, byte_offset=2) == cs.BAD_PARAMETER and o.count(cs.PER_CALL) == 2
    # an object that never uses the mode: the session trace's existing planner binding refuses and counts as it did
    p = sh.PlanObject(S)
    p.attach()
    assert p.tick(calls=2)[0] == sh.UNSUPPORTED and p.tick()[0] == 0 and p.ticks == 1


# ---- the records -----------------------------------------------------------------------------------------------------------------
def _geometry(kind, S, slots, ring):
    """(session_stride, slot_stride, records in the buffer) of a session-major [S][ring] or call-major [ring][S] buffer."""
    return (ring, 1, S * ring) if kind == "session-major" else (1, S, S * ring)


def _pattern(S, T, seed, packets):
    """Per-tick flags [T, S] and msInSndCardBuf [T, S]: about a quarter idle (one session always calls, one never does in the first
    ticks), some ticks without a far end, half calls for the odd sessions of a packet tick, per-session delays that move."""
    rs = np.random.RandomState(seed)
    flags = np.zeros((T, S), dtype=np.uint8)
    flags[rs.rand(T, S) < 0.25] = cs.IDLE
    flags[:, 0] &= ~np.uint8(cs.IDLE)
    flags[:2, S - 1] = cs.IDLE
    flags[(rs.rand(T, S) < 0.15) & (flags == 0)] = cs.NO_FAREND
    if packets:
        flags[:, 1::2] |= np.where(flags[:, 1::2] & cs.IDLE, 0, cs.HALF_CALL).astype(np.uint8)
    ms = np.tile(np.array([40, 0, 120, 64, 250, 16, 90][:S], dtype=np.int16), (T, 1))
    ms[T // 2:, 2] = 30                                                             # a delay jump: knownDelay moves
    return flags, ms


def _run_pair(K, packets, kind, ring, S=5, calls_total=36, seed=11):
    """A: K-call / packet ticks under the call trace.  B: the same calls as K ordinary ticks each under the session trace, same
    geometry.  Returns (A, B, bufA, bufB, per-call facts of B: flow words [S, C, 32], blocks [S, C], digests [S, C, 24], called [C, S])."""
    T = calls_total // K
    C_ = T * K
    rates = np.array([16000, 8000, 16000, 8000, 16000][:S], dtype=np.int32) if packets else None
    far = np.random.RandomState(seed).randint(-8000, 8000, (S, C_ * 3 * 64)).astype(np.int16)
    near = (far // 2 + np.random.RandomState(seed + 1).randint(-500, 500, far.shape)).astype(np.int16)
    A, B = cs.SimSessions(far, near, rates=rates), cs.SimSessions(far, near, rates=rates)
    ss, cstride, n_rec = _geometry(kind, S, C_, ring)
    bufA, bufB = cs.trace_buffer(n_rec + 2 * GUARD), cs.trace_buffer(n_rec + 2 * GUARD)
    assert A.attach(cs.PER_CALL, bufA, ss, cstride, ring, byte_offset=GUARD * 64) == 0
    assert B.attach(cs.PER_TICK, bufB, ss, cstride, ring, byte_offset=GUARD * 64) == 0
    flags, ms = _pattern(S, T, seed, packets)
    n = 160
    flow = np.zeros((S, C_, 32), dtype=np.int32)
    blocks = np.full((S, C_), -1, dtype=np.int32)
    digests = np.zeros((S, C_, 24), dtype=np.uint32)
    for t in range(T):
        rc, fam, blk = A.tick(ms[t], flags=flags[t], n=n, calls=K, packets=packets)
        assert rc == 0 and fam == (5 if packets else 4), (t, rc, fam)
        assert A.count(cs.PER_CALL) == (t + 1) * K
        for c in range(K):
            rc, _, b1 = B.tick(ms[t], flags=flags[t], n=n)
            assert rc == 0
            j = t * K + c
            blocks[:, j] = b1[:, 0]
            assert np.array_equal(blk[:, c], b1[:, 0]), (t, c)                      # call c's plan runs the blocks of ordinary tick c
            for s in range(S):
                flow[s, j], digests[s, j] = B.flow(s), B.digest(s)
        assert B.count(cs.PER_TICK) == (t + 1) * K
    called = np.repeat((flags & cs.IDLE) == 0, K, axis=0)
    return A, B, bufA, bufB, flow, blocks, digests, called, (ss, cstride, n_rec)


@pytest.mark.parametrize("packets", [False, True], ids=["k-call", "packet"])
@pytest.mark.parametrize("K", [2, 3, 6])
def test_records_equal_the_twins_fields_and_the_per_tick_trace_byte_for_byte(K, packets):
    """A ring that holds every call: every field of every record against the twin's state after that call pair -- wrapper fields from
    its wrapper words by the header's table, `core` from its core digest --, idle sessions' slots and the guards untouched, and the
    whole buffer the bytes the per-tick trace of K ordinary ticks leaves.  The packet tick has half-call sessions and both rates."""
    S, kind = 5, ("session-major" if K != 3 else "call-major")
    A, B, bufA, bufB, flow, blocks, digests, called, (ss, cstride, n_rec) = _run_pair(K, packets, kind, ring=36)
    C_ = called.shape[0]
    assert bufA.tobytes() == bufB.tobytes()
    fill = cs.trace_buffer(1)[0]
    assert (bufA[:GUARD] == fill).all() and (bufA[-GUARD:] == fill).all()
    rec = bufA[GUARD:GUARD + n_rec]
    rates = A.rates
    got = np.stack([[rec[s * ss + j * cstride] for j in range(C_)] for s in range(S)])
    want = np.zeros((S, C_), dtype=DT)
    for s in range(S):
        for j in range(C_):
            if called[j, s]:
                r = sh.header_record(flow[s, j], j, int(blocks[s, j]), int(rates[s]) // 1000)
                r["core"] = th.records_of_digests(digests[s, j])
                want[s, j] = r
    assert sh.first_record_difference(got, want, called.T) is None, sh.first_record_difference(got, want, called.T)
    assert (got[~called.T] == fill).all()                                           # no record for a session that sat out
    # the track is alive: start-up ends, blocks run, the core's estimate moves -- constants cannot pass
    m = called.T
    assert {0, 1} <= set(got["ec_startup"][m].tolist()) and {0, 2} <= set(got["blocks"][m].tolist())
    assert len(set(got["core"]["tot_count"][m].tolist())) > 10
    assert set(got["samp_khz"][m].tolist()) == ({8, 16} if packets else {16})
    # outputs, wrapper words and core state: the K-call tick IS the K ordinary ticks
    assert np.array_equal(A.out, B.out) and np.array_equal(A.blocks_run(), B.blocks_run())
    for s in range(S):
        assert np.array_equal(A.flow(s)[:17], B.flow(s)[:17]) and np.array_equal(A.digest(s), B.digest(s)), s


@pytest.mark.parametrize("kind", ["session-major", "call-major"])
@pytest.mark.parametrize("K,ring", [(2, 1), (3, 1), (3, 2), (6, 1), (6, 4), (6, 5), (3, 7), (6, 6)])
def test_short_rings_leave_what_in_order_writing_leaves(K, ring, kind):
    """ring_calls == 1 keeps the latest call's record; a ring shorter than the tick keeps the last call of every slot; a ring that is
    no multiple of K wraps inside a tick.  Byte for byte the buffer of the per-tick trace, whose K ticks do write in order."""
    A, B, bufA, bufB, flow, blocks, digests, called, (ss, cstride, n_rec) = _run_pair(K, False, kind, ring, S=3, calls_total=18)
    assert bufA.tobytes() == bufB.tobytes()
    rec = bufA[GUARD:GUARD + n_rec]
    C_ = called.shape[0]
    for s in range(3):
        last = {}
        for j in range(C_):
            if called[j, s]:
                last[j % ring] = j
        for slot in range(ring):
            r = rec[s * ss + slot * cstride]
            if slot in last:
                assert r["tick"] == last[slot] and r["blocks"] == blocks[s, last[slot]], (s, slot)
            else:
                assert r == cs.trace_buffer(1)[0]


def test_one_call_ticks_and_k_call_ticks_share_the_slot_numbers():
    """calls == 1 (the session trace's tick with the slot as its number), K-call ticks and a tick nobody makes, mixed on one object:
    the numbering stays continuous."""
    S = 3
    o = _object(S, blocks=200)
    buf = cs.trace_buffer(S * 32)
    assert o.attach(cs.PER_CALL, buf, 32, 1, 32) == 0
    idle = np.full(S, cs.IDLE, dtype=np.uint8)
    some = np.array([0, cs.IDLE, cs.NO_FAREND], dtype=np.uint8)
    plan = [(1, None), (3, None), (1, some), (2, idle), (6, some), (1, None), (2, None)]
    slot, want = 0, {s: [] for s in range(S)}
    for calls, flags in plan:
        assert o.tick(40, flags=flags, calls=calls)[0] == 0
        for s in range(S):
            if flags is None or not flags[s] & cs.IDLE:
                want[s] += list(range(slot, slot + calls))
        slot += calls
        assert o.count(cs.PER_CALL) == slot
    rec = buf.reshape(S, 32)
    fill = cs.trace_buffer(1)[0]
    for s in range(S):
        written = [j for j in range(32) if rec[s, j] != fill]
        assert written == want[s], (s, written, want[s])
        assert [int(rec[s, j]["tick"]) for j in written] == written


# ---- the build -------------------------------------------------------------------------------------------------------------------
TICK_UNIT, PLAN_UNIT = "aecm_call_trace_kernels.hip", "aecm_call_trace_plan_kernels.hip"
NEW_TICK = ("aecm_calls_traced_tick_kernel", "aecm_packets_traced_tick_kernel")
NEW_PLAN = ("aecm_plan_calls_traced_kernel", "aecm_plan_packets_traced_kernel")
TWINNED = ("aecm_tick_calls_kernel", "aecm_tick_packets_kernel", "aecm_flow_plan_calls_kernel", "aecm_flow_plan_packets_kernel")


def test_both_recipes_list_the_new_units_with_their_flags():
    from webrtc_aecm_amd import build
    assert TICK_UNIT in build.KERNEL_SOURCES and PLAN_UNIT in build.KERNEL_SOURCES
    assert build.SOURCE_FLAGS[TICK_UNIT] == build.SOURCE_FLAGS["aecm_tick_calls_kernels.hip"] == build.UNIFORM_BRANCH_FLAGS
    assert PLAN_UNIT not in build.SOURCE_FLAGS and "aecm_tick_calls_plan_kernels.hip" not in build.SOURCE_FLAGS
    cmake = (ROOT / "CMakeLists.txt").read_text()
    assert f"${{CSRC}}/{TICK_UNIT}" in cmake and f"${{CSRC}}/{PLAN_UNIT}" in cmake
    no_flags = cmake[cmake.index('set(extra ${AECM_UNIFORM_BRANCH_FLAGS})'):cmake.index('set(extra "")')]
    assert PLAN_UNIT[:-4] in no_flags and TICK_UNIT[:-4] not in no_flags
    keep = re.search(r"if\(([^\n]*)\)\n\s*list\(APPEND extra \$\{AECM_KEEP_BRANCHES_FLAGS\}\)", cmake).group(1)
    for pattern in re.findall(r'MATCHES "([^"]+)"', keep):                          # (the block kernels' extra flags: neither unit)
        assert pattern not in TICK_UNIT and pattern not in PLAN_UNIT, pattern
    for name in NEW_TICK + NEW_PLAN:                                                # existing tests count matches of these
        assert not any(t in name for t in TWINNED), name


def _metadata(tmp_path):
    from webrtc_aecm_amd import build, isa_census
    lib = tmp_path / build.LIB.name
    lib.write_bytes(build.build().read_bytes())
    subprocess.run([isa_census._tool("llvm-objdump"), "--offloading", str(lib)], check=True, capture_output=True)
    meta = ""
    for obj in sorted(tmp_path.glob(lib.name + ".*amdgcn*gfx950*")):
        meta += subprocess.run([isa_census._tool("llvm-readelf"), "--notes", str(obj)], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {f: int(re.search(rf"\.{f}:\s+(\d+)", block).group(1)) for f in ("sgpr_count", "vgpr_count", "private_segment_fixed_size")}
    return out


def test_new_kernels_are_in_the_code_object_and_keep_the_occupancy_of_their_twins(tmp_path):
    """Every new kernel once per instantiation; registers of the new tick kernels admit the >= 7 waves per SIMD that
    tests/test_tick_calls.py derives from the metadata for the kernels they twin.  Their scratch is printed next to the untraced
    kernels' of the same build (no bound on it is asserted: none has been measured against time)."""
    from webrtc_aecm_amd import build, isa_census
    ours = isa_census.census_of_text(isa_census.disassemble(build.build()))
    for name in NEW_TICK:
        for clean in (0, 1):
            assert len([k for k in ours if re.search(rf"{name}ILb{clean}EEE", k)]) == 1, (name, clean)
    for name in NEW_PLAN:
        assert len([k for k in ours if name in k]) == 1, name
    for name in TWINNED[:2]:
        assert len([k for k in ours if name in k]) == 2, name
    for name in TWINNED[2:]:
        assert len([k for k in ours if name in k]) == 1, name
    meta = _metadata(tmp_path)
    seen = 0
    for new, old in zip(NEW_TICK, TWINNED[:2]):
        for clean in (0, 1):
            (kn, mn), = [(k, v) for k, v in meta.items() if re.search(rf"{new}ILb{clean}EEE", k)]
            (ko, mo), = [(k, v) for k, v in meta.items() if re.search(rf"{old}ILb{clean}EEE", k)]
            print(f"{new}<{clean}> sgpr {mn['sgpr_count']} vgpr {mn['vgpr_count']} scratch {mn['private_segment_fixed_size']} B   |   "
                  f"{old}<{clean}> sgpr {mo['sgpr_count']} vgpr {mo['vgpr_count']} scratch {mo['private_segment_fixed_size']} B")
            sgpr, vgpr = mn["sgpr_count"], mn["vgpr_count"]
            assert min(8, 512 // (-(-vgpr // 8) * 8), 800 // (-(-sgpr // 16) * 16 + 16)) >= 7, (new, clean, sgpr, vgpr)
            seen += 1
    assert seen == 4


def test_untraced_kernels_keep_their_fingerprints():
    """The existing goldens' checks, from here as well: an object that never attaches a call trace runs the kernels it ran."""
    import test_sparse_ticks
    import test_tick_packets
    test_tick_packets.test_k_call_kernels_are_the_kernels_they_were()
    test_sparse_ticks.test_dense_tick_kernels_are_the_kernels_they_were()

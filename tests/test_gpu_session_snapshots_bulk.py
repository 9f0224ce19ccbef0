"""Bulk session snapshots on the GPU (WebRtcAecmSessions_ExportSessions / ImportSessions and their *Device forms): a list of
sessions, one gather or scatter launch.  The yardstick is the single-session pair, which keeps its own code path: every snapshot
is byte for byte ExportSession's, an import leaves what a loop of ImportSession calls leaves, a migrated call continues bit-exactly,
a refused list changes nothing.  Signals and call patterns: sparse_helpers."""
import numpy as np
import pytest

import sparse_helpers as sh
import webrtc_aecm_amd as aecm
from oracle import pyoracle

pytestmark = pytest.mark.gpu

IDLE, NO_FAREND, HALF_CALL = aecm.ffi.SESSION_IDLE, aecm.ffi.SESSION_NO_FAREND, aecm.ffi.SESSION_HALF_CALL
BAD = aecm.ffi.AECM_BAD_PARAMETER_ERROR
SIZE = 34304
FLOW_AT, F_BLK_POS, F_NEAR_LAG = 16192, 16, 25
SCAL_AT, S_STARTUP, S_MULT = 32 + 32 + 12 * 64 * 4, 2, 29


def tick(sb, flags_t, ms_t, far, near, clean, cursors, n):
    """One tick of the host form: every live session's next n samples.  Returns (out[S, n], codes[S])."""
    live = (flags_t & IDLE) == 0
    f, d, c = sh.tick_rows(far, near, clean, cursors, live, n)
    rc, out, codes = sb.tick_host_per_session(f, d, ms_t, c, flags=flags_t)
    nz = codes[codes != 0]
    assert rc == (int(nz[0]) if nz.size else 0)
    cursors[live] += n
    return out, codes


def singles(sb, sessions):
    blobs = []
    for k in sessions:
        rc, snap = sb.export_session(int(k))
        assert rc == 0 and len(snap) == SIZE
        blobs.append(snap)
    return b"".join(blobs)


def words(snap, at, count):
    return np.frombuffer(snap[at:at + 4 * count], dtype=np.int32)


def device_export(sb, sessions, offset=0):
    import torch
    count = sb.num_streams if sessions is None else len(sessions)
    t = torch.full((count * SIZE + 16,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert sb.export_sessions_device(t.data_ptr() + offset, sessions) == 0
    return t.cpu().numpy()[offset:offset + count * SIZE].tobytes()


def device_import(sb, sessions, blobs, any_rate=False, offset=0, count=None):
    import torch
    raw = np.frombuffer(blobs, dtype=np.uint8)
    t = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda")
    t[offset:offset + raw.size] = torch.from_numpy(raw.copy()).cuda()
    torch.cuda.synchronize()
    return sb.import_sessions_device(t.data_ptr() + offset, sessions, raw.size // SIZE if count is None else count, any_rate)


# T, n and the idle ticks of sessions 1, 2, 3.  A session that calls with msInSndCardBuf 40 from the start leaves the start-up
# phase with its sixth call (aecm_flow_plan.h: FlowStartup), so F_BLK_POS = 64 * floor(n * (calls - 6) / 64): 8 320 = 8 192 + 128
# after 58 calls of 160 samples or 110 of 80.  60 ticks of 80 samples are 4 800 samples: no session of that run can reach the ring's end.
BYTES_CASES = [(16000, 160, 60, True, (1, 2, 3)), (8000, 80, 60, False, (1, 2, 3)), (8000, 80, 205, False, (94, 95, 96))]


@pytest.mark.parametrize("fs,n,T,with_clean,idle_ticks", BYTES_CASES)
def test_bytes(fs, n, T, with_clean, idle_ticks):
    """export_sessions(list), host and device form, is the concatenation of export_session(k): 9 sessions ticked with idle
    sessions among them, exported where the out tail crosses the ring's end (some session's F_BLK_POS mod 8 192 in {64, 128,
    192}; not reachable in the 60 ticks of 80 samples, where it is not asserted), where the near tail does (205 ticks of 80 samples:
    near position mod 8 192 = 16) and while a session lags (idle in the last ticks).  Lists: none, one, the last, unordered, all;
    the device form into a 16-byte-aligned tensor and once into one that is only 4-byte aligned."""
    S = 9
    far, near, clean = sh.signals(500, S, T * n, fs, with_clean=with_clean)
    flags, ms = sh.pattern(11 + T, S, T, 0.25, n=n)
    flags[:, :5] = 0
    for s, k in zip((1, 2, 3), idle_ticks):
        flags[8:8 + k, s] = IDLE
    flags[-2:, 4] = IDLE                                      # session 4 is exported while it lags two ticks
    sb = aecm.AecmSessions(S, fs, 1, 3)
    cursors = np.zeros(S, dtype=np.int64)
    for t in range(T):
        tick(sb, flags[t], ms[t], far, near, clean, cursors, n)
    every = singles(sb, range(S))
    blk = [int(words(every[k * SIZE:(k + 1) * SIZE], FLOW_AT, 32)[F_BLK_POS]) & 8191 for k in range(S)]
    print("F_BLK_POS mod 8192:", blk, "near position mod 8192:", (T * n) % 8192)
    if T * n > 8192 + 256:
        assert any(b in (64, 128, 192) for b in blk), blk
    if T == 205:
        assert (T * n) % 8192 == 16
    assert (flags[-1] & IDLE).any() and (flags[-1, 4] & IDLE)
    assert all(words(every[k * SIZE:(k + 1) * SIZE], FLOW_AT, 32)[F_NEAR_LAG] == 0 for k in range(S))
    for lst in ([], [0], [8], [5, 2, 7], None):
        want = every if lst is None else b"".join(every[k * SIZE:(k + 1) * SIZE] for k in lst)
        rc, got = sb.export_sessions(lst)
        assert rc == 0 and got == want, ("host form", lst)
        if lst != []:
            assert device_export(sb, lst) == want, ("device form", lst)
    assert device_export(sb, [5, 2, 7], offset=4) == b"".join(every[k * SIZE:(k + 1) * SIZE] for k in (5, 2, 7)), "4-byte-aligned buffer"
    assert sb.export_sessions_device(0, []) == 0             # count 0: nothing happens, whatever the pointer
    assert singles(sb, range(S)) == every                     # the exporting object is not changed
    sb.close()


def make_b(fs=16000, n=160, S=12):
    """An object of another age without a clean ring: 9 ticks, the last two made by nobody (deferred lag != 0)."""
    far, near, _ = sh.signals(900, S, 9 * n, fs)
    flags, ms = sh.pattern(5, S, 9, 0.2, n=n)
    flags[:3] = 0
    flags[-2:] = IDLE
    sb = aecm.AecmSessions(S, fs, 1, 3)
    cursors = np.zeros(S, dtype=np.int64)
    for t in range(9):
        tick(sb, flags[t], ms[t], far, near, None, cursors, n)
    return sb


@pytest.fixture(scope="module")
def object_a():
    """Object A: 9 sessions at 16 kHz / 160 with a clean input, 25 ticks with idle sessions, then a far-end burst (one call each)
    whose Process has not come yet.  Yields (object, signals, cursors, the burst's rows); the object is not changed by the tests
    that only export from it."""
    fs, n, S, T0 = 16000, 160, 9, 25
    far, near, clean = sh.signals(700, S, (T0 + 40) * n, fs, with_clean=True)
    flags, ms = sh.pattern(21, S, T0, 0.2, n=n, flags_p=0.1, ms_spread=True)
    flags[:, 3] &= ~np.uint8(IDLE)
    sb = aecm.AecmSessions(S, fs, 1, 3)
    cursors = np.zeros(S, dtype=np.int64)
    for t in range(T0):
        tick(sb, flags[t], ms[t], far, near, clean, cursors, n)
    burst = np.stack([far[s, cursors[s]:cursors[s] + n] for s in range(S)])
    assert sb.buffer_farend_host(burst, n, 1) == 0
    yield sb, (far, near, clean), cursors, (flags, ms)
    sb.close()


def test_migration(object_a):
    """A's sessions [3, 0, 7, 4] -- exported right after a far-end burst, before the matching Process -- go into B's slots
    [1, 10, 2, 6]; 30 more ticks in B and in A (the un-migrated twin: an export changes nothing), idle sessions among them:
    output rows and codes equal tick for tick, the sessions' states equal at the end; session 3 against the unmodified reference
    where it is built."""
    a, (far, near, clean), cursors_a, (flags0, ms0) = object_a
    fs, n, SA, K = 16000, 160, 9, 30
    src, dst = [3, 0, 7, 4], [1, 10, 2, 6]
    rc, blobs = a.export_sessions(src)
    assert rc == 0 and blobs == singles(a, src)
    b = make_b()
    before = b.export_sessions(None)[1]
    assert all(words(before[k * SIZE:(k + 1) * SIZE], 0, 8)[3] == 0 for k in range(12))          # B has no clean ring yet
    assert device_import(b, dst, blobs) == 0
    cursors = cursors_a.copy()
    flags, ms = sh.pattern(33, SA, K, 0.25, n=n, flags_p=0.1, ms_spread=True)
    flags[0] = NO_FAREND                                      # the Process that matches the burst: its far frames are buffered already
    cursors_far = cursors + n                                 # (the far rows run one tick ahead from here on)
    bfar, bnear, bclean = sh.signals(950, 12, K * n, fs, with_clean=True)
    bflags, bms = sh.pattern(34, 12, K, 0.3, n=n)
    bcur = np.zeros(12, dtype=np.int64)
    outs = []
    for t in range(K):
        live = (flags[t] & IDLE) == 0
        f, _, _ = sh.tick_rows(far, near, clean, cursors_far, live, n)
        _, d, c = sh.tick_rows(far, near, clean, cursors, live, n)
        rc, oa, ca = a.tick_host_per_session(f, d, ms[t], c, flags=flags[t])
        blive = (bflags[t] & IDLE) == 0
        bf, bd, bc = sh.tick_rows(bfar, bnear, bclean, bcur, blive, n)
        bfl, bm = bflags[t].copy(), bms[t].copy()
        for s, k in zip(src, dst):
            bf[k], bd[k], bc[k], bfl[k], bm[k] = f[s], d[s], c[s], flags[t, s], ms[t, s]
        rc, ob, cb = b.tick_host_per_session(bf, bd, bm, bc, flags=bfl)
        for s, k in zip(src, dst):
            assert np.array_equal(oa[s], ob[k]) and ca[s] == cb[k], (t, s, k)
        outs.append(oa[3].copy())
        cursors[live] += n
        cursors_far[live & ((flags[t] & NO_FAREND) == 0)] += n
        bcur[blive & ~np.isin(np.arange(12), dst)] += n
    assert any(o.any() for o in outs)
    for s, k in zip(src, dst):
        assert sh.snapshot_state(a.export_session(s)[1]) == sh.snapshot_state(b.export_session(k)[1]), (s, k)
    if pyoracle.have_reference():
        # session 3 on an instance of the reference: its 25 ticks, the burst, the 30 ticks
        ref = pyoracle.RefSession(fs, 1, 3)
        cur = 0
        for t in range(flags0.shape[0]):
            if flags0[t, 3] & IDLE:
                continue
            sl = slice(cur, cur + n)
            sh.session_call(ref, far[3, sl], near[3, sl], clean[3, sl], n, int(flags0[t, 3]), ms0[t, 3])
            cur += n
        assert cur == cursors_a[3] and ref.buffer_farend(far[3, cur:cur + n]) == 0
        cur_far = cur + n
        for t in range(K):
            if flags[t, 3] & IDLE:
                assert not outs[t].any()
                continue
            code, o = sh.session_call(ref, far[3, cur_far:cur_far + n], near[3, cur:cur + n], clean[3, cur:cur + n], n, int(flags[t, 3]), ms[t, 3])
            assert np.array_equal(o, outs[t]), t
            cur += n
            cur_far += 0 if flags[t, 3] & NO_FAREND else n
    b.close()


def test_import_equals_a_loop_of_imports(object_a):
    """The same list through import_sessions (host and device form) and through import_session one by one: the objects' complete
    exports are identical.  Across rates: a mixed object's sessions into a uniform one with any_rate (refused without), every
    slot's rate afterwards, again against the loop."""
    a = object_a[0]
    src, dst = [3, 0, 7, 4], [1, 10, 2, 6]
    blobs = singles(a, src)
    loop = make_b()
    for i, k in enumerate(dst):
        assert loop.import_session(k, blobs[i * SIZE:(i + 1) * SIZE]) == 0
    want = loop.export_sessions(None)[1]
    assert want == singles(loop, range(12))
    for form in ("host", "device", "device4"):
        b = make_b()
        rc = b.import_sessions(dst, blobs) if form == "host" else device_import(b, dst, blobs, offset=4 if form == "device4" else 0)
        assert rc == 0 and b.export_sessions(None)[1] == want, form
        b.close()
    loop.close()
    # a mixed object: 8 kHz sessions make half calls of the 160-sample tick
    S, n = 6, 160
    rates = np.array([16000, 8000, 8000, 16000, 8000, 16000], dtype=np.int32)
    m = aecm.AecmSessions(S, 16000, 1, 3, rates=rates)
    far, near, _ = sh.signals(40, S, 12 * n, 16000)
    fl = np.where(rates == 8000, HALF_CALL, 0).astype(np.uint8)
    for t in range(12):
        rc, _, _ = m.tick_host_per_session(far[:, t * n:(t + 1) * n], near[:, t * n:(t + 1) * n], np.full(S, 40, dtype=np.int16), flags=fl)
        assert rc == 0
    rc, mixed = m.export_sessions([4, 0, 1])
    assert rc == 0 and mixed == singles(m, [4, 0, 1])
    slots = [7, 2, 11]
    loop = make_b()
    for i, k in enumerate(slots):
        assert loop.import_session_any_rate(k, mixed[i * SIZE:(i + 1) * SIZE]) == 0
    want = loop.export_sessions(None)[1]
    objects = []
    for form in ("host", "device"):
        b = make_b()
        before = b.export_sessions(None)[1]
        refuse = b.import_sessions(slots, mixed) if form == "host" else device_import(b, slots, mixed)
        assert refuse == BAD and b.export_sessions(None)[1] == before, form
        rc = b.import_sessions(slots, mixed, any_rate=True) if form == "host" else device_import(b, slots, mixed, any_rate=True)
        assert rc == 0 and b.export_sessions(None)[1] == want, form
        got = [b.get_session_rate(k) for k in range(12)]
        assert got == [(0, {7: 8000, 2: 16000, 11: 8000}.get(k, 16000)) for k in range(12)], (form, got)
        assert got == [loop.get_session_rate(k) for k in range(12)]
        objects.append(b)
    # ... and the objects tick on alike (the launch routing goes by the rate mirrors: an object that now holds 8 kHz sessions)
    far, near, _ = sh.signals(60, 12, 4 * n, 16000)
    fl = np.array([HALF_CALL if k in (7, 11) else 0 for k in range(12)], dtype=np.uint8)
    for t in range(4):
        rows = [o.tick_host_per_session(far[:, t * n:(t + 1) * n], near[:, t * n:(t + 1) * n], np.full(12, 40, dtype=np.int16), flags=fl)
                for o in [loop] + objects]
        for rc, out, codes in rows[1:]:
            assert rc == rows[0][0] and np.array_equal(out, rows[0][1]) and np.array_equal(codes, rows[0][2]), t
    for o in objects:
        assert o.export_sessions(None)[1] == loop.export_sessions(None)[1]
        o.close()
    loop.close(), m.close()


def _put(blobs, index, at, value):
    raw = bytearray(blobs)
    raw[index * SIZE + at:index * SIZE + at + 4] = np.array([value], dtype=np.int32).tobytes()
    return bytes(raw)


def _other_rate(blobs, index):
    """Snapshot `index` as a consistent snapshot of 8 kHz: header, core header and core state agree."""
    return _put(_put(_put(blobs, index, 8, 8000), index, 32 + 8, 8000), index, SCAL_AT + 4 * S_MULT, 1)


ALL_OR_NOTHING = {
    "magic": lambda blobs: (_put(blobs, 3, 0, 0x4e534542), [1, 10, 2, 6, 4]),
    "lag word 81": lambda blobs: (_put(blobs, 3, FLOW_AT + 4 * F_NEAR_LAG, 81), [1, 10, 2, 6, 4]),
    "core scalar": lambda blobs: (_put(blobs, 3, SCAL_AT + 4 * S_STARTUP, 3), [1, 10, 2, 6, 4]),
    "other rate": lambda blobs: (_other_rate(blobs, 3), [1, 10, 2, 6, 4]),
    "duplicate slot": lambda blobs: (blobs, [1, 10, 2, 10, 4]),
    "slot S": lambda blobs: (blobs, [1, 10, 2, 12, 4]),
}


@pytest.mark.parametrize("case", list(ALL_OR_NOTHING) + ["size_bytes off by one", "device pointer off by 2"])
def test_all_or_nothing(object_a, case):
    """Five snapshots of which the fourth is bad, a bad list or bad arguments: AECM_BAD_PARAMETER_ERROR from the host form and
    from the device form, the object byte for byte what it was, and still without a clean ring (the snapshots carry one)."""
    import torch
    a = object_a[0]
    good = singles(a, [3, 0, 7, 4, 8])
    assert all(words(good[k * SIZE:(k + 1) * SIZE], 0, 8)[3] == 1 for k in range(5))
    b = make_b()
    before = b.export_sessions(None)[1]
    lib = b.lib
    if case in ALL_OR_NOTHING:
        blobs, slots = ALL_OR_NOTHING[case](good)
        assert b.import_sessions(slots, blobs) == BAD
        assert device_import(b, slots, blobs) == BAD
        if "slot" in case:                                    # a list is a list on export too
            assert b.export_sessions(slots)[0] == BAD
            t = torch.zeros(5 * SIZE, dtype=torch.uint8, device="cuda")
            assert b.export_sessions_device(t.data_ptr(), slots) == BAD
    elif case == "size_bytes off by one":
        slots = np.array([1, 10, 2, 6, 4], dtype=np.int32)
        host = np.frombuffer(good, dtype=np.uint8).copy()
        t = torch.from_numpy(host).cuda()
        out = np.zeros(5 * SIZE + 1, dtype=np.uint8)
        for size in (5 * SIZE - 1, 5 * SIZE + 1):
            assert lib.WebRtcAecmSessions_ImportSessions(b.h, slots.ctypes.data, 5, host.ctypes.data, size, 0) == BAD
            assert lib.WebRtcAecmSessions_ImportSessionsDevice(b.h, slots.ctypes.data, 5, t.data_ptr(), size, 0) == BAD
            assert lib.WebRtcAecmSessions_ExportSessions(b.h, slots.ctypes.data, 5, out.ctypes.data, size) == BAD
            assert lib.WebRtcAecmSessions_ExportSessionsDevice(b.h, slots.ctypes.data, 5, t.data_ptr(), size) == BAD
        assert lib.WebRtcAecmSessions_ImportSessions(b.h, slots.ctypes.data, -1, host.ctypes.data, 0, 0) == BAD
        assert lib.WebRtcAecmSessions_ImportSessions(b.h, slots.ctypes.data, 5, None, 5 * SIZE, 0) == aecm.ffi.AECM_NULL_POINTER_ERROR
        assert lib.WebRtcAecmSessions_ExportSessionsDevice(b.h, slots.ctypes.data, 5, None, 5 * SIZE) == aecm.ffi.AECM_NULL_POINTER_ERROR
    else:
        # (the host forms know no alignment: this is a rule of the *Device forms, import and export alike)
        assert device_import(b, [1, 10, 2, 6, 4], good, offset=2) == BAD
        t = torch.zeros(5 * SIZE + 16, dtype=torch.uint8, device="cuda")
        assert b.export_sessions_device(t.data_ptr() + 2, [1, 10, 2, 6, 4]) == BAD
    after = b.export_sessions(None)[1]
    assert after == before
    assert all(words(after[k * SIZE:(k + 1) * SIZE], 0, 8)[3] == 0 for k in range(12))           # has_clean 0: no ring was allocated
    assert b.import_sessions([1, 10, 2, 6, 4], good) == 0                                        # ... and the object still takes a good list
    assert words(b.export_session(0)[1], 0, 8)[3] == 1
    b.close()


def test_chunking():
    """259 sessions -- one stage chunk of the host forms (256) and three more -- through export_sessions, import_sessions into a fresh
    object and export_sessions again: the same bytes; sessions on both sides of the chunk boundary against export_session."""
    S, fs, n, T = 259, 8000, 80, 12
    rng = np.random.default_rng(3)
    far = rng.integers(-8000, 8000, (S, T * n)).astype(np.int16)
    near = (far // 2 + rng.integers(-300, 300, (S, T * n))).astype(np.int16)
    flags, ms = sh.pattern(8, S, T, 0.2, n=n, ms_spread=True)
    sb = aecm.AecmSessions(S, fs, 1, 3)
    cursors = np.zeros(S, dtype=np.int64)
    for t in range(T):
        tick(sb, flags[t], ms[t], far, near, None, cursors, n)
    rc, blobs = sb.export_sessions(None)
    assert rc == 0 and len(blobs) == S * SIZE
    for k in (0, 255, 256, 258):
        assert blobs[k * SIZE:(k + 1) * SIZE] == sb.export_session(k)[1], k
    fresh = aecm.AecmSessions(S, fs, 1, 3)
    assert fresh.import_sessions(None, blobs) == 0
    rc, again = fresh.export_sessions(None)
    assert rc == 0 and again == blobs
    order = np.random.default_rng(4).permutation(S).astype(np.int32)      # an unordered list across the chunks
    rc, shuffled = sb.export_sessions(order)
    assert rc == 0 and shuffled == b"".join(blobs[k * SIZE:(k + 1) * SIZE] for k in order)
    sb.close(), fresh.close()

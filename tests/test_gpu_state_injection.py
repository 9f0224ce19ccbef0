"""The import gate on the device, and the block kernels started from every kind of state the gate admits.

Gate matrix: every rule of tests/state_corpus.py (STATE_RULES and the rule over the four supGainErrParam words) at lo - 1, lo, hi
and hi + 1, lane rules at lanes 0, 35, 36 and 63, through every import entry point -- the host's copy of the gate (ImportState,
ImportSession) and the device's (the validation kernels of ImportStates / ImportStatesDevice / ImportSessions /
ImportSessionsDevice).  Every verdict equals the restatement's; a refusal changes no byte of any stream, an acceptance leaves
exactly the blob.

Parity: states of the corpus that tests/test_state_injection.py's checks admit and clear are first cleared again HERE on the CPU
(simulator with the claims checked = oracle, outputs and whole images), then imported and run through the kernel families in
launches of 1, 2 and 3 blocks: every output sample and every word of the exported state, bit-exact.  No state reaches the device
before its CPU clearance."""
import functools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import inject_sim
import state_corpus as sc
import test_gpu_pipelined_clean as P
import test_gpu_session_snapshots_bulk as SB
import webrtc_aecm_amd as aecm
from helpers import GOLDEN
from oracle import pyoracle

pytestmark = pytest.mark.gpu
BAD = aecm.ffi.AECM_BAD_PARAMETER_ERROR
RATES = (16000, 8000)
N = sc.BLOB_BYTES
SESSION_CORE_AT = 32                       # a session snapshot: its own 32-byte header, then the block stream's blob
POSITIONS = (0, 2, 4)                      # first, middle, last of 5


def _probes(fs):
    """Class (a) of the corpus at this rate: (state, admitted)."""
    return [(s, s.expected_defect() is None) for s in sc.rule_mutations() if s.fs == fs]


def _bases(fs, count=5):
    return [b for b in sc.base_states() if b.fs == fs and not b.name.endswith("age0")][:count]


# ---- gate matrix: the batch forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", RATES)
def test_gate_matrix_batch_forms(fs):
    import torch
    lib = aecm.load()
    assert lib.WebRtcAecmBatch_state_size_bytes() == N
    probes = _probes(fs)
    assert len(probes) > 150 and sum(ok for _, ok in probes) > 60
    b = aecm.AecmBatch(5, fs)
    cur = np.stack([np.frombuffer(s.blob(), dtype=np.uint8) for s in _bases(fs)]).copy()
    b.import_states(0, cur)
    assert np.array_equal(b.export_states(0, 5), cur)
    unaligned = np.zeros(5 * N + 1, dtype=np.uint8)[1:]
    assert unaligned.ctypes.data % 4 != 0

    def single(pos, five):
        return lib.WebRtcAecmBatch_ImportState(b.h, pos, five[pos].tobytes(), N)

    def host(pos, five):
        return lib.WebRtcAecmBatch_ImportStates(b.h, 0, 5, five.ctypes.data, five.nbytes)

    def host_unaligned(pos, five):
        unaligned[:] = five.reshape(-1)
        return lib.WebRtcAecmBatch_ImportStates(b.h, 0, 5, unaligned.ctypes.data, unaligned.nbytes)

    def device(pos, five):
        t = torch.from_numpy(five).cuda()
        torch.cuda.synchronize()
        return lib.WebRtcAecmBatch_ImportStatesDevice(b.h, 0, 5, t.data_ptr(), five.nbytes)

    for k, (st, ok) in enumerate(probes):
        pos = POSITIONS[k % 3]
        five = cur.copy()
        five[pos] = np.frombuffer(st.blob(), dtype=np.uint8)
        for name, form in (("ImportState", single), ("ImportStates", host), ("ImportStates, unaligned buffer", host_unaligned), ("ImportStatesDevice", device)):
            rc = form(pos, five)
            after = b.export_states(0, 5)
            if ok:
                assert rc == 0, f"{name} refuses {st.name} at position {pos}"
                assert np.array_equal(after, five), f"{name}, {st.name}: " + sc.describe_image_diff(sc.image_of_blob(after[pos]), st.image, live_only=False)
                b.import_states(0, cur)                         # back to the five base states for the next form
            else:
                assert rc == BAD, f"{name} admits {st.name} at position {pos} (restatement: {st.expected_defect()}), code {rc}"
                assert np.array_equal(after, cur), f"{name} refused {st.name} but changed a stream"
    b.close()


# ---- gate matrix: the session forms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,any_rate", [(16000, False), (16000, True), (8000, False)])
def test_gate_matrix_session_forms(fs, any_rate):
    """The core rules through ImportSession (the host's gate), ImportSessions and ImportSessionsDevice (the device's, one worker
    per scalar field and lane, worker 0 the rule over several fields)."""
    sb = SB.make_b(fs, 160 if fs == 16000 else 80, S=5)
    size = SB.SIZE
    rc, every = sb.export_sessions(None)
    assert rc == 0 and len(every) == 5 * size
    cur = np.frombuffer(every, dtype=np.uint8).reshape(5, size).copy()
    core = slice(SESSION_CORE_AT, SESSION_CORE_AT + N)
    assert bytes(cur[0, core])[:8] == sc.State("x", fs, *sc.base_states()[0].image).blob()[:8]          # magic and layout version: the core blob lies here
    lst = list(range(5))

    def exported():
        rc, raw = sb.export_sessions(None)
        assert rc == 0
        return np.frombuffer(raw, dtype=np.uint8).reshape(5, size)

    def single(pos, five):
        return sb.import_session_any_rate(pos, five[pos].tobytes()) if any_rate else sb.import_session(pos, five[pos].tobytes())

    def host(pos, five):
        return sb.import_sessions(lst, five, any_rate)

    def device(pos, five):
        return SB.device_import(sb, lst, five.tobytes(), any_rate)

    for k, (st, ok) in enumerate(_probes(fs)):
        pos = POSITIONS[k % 3]
        five = cur.copy()
        five[pos, core] = np.frombuffer(st.blob(), dtype=np.uint8)
        for name, form in (("ImportSession", single), ("ImportSessions", host), ("ImportSessionsDevice", device)):
            rc = form(pos, five)
            after = exported()
            if ok:
                assert rc == 0, f"{name} refuses {st.name} at position {pos}, code {rc}"
                assert np.array_equal(after[pos, core], five[pos, core]), f"{name}, {st.name}: " + sc.describe_image_diff(
                    sc.image_of_blob(after[pos, core]), st.image, live_only=False)
                others = [p for p in range(5) if p != pos]
                assert np.array_equal(after[others], cur[others]), f"{name}, {st.name}: another session changed"
                assert sb.import_sessions(lst, cur) == 0
            else:
                assert rc == BAD, f"{name} admits {st.name} at position {pos} (restatement: {st.expected_defect()}), code {rc}"
                assert np.array_equal(after, cur), f"{name} refused {st.name} but changed a session"
    sb.close()


# ---- parity of admitted states ---------------------------------------------------------------------------------------------------
MIN_STATES = 256
LAUNCHES = sc.LAUNCHES


@functools.lru_cache(maxsize=None)
def cleared(fs):
    """The states of this rate that go to the device, and what they must give: base states, ALL admitted states of class (a) and
    class (b), and combinations up to MIN_STATES.  Both ways -- without and with the clean input -- each is run here on the
    simulator with the claims checked and on the oracle; the two must agree in every output sample and every live state word and no
    claim may be violated, or nothing is launched.  Returns dict(states, blobs, far, near, clean, plain=(out, images), with_clean=...,
    ragged=(lens, out, images))."""
    corpus = [s for s in sc.corpus() if s.fs == fs and s.expected_defect() is None]
    fixed = len(sc.base_states()) + len(sc.rule_mutations()) + len(sc.extreme_mutations())
    admitted_fixed = [s for s in sc.corpus()[:fixed] if s.fs == fs and s.expected_defect() is None]
    mine = {id(s) for s in admitted_fixed}
    states = admitted_fixed + [s for s in corpus if id(s) not in mine][:max(0, MIN_STATES - len(admitted_fixed))]
    assert len(states) >= MIN_STATES
    for s in states:
        assert inject_sim.validate(s.vec, s.scal, s.fs) is None, s.name
    audio = [sc.continuation_audio(500000 + fs + i) for i in range(len(states))]
    far, near, clean = (np.ascontiguousarray(np.stack([a[k] for a in audio])) for k in range(3))
    res = dict(states=states, blobs=np.stack([np.frombuffer(s.blob(), dtype=np.uint8) for s in states]), far=far, near=near, clean=clean)

    def clear(with_clean, lens_per_state=None):
        vec, scal, hist = sc.stack(states)
        outs = np.zeros_like(near)
        if lens_per_state is None:
            kinds, values, outs = inject_sim.run_many(vec, scal, hist, far, near, clean, np.full(len(states), with_clean, dtype=np.uint8), LAUNCHES)
            assert not kinds.any(), [(states[i].name, inject_sim.KINDS[int(kinds[i])]) for i in np.flatnonzero(kinds)][:10]
        for i, s in enumerate(states):
            n = sc.N_BLOCKS * 64 if lens_per_state is None else int(lens_per_state[i]) * 64
            if lens_per_state is not None:
                kind, o = inject_sim.run(vec[i], scal[i], hist[i], far[i, :n], near[i, :n], clean[i, :n] if with_clean else None)
                assert kind is None, (s.name, kind)
                outs[i, :n] = o
            o = pyoracle.OracleStream(fs).import_image(*s.image)
            exp = o.process_blocks(far[i, :n], near[i, :n], clean[i, :n] if with_clean else None)
            assert np.array_equal(outs[i, :n], exp), f"CPU clearance: simulator and oracle differ on {s.name}"
            diff = sc.describe_image_diff((vec[i], scal[i], hist[i]), o.export_image())
            assert not diff, f"CPU clearance: {s.name}: {diff}"
        return outs, (vec, scal, hist)
    res["plain"] = clear(False)
    res["with_clean"] = clear(True)
    lens = (np.arange(len(states)) % 7).astype(np.int32)
    res["ragged"] = (lens, *clear(False, lens))
    return res


def _assert_images(b, c, images, what):
    got = b.export_states(0, len(c["states"]))
    vec, scal, hist = images
    for i, s in enumerate(c["states"]):
        diff = sc.describe_image_diff(sc.image_of_blob(got[i]), (vec[i], scal[i], hist[i]))
        assert not diff, f"{what}: state of {s.name} after the launches: {diff}"


def _assert_out(c, out, exp, what):
    bad = np.flatnonzero((out != exp).any(axis=1))
    assert bad.size == 0, f"{what}: output differs for {len(bad)} states, first {c['states'][int(bad[0])].name} at sample {int(np.flatnonzero(out[bad[0]] != exp[bad[0]])[0])}"


def _loaded_batch(c, fs, variant=aecm.KERNEL_FAST):
    """One ImportStatesDevice loads all the states; the export gives the blobs back word for word, dead words included."""
    import torch
    n = len(c["states"])
    b = aecm.AecmBatch(n, fs, variant=variant)
    t = torch.from_numpy(c["blobs"]).cuda()
    torch.cuda.synchronize()
    b.import_states_device(0, n, t.data_ptr())
    assert np.array_equal(b.export_states(0, n), c["blobs"])
    return b


def _run_launches(b, c, with_clean, want, what, launches=LAUNCHES):
    exp_out, images = c["with_clean" if with_clean else "plain"]
    outs, at = [], 0
    assert sum(launches) == sc.N_BLOCKS
    for n in launches:
        d = b.describe_launch(n, clean=with_clean)
        assert want(d, n), (what, n, d)
        sl = slice(at * 64, (at + n) * 64)
        cut = lambda a: np.ascontiguousarray(a[:, sl])
        outs.append(P._run(b, cut(c["far"]), cut(c["near"]), cut(c["clean"]) if with_clean else None, n))
        at += n
    _assert_out(c, np.concatenate(outs, axis=1), exp_out, what)
    _assert_images(b, c, images, what)


# name: (kernel variant, set-up, the launch form asserted before a launch of n blocks, the launches).  A launch takes the chunk queue
# from two chunks on (aecm_block_kernels.hip: QueueLaunchApplies): chunks of 2 as ONE launch of the six blocks (the state goes through
# memory after blocks 2 and 4), chunks of 1 in the launches of 2 and 3 blocks (through memory after every block).
FORMS = {
    "one wavefront per stream, fast": (aecm.KERNEL_FAST, lambda b: b.set_launch_pipelining(0), lambda d, n: d == (0, 0), LAUNCHES),
    "one wavefront per stream, safe": (aecm.KERNEL_SAFE, lambda b: b.set_launch_pipelining(0), lambda d, n: d[0] in (0, 1), LAUNCHES),
    "chunk queue, chunks of 2": (aecm.KERNEL_FAST, lambda b: b.set_launch_chunking(2, 0), lambda d, n: d == (2, 2), (sc.N_BLOCKS,)),
    "chunk queue, chunks of 1": (aecm.KERNEL_FAST, lambda b: (b.set_launch_pipelining(0), b.set_launch_chunking(1, 0)),
                                 lambda d, n: d == ((2, 1) if n >= 2 else (0, 0)), LAUNCHES),
    "pipelined, sixteen waves": (aecm.KERNEL_FAST, lambda b: (b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1, **P.SHAPES["sixteen waves (42240)"][0]),
                                                              b.set_clean_pipelining(True)), lambda d, n: d[0] == 3 and d[1] & ~P.CLEAN_BIT == 0x1a02, LAUNCHES),
    "pipelined, six waves": (aecm.KERNEL_FAST, lambda b: (b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1, **P.SHAPES["six waves (20)"][0]),
                                                          b.set_clean_pipelining(True)), lambda d, n: d[0] == 3 and d[1] & ~P.CLEAN_BIT == 0x000, LAUNCHES),
}


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("with_clean", [False, True], ids=["plain", "clean"])
@pytest.mark.parametrize("form", list(FORMS))
def test_parity_of_admitted_states(form, with_clean, fs):
    c = cleared(fs)                                           # CPU clearance first: fails here, before any launch, if it does not hold
    variant, setup, want, launches = FORMS[form]
    b = _loaded_batch(c, fs, variant)
    setup(b)
    _run_launches(b, c, with_clean, want, f"{form}{', clean input' if with_clean else ''}, {fs} Hz", launches)
    b.close()


@pytest.mark.parametrize("fs", RATES)
def test_parity_ragged_queue(fs):
    """The ragged queue, lengths 0 .. 6 in one launch; a stream of length 0 keeps its imported state word for word."""
    import test_gpu_ragged as R
    c = cleared(fs)
    lens, exp_out, images = c["ragged"]
    b = _loaded_batch(c, fs)
    b.set_launch_chunking(2, 0)
    d = b.describe_ragged_launch(lens)
    assert (d["form"], d["chunk_blocks"]) == (2, 2), d
    out = R._run_device(b, c["far"], c["near"], lens, sc.N_BLOCKS)
    for i, s in enumerate(c["states"]):
        n = int(lens[i]) * 64
        assert np.array_equal(out[i, :n], exp_out[i, :n]), f"ragged queue: output of {s.name} (length {lens[i]})"
        assert (out[i, n:] == R.SENTINEL).all(), s.name
    _assert_images(b, c, images, "ragged queue")
    got = b.export_states(0, len(lens))
    zero = np.flatnonzero(lens == 0)
    assert np.array_equal(got[zero], c["blobs"][zero])
    b.close()


@pytest.mark.parametrize("fs", RATES)
def test_parity_traced_launch(fs):
    """The same launches with a block trace attached (the trace kernels are instantiations of their own)."""
    import torch
    c = cleared(fs)
    b = _loaded_batch(c, fs)
    trace = torch.zeros((len(c["states"]), max(LAUNCHES), 8), dtype=torch.int32, device="cuda")
    b.set_block_trace(trace.data_ptr(), max(LAUNCHES), 1)
    _run_launches(b, c, False, lambda d, n: d[0] != 3, f"traced launch, {fs} Hz")
    assert int(trace.abs().sum().item()) != 0
    b.clear_block_trace()
    b.close()


# ---- parity through the session object -------------------------------------------------------------------------------------------
PREROLL_TICKS = 8              # with msInSndCardBuf 40 a session leaves the start-up phase with its sixth call: blocks flow from then on


@functools.lru_cache(maxsize=None)
def cleared_sessions(fs):
    """One simulated session (the product's Session class over the simulated engine, claims checked) per state of cleared(fs):
    PREROLL_TICKS ticks of its own audio, then the state becomes its core state (simlib.engine_inject_next) and it makes three
    ordinary ticks and the three call pairs of one K = 3 tick.  Returns (n, far, near [S, 14 * n], out, the core images at the end).
    The wrapper state -- rings, positions, start-up -- is what the preroll left, on the CPU as in the snapshot the device exports."""
    import simlib
    c = cleared(fs)
    n = 160 if fs == 16000 else 80
    S, T = len(c["states"]), PREROLL_TICKS + 6
    rs = np.random.RandomState(fs + 99)
    levels = np.array([0, 3, 300, 8000, 32768], dtype=np.int64)
    env = np.repeat(levels[rs.randint(0, len(levels), size=(S, T))], n, axis=1)
    far = (rs.randint(-32768, 32768, size=(S, T * n)).astype(np.int64) * env >> 15).clip(-32768, 32767).astype(np.int16)
    near = (np.roll(far, 23, axis=1).astype(np.int64) // 2 + rs.randint(-2000, 2001, size=(S, T * n))).clip(-32768, 32767).astype(np.int16)
    out = np.zeros_like(near)
    vec, scal, hist = sc.stack(c["states"])
    images = []
    for i in range(S):
        sess = simlib.SimSession()
        assert sess.init(fs) == 0
        for t in range(T):
            if t == PREROLL_TICKS:
                simlib.engine_inject_next(vec[i], scal[i], hist[i])
            sl = slice(t * n, (t + 1) * n)
            assert sess.buffer_farend(far[i, sl]) == 0
            rc, out[i, sl] = sess.process(near[i, sl], None, 40)
            assert rc == 0
        img = simlib.engine_last_image()
        assert img is not None, "no block ran after the injection"
        images.append(img)
    return n, far, near, out, images


@pytest.mark.parametrize("fs", RATES)
def test_parity_through_import_sessions(fs):
    """ImportSessions loads the states as the core states of live sessions (the wrapper state of each is its own, PREROLL_TICKS ticks
    old); three ordinary ticks and one TickCalls with K = 3 give what the simulated sessions give, and leave their core images."""
    n, far, near, exp_out, exp_images = cleared_sessions(fs)          # on the CPU first
    c = cleared(fs)
    S = len(c["states"])
    sb = aecm.AecmSessions(S, fs, 1, 3)
    for t in range(PREROLL_TICKS):
        sl = slice(t * n, (t + 1) * n)
        rc, out = sb.tick_host(far[:, sl], near[:, sl], 40)
        assert rc == 0 and np.array_equal(out, exp_out[:, sl]), ("preroll", t)
    rc, every = sb.export_sessions(None)
    assert rc == 0
    blobs = np.frombuffer(every, dtype=np.uint8).reshape(S, SB.SIZE).copy()
    blobs[:, SESSION_CORE_AT:SESSION_CORE_AT + N] = c["blobs"]
    assert sb.import_sessions(None, blobs) == 0
    at = PREROLL_TICKS * n
    for t in range(3):
        rc, out = sb.tick_host(far[:, at:at + n], near[:, at:at + n], 40)
        assert rc == 0
        _assert_out(c, out, exp_out[:, at:at + n], f"ordinary tick {t} after ImportSessions, {fs} Hz")
        at += n
    rc, out, codes = sb.tick_calls_host(far[:, at:at + 3 * n], near[:, at:at + 3 * n], 3, 40)
    assert rc == 0 and not codes.any()
    _assert_out(c, out, exp_out[:, at:at + 3 * n], f"TickCalls K = 3 after ImportSessions, {fs} Hz")
    rc, every = sb.export_sessions(None)
    assert rc == 0
    got = np.frombuffer(every, dtype=np.uint8).reshape(S, SB.SIZE)
    for i, s in enumerate(c["states"]):
        diff = sc.describe_image_diff(sc.image_of_blob(got[i, SESSION_CORE_AT:SESSION_CORE_AT + N]), exp_images[i])
        assert not diff, f"core state of the session started from {s.name}: {diff}"
    sb.close()


def test_checked_build_counts_nothing_on_admitted_states(tmp_path):
    """libaecm_mi355x_checked.so in a child process: the same states as one wavefront per stream, through the chunk queue and
    pipelined.  Both audit counters stay 0 and outputs and states equal the CPU's."""
    from webrtc_aecm_amd import build
    assert build.LIB_CHECKED.exists()
    for fs in RATES:
        cleared(fs)                                           # CPU clearance in this process too, before the child launches anything
    script = tmp_path / "audit_states.py"
    script.write_text(textwrap.dedent("""
        import webrtc_aecm_amd as aecm
        import test_gpu_state_injection as T
        assert aecm.check_counters(0, reset=True) is not None
        for fs in T.RATES:
            c = T.cleared(fs)
            for form, setup, want, launches in ((0, lambda b: b.set_launch_pipelining(0), lambda d, n: d[0] == 0, T.LAUNCHES),
                                                (2, lambda b: b.set_launch_chunking(2, 0), lambda d, n: d[0] == 2, (6,)),
                                                (3, lambda b: b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1), lambda d, n: d[0] == 3, T.LAUNCHES)):
                b = T._loaded_batch(c, fs)
                setup(b)
                T._run_launches(b, c, False, want, f"checked build, form {form}, {fs} Hz", launches)
                b.close()
        k = aecm.check_counters(0)
        print("AUDIT", int(k[0]), int(k[1]))
    """))
    env = dict(os.environ, AECM_LIB_PATH=str(build.LIB_CHECKED),
               PYTHONPATH=os.pathsep.join([str(GOLDEN.parent.parent), str(GOLDEN.parent), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("AUDIT")]
    assert line and line[-1].split()[1:] == ["0", "0"], r.stdout[-500:]

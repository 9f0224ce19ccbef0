#!/usr/bin/env python3
"""Generate tests/golden/*.npz from the UNMODIFIED reference (oracle/_ref/libaecm_ref.so).

Run in the build container (needs /root/reference to build the reference .so).  The fixtures hold
only data: generator recipe ids (seed, n_blocks, fs, config) + expected outputs + state digests.
Inputs are regenerated bit-identically by webrtc_aecm_amd.synth on any machine.
"""
import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import pyoracle  # noqa: E402
from webrtc_aecm_amd.synth import synth_clean, synth_pair  # noqa: E402

GOLD = ROOT / "tests" / "golden"

# (seed, n_blocks, fs, cng, echo_mode, profile)
BLOCK_CASES = [
    (0, 1200, 16000, 1, 3, None),
    (1, 1200, 16000, 1, 1, None),
    (2, 1200, 8000, 1, 4, None),
    (3, 1200, 8000, 0, 0, None),
    (100, 4200, 16000, 1, 3, "silent"),
]
# (seed, seconds, fs, frame, cng, echo_mode, ms, with nearendClean = synth_clean(near))
SESSION_CASES = [
    (7, 10, 16000, 160, 1, 1, 40, 0),     # the reference CLI's parameters (main.cc:102-105,163-164)
    (8, 6, 8000, 80, 1, 3, 40, 0),
    (9, 4, 16000, 160, 0, 2, 700, 0),     # ms out of range -> warning path, clamped
    (10, 6, 16000, 160, 1, 3, 40, 1),     # noise suppressor upstream: WebRtcAecm_Process(noisy, clean, ...)
    (11, 4, 8000, 160, 1, 1, 40, 1),
]
# Jittering msInSndCardBuf + far-end underruns (tests/helpers.py: call_pattern): (seed, seconds, fs, frame, cng, echo_mode)
SESSJIT_CASES = [
    (12, 6, 16000, 160, 1, 3),
    (13, 6, 8000, 80, 1, 1),
    (14, 5, 16000, 80, 0, 4),
]
# Far-end bursts (k = 0..3 and 30 WebRtcAecm_BufferFarend calls per WebRtcAecm_Process) + mid-session set_config / InitEchoPath /
# re-Init at the other rate (tests/helpers.py: call_pattern(bursts=True), reconfiguration_events): (seed, seconds, fs, frame)
# Ragged batches (WebRtcAecmBatch_ProcessBlocksRagged): (name, streams, n_blocks, fs, first seed) -- stream s runs its first lens[s]
# blocks (random in [0, n_blocks]; 0, n_blocks and 1 among them) with the configuration tests/helpers.py: stream_config(s) gives it
RAGGED_CASES = [
    ("ragged_16k", 48, 200, 16000, 7000),
]
# The same with a clean near-end input (WebRtcAecm_ProcessBlock's nearendClean): the clean rows are
# tests/test_gpu_pipelined_clean.py: _clean_of of the batch's far / near rows (even streams synth_clean, odd ones a quieter mix)
RAGGED_CLEAN_CASES = [
    ("ragged_clean_16k", 48, 200, 16000, 7100),
]
SESSBURST_CASES = [
    (15, 3, 16000, 160),
    (16, 3, 8000, 80),
]


def main():
    pyoracle.build()
    assert pyoracle.have_reference(), "reference .so missing"
    GOLD.mkdir(parents=True, exist_ok=True)
    only = sys.argv[1] if len(sys.argv) > 1 else ""      # regenerate only the fixtures whose name contains this
    for seed, nb, fs, cng, em, prof in BLOCK_CASES:
        if only and only not in f"block_s{seed}_":
            continue
        far, near = synth_pair(seed, nb, fs, prof)
        r = pyoracle.RefCoreStream(fs, cng, em)
        digs = []
        outs = []
        for c in range(0, nb, 300):
            outs.append(r.process(far[c * 64:(c + 300) * 64], near[c * 64:(c + 300) * 64]))
            digs.append(r.digest())
        out = np.concatenate(outs)
        keep = out if prof is None else out[-600 * 64:]      # long cases: keep the tail + digests only
        np.savez_compressed(GOLD / f"block_s{seed}_fs{fs}_c{cng}_e{em}.npz", seed=seed, n_blocks=nb, fs=fs, cng=cng,
                            echo_mode=em, profile=prof or "", out=keep, digests=np.stack(digs),
                            sha256=hashlib.sha256(out.tobytes()).hexdigest())
        print("block", seed, fs, cng, em, prof, hashlib.sha256(out.tobytes()).hexdigest()[:16])
    for seed, secs, fs, frame, cng, em, ms, with_clean in SESSION_CASES:
        name = f"session_s{seed}_fs{fs}_f{frame}_c{cng}_e{em}_ms{ms}" + ("_clean" if with_clean else "")
        if only and only not in name:
            continue
        nb = secs * fs // 64
        far, near = synth_pair(seed, nb, fs, "mixed")
        clean = synth_clean(near) if with_clean else None
        n = (far.size // frame) * frame
        s = pyoracle.RefSession(fs, cng, em)
        lib = s.lib
        out = near.copy()
        codes = set()
        buf = np.empty(frame, dtype=np.int16)
        for i in range(n // frame):
            f = far[i * frame:(i + 1) * frame]
            d = out[i * frame:(i + 1) * frame]
            c = clean[i * frame:(i + 1) * frame].ctypes.data if with_clean else None
            assert lib.WebRtcAecm_BufferFarend(s.h, f.ctypes.data, frame) == 0
            codes.add(int(lib.WebRtcAecm_Process(s.h, d.ctypes.data, c, buf.ctypes.data, frame, ms)))
            d[:] = buf
        np.savez_compressed(GOLD / f"{name}.npz", seed=seed, n_blocks=nb,
                            fs=fs, frame=frame, cng=cng, echo_mode=em, ms=ms, clean=with_clean, out=out[:n],
                            codes=np.array(sorted(codes)), sha256=hashlib.sha256(out[:n].tobytes()).hexdigest())
        print("session", seed, fs, frame, cng, em, ms, with_clean, sorted(codes))
    sys.path.insert(0, str(ROOT / "tests"))
    from helpers import call_pattern, drive_session
    for seed, secs, fs, frame, cng, em in SESSJIT_CASES:
        name = f"sessjit_s{seed}_fs{fs}_f{frame}_c{cng}_e{em}"
        if only and only not in name:
            continue
        nb = secs * fs // 64
        far, near = synth_pair(seed, nb, fs, "mixed")
        n_calls = far.size // frame
        ms_seq, far_present = call_pattern(seed, n_calls)
        out, codes = drive_session(pyoracle.RefSession(fs, cng, em), far, near, frame, ms_seq, far_present)
        np.savez_compressed(GOLD / f"{name}.npz", seed=seed, n_blocks=nb, fs=fs, frame=frame, cng=cng, echo_mode=em,
                            ms_seq=ms_seq, far_present=far_present, out=out, codes=codes,
                            sha256=hashlib.sha256(out.tobytes()).hexdigest())
        print("sessjit", seed, fs, frame, cng, em, sorted(set(codes.tolist())), int((far_present == 0).sum()), "underruns")
    from helpers import far_frames_needed, reconfiguration_events
    for seed, secs, fs, frame in SESSBURST_CASES:
        name = f"sessburst_s{seed}_fs{fs}_f{frame}"
        if only and only not in name:
            continue
        n_calls = secs * fs // frame
        ms_seq, far_calls = call_pattern(seed, n_calls, bursts=True)
        far, _ = synth_pair(seed, far_frames_needed(far_calls) * frame // 64 + 1, fs, "mixed")
        _, near = synth_pair(seed, n_calls * frame // 64 + 1, fs, "mixed")
        r = pyoracle.RefSession(fs, 1, 3)
        out, codes = drive_session(r, far, near, frame, ms_seq, far_calls, events=reconfiguration_events(fs, n_calls))
        np.savez_compressed(GOLD / f"{name}.npz", seed=seed, n_calls=n_calls, fs=fs, frame=frame, ms_seq=ms_seq, far_calls=far_calls, out=out,
                            codes=codes, paths=np.stack(r.event_log), sha256=hashlib.sha256(out.tobytes()).hexdigest())
        print("sessburst", seed, fs, frame, sorted(set(codes.tolist())), int(far_calls.sum()), "far calls for", n_calls, "near calls")
    # Sparse session ticks (AECM_SESSION_IDLE; tests/sparse_helpers.py: golden_pattern): every session on a reference instance
    # of its own that in an idle tick is not called.  Arrays only: the recipe's seeds, the flags and msInSndCardBuf of every
    # tick, the outputs (an idle tick: zeros), the codes and the final echo paths.
    import sparse_helpers
    for name, (fs, frame, seed) in sparse_helpers.GOLDEN_CASES.items():
        if only and only not in name:
            continue
        flags, ms = sparse_helpers.golden_pattern(fs, frame, seed)
        T, S = flags.shape
        far, near, _ = sparse_helpers.signals(seed, S, T * frame, fs)
        out, codes, paths = sparse_helpers.drive_reference(lambda: pyoracle.RefSession(fs, 1, 3), fs, flags, ms, np.full(T, frame), far, near)
        np.savez_compressed(GOLD / f"{name}.npz", seed=seed, fs=fs, frame=frame, flags=flags, ms=ms, out=out, codes=codes.astype(np.int16), paths=paths)
        print("sesssparse", fs, frame, "live calls", int(((flags & 4) == 0).sum()), "of", T * S, sorted(set(codes.ravel().tolist())))
    # Ticks of K call pairs (WebRtcAecmSessions_TickCalls; tests/calls_helpers.py: golden_pattern): 9 sessions x 48 calls, every
    # session on a reference instance of its own that makes the K pairs of a tick in order (far, near, far, near, ...) and is not
    # called in an idle tick.  Arrays only: the recipe's seed and K, per-tick flags and msInSndCardBuf, outputs, codes, final echo paths.
    import calls_helpers
    for name, (fs, frame, K, seed) in calls_helpers.GOLDEN_CASES.items():
        if only and only not in name:
            continue
        flags, ms = calls_helpers.golden_pattern(frame, K, seed)
        far, near, _ = sparse_helpers.signals(seed, calls_helpers.GOLDEN_S, calls_helpers.GOLDEN_CALLS * frame, fs)
        out, codes, refs = calls_helpers.run_reference(lambda: pyoracle.RefSession(fs, 1, 3), calls_helpers.calls_ops(K, frame, flags, ms),
                                                       calls_helpers.Feed(far, near))
        paths = np.stack([r.get_echo_path()[1] for r in refs])
        np.savez_compressed(GOLD / f"{name}.npz", seed=seed, fs=fs, frame=frame, calls=K, flags=flags, ms=ms, out=out, codes=codes.astype(np.int16), paths=paths)
        print("sesscalls", fs, frame, K, "live calls", int(((flags & 4) == 0).sum()) * K, sorted(set(codes.ravel().tolist())))
    # Objects of mixed rates and call sizes (WebRtcAecmSessions_InitRates, AECM_SESSION_HALF_CALL; tests/mixed_helpers.py: the mixed
    # run): every session on a reference instance of its own, initialised at ITS rate and called with ITS sizes.  Arrays only:
    # the seed, the per-session rates, flags, msInSndCardBuf and burst calls of every tick, outputs, codes, final echo paths --
    # once without and once with a clean input (the clean rows: synth_clean of the near rows).
    import mixed_helpers as mh
    for name, (seed, idle_p, with_bursts) in mh.GOLDEN_CASES.items():
        if only and only not in name:
            continue
        flags, ms = mh.mixed_pattern(seed, idle_p=idle_p)
        T, S = flags.shape
        bursts = mh.burst_pattern(seed) if with_bursts else np.zeros((T, S), np.uint8)
        burst_far = mh.burst_signals(seed)
        far, near, clean = mh.signals(seed, mh.RATES, T * 160, with_clean=True)
        make = lambda fs: pyoracle.RefSession(fs, 1, 3)
        res = {}
        for key, c in (("", None), ("_clean", clean)):
            out, codes, paths, _, active = mh.drive_reference(make, mh.RATES, flags, ms, 160, far, near, c, bursts, burst_far)
            res.update({"out" + key: out, "codes" + key: codes.astype(np.int16), "paths" + key: paths, "active_from" + key: active.astype(np.int16)})
        np.savez_compressed(GOLD / f"{name}.npz", seed=seed, object_fs=mh.OBJECT_FS, rates=mh.RATES, flags=flags, ms=ms, bursts=bursts, **res)
        print("sessmixed", name, "half calls", int((((flags & 8) != 0) & ((flags & 4) == 0)).sum()), "active from", res["active_from"].tolist(),
              sorted(set(res["codes"].ravel().tolist())))
    # Packet ticks (WebRtcAecmSessions_TickPackets; tests/packets_helpers.py: golden_pattern): the 9 sessions and rates of the mixed
    # run, 48 calls each in packets of K, every session on a reference instance at ITS rate making its K calls of ITS size (80 with
    # a half flag) in order on packed rows.  Arrays only: flags, msInSndCardBuf, outputs (zeros where no call delivers), codes, paths.
    import packets_helpers as ph
    for name, (fs, frame, K, seed) in ph.GOLDEN_CASES.items():
        if only and only not in name:
            continue
        flags, ms = ph.golden_pattern(K, seed)
        far, near, _ = mh.signals(seed, mh.RATES, ph.GOLDEN_CALLS * frame)
        out, codes, refs = ph.run_reference(lambda rate: pyoracle.RefSession(rate, 1, 3), mh.RATES, ph.packets_ops(K, frame, flags, ms), ph.Feed(far, near))
        paths = np.stack([r.get_echo_path()[1] for r in refs])
        np.savez_compressed(GOLD / f"{name}.npz", seed=seed, fs=fs, frame=frame, calls=K, rates=mh.RATES, flags=flags, ms=ms, out=out,
                            codes=codes.astype(np.int16), paths=paths)
        print("sesspackets", fs, frame, K, "half packets", int((((flags & 8) != 0) & ((flags & 4) == 0)).sum()), sorted(set(codes.ravel().tolist())))
    # K-call ticks with a clean near-end input per session (WebRtcAecmSessions_SetSplitCallTicks; tests/split_calls_helpers.py:
    # golden_pattern): the 11 sessions of the split run, those of NEVER11 on instances whose every Process gets nearendClean = NULL,
    # the others their clean rows, 48 calls each in ticks of K.  Arrays only: flags, msInSndCardBuf, outputs, codes, paths.
    import split_calls_helpers as sch
    import split_helpers as sph
    for name, (fs, frame, K, seed) in sch.GOLDEN_CASES.items():
        if only and only not in name:
            continue
        flags, ms = sch.golden_pattern(K, seed)
        far, near, clean = sparse_helpers.signals(seed, sph.S11, sch.GOLDEN_CALLS * frame, fs, with_clean=True)
        refs = sch.reference_sessions(lambda rate: pyoracle.RefSession(rate, 1, 3), [fs] * sph.S11, sph.NEVER11)
        out, codes, _ = calls_helpers.run_reference(None, calls_helpers.calls_ops(K, frame, flags, ms),
                                                    calls_helpers.Feed(far, near, sph.object_clean(clean, sph.NEVER11)), sessions=refs)
        paths = np.stack([r.get_echo_path()[1] for r in refs])
        np.savez_compressed(GOLD / f"{name}.npz", seed=seed, fs=fs, frame=frame, calls=K, never=np.array(sph.NEVER11, dtype=np.int32), flags=flags, ms=ms,
                            out=out, codes=codes.astype(np.int16), paths=paths)
        print("sesssplitcalls", fs, frame, K, "live calls", int(((flags & 4) == 0).sum()) * K, sorted(set(codes.ravel().tolist())))
    # The block corpus as sessions (tests/corpus_sessions.py): every case of a rate without a clean input as one session, ordinary
    # ticks with call_pattern delays and underruns for the whole case.  Kept: the output tail, a SHA-256 of the whole output, the
    # non-zero codes and the final echo paths.
    import corpus_sessions as cs
    for name, fs in cs.GOLDEN_CASES.items():
        if only and only not in name:
            continue
        cases = cs.session_cases(fs)
        ops, far, near, rates = cs.plan(cases, fs)
        refs = [cs.configure_session(pyoracle.RefSession(c["fs"], 1, 3), c) for c in cases]
        out, codes, refs = ph.run_reference(None, rates, ops, ph.Feed(far, near), sessions=refs)
        np.savez_compressed(GOLD / f"{name}.npz", fs=fs, names=np.array([c["name"] for c in cases]),
                            **cs.summary(cases, out, codes, np.stack([r.get_echo_path()[1] for r in refs])))
        print("sesscorpus", fs, len(cases), "sessions", len(ops), "ticks")
    # The session-flow corpus (tests/flow_corpus.py): every object of it, one reference instance per session at the session's rate and
    # call sizes.  Kept: a SHA-256 of every session's output, the non-zero codes and the final echo paths.
    import flow_corpus as fc
    for family, name in fc.GOLDEN_NAMES.items():
        if only and only not in name:
            continue
        sch = fc.family_schedule(family)
        far, near = fc.signals(sch)
        out, codes, paths = fc.drive_reference(sch, far, near, lambda rate: pyoracle.RefSession(rate, 1, 3))
        np.savez_compressed(GOLD / f"{name}.npz", **fc.summary(out, codes, paths))
        print("sessflow", family, out.shape, "codes", int((codes != 0).sum()))
    # The session surface fuzz (tests/surface_fuzz.py): per case the SHA-256 of the program and of what the reference answers to it
    # (every code, every output row, the echo paths).
    if not only or only in "session_surface_fuzz":
        import json
        import surface_fuzz as sf
        pins = {}
        for case in sorted(sf.CASES):
            prog = sf.generate(case)
            pins[case] = dict(program=sf.program_sha256(prog), expected=sf.run_reference(case, prog).digest.hexdigest())
            print("surface fuzz", case, len(prog), "ops")
        (GOLD / "session_surface_fuzz.json").write_text(json.dumps(pins, indent=1, sort_keys=True) + "\n")
    from helpers import stream_config
    for name, S, nb, fs, seed0 in RAGGED_CASES:
        if only and only not in name:
            continue
        lens = np.random.RandomState(seed0).randint(0, nb + 1, size=S).astype(np.int32)
        lens[:3] = (0, nb, 1)
        seeds = np.arange(seed0, seed0 + S)
        cfgs = [stream_config(s) for s in range(S)]
        hashes, digs = [], []
        for s in range(S):
            far, near = synth_pair(int(seeds[s]), nb, fs)
            r = pyoracle.RefCoreStream(fs, *cfgs[s])
            out = r.process(far[:lens[s] * 64], near[:lens[s] * 64]) if lens[s] else np.zeros(0, np.int16)
            hashes.append(hashlib.sha256(out.tobytes()).hexdigest())
            digs.append(r.digest())
        np.savez_compressed(GOLD / f"{name}.npz", fs=fs, n_blocks=nb, lens=lens, seeds=seeds, cng=np.array([c[0] for c in cfgs]),
                            echo_mode=np.array([c[1] for c in cfgs]), sha256=np.array(hashes), digests=np.stack(digs))
        print("ragged", name, S, nb, fs, int(lens.sum()), "blocks")
    for name, S, nb, fs, seed0 in RAGGED_CLEAN_CASES:
        if only and only not in name:
            continue
        from helpers import process_clean, synth_streams
        from test_gpu_pipelined_clean import _clean_of
        lens = np.random.RandomState(seed0).randint(0, nb + 1, size=S).astype(np.int32)
        lens[:3] = (0, nb, 1)
        seeds = np.arange(seed0, seed0 + S)
        cfgs = [stream_config(s) for s in range(S)]
        far, near = synth_streams(seeds.tolist(), nb, fs)
        clean = _clean_of(far, near)
        hashes, digs = [], []
        for s in range(S):
            r = pyoracle.RefCoreStream(fs, *cfgs[s])
            out = process_clean(r, far[s], near[s], clean[s], 0, int(lens[s]))
            hashes.append(hashlib.sha256(out.tobytes()).hexdigest())
            digs.append(r.digest())
        np.savez_compressed(GOLD / f"{name}.npz", fs=fs, n_blocks=nb, lens=lens, seeds=seeds, cng=np.array([c[0] for c in cfgs]),
                            echo_mode=np.array([c[1] for c in cfgs]), sha256=np.array(hashes), digests=np.stack(digs))
        print("ragged clean", name, S, nb, fs, int(lens.sum()), "blocks")
    if only:
        return
    # 60 s reference-CLI-shaped run: hash only
    far, near = synth_pair(60, 15000, 16000, "mixed")
    s = pyoracle.RefSession(16000, 1, 1)
    out = s.run(far, near, 160, 40)
    (GOLD / "session_60s_16k.sha256").write_text(hashlib.sha256(out.tobytes()).hexdigest() + "\n")
    print("60 s hash", hashlib.sha256(out.tobytes()).hexdigest()[:16])


if __name__ == "__main__":
    main()

"""Shared by tests/test_block_trace.py and tests/test_gpu_block_trace.py: the reference tracks of the block trace -- what a CPU
checker's state shows after every block, read through its 24-word digest (oracle/ref_shim.cc: refshim_core_digest,
aecm_host_state.cpp: ComputeDigest) -- as webrtc_aecm_amd.ffi.BLOCK_TRACE_DTYPE records.  Computed once per process."""
from __future__ import annotations

import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from helpers import checker_name, stream_config
from oracle import pyoracle
from webrtc_aecm_amd.ffi import BLOCK_TRACE_DTYPE
from webrtc_aecm_amd.synth import synth_clean, synth_pair

N_STREAMS, N_BLOCKS = 6, 1100          # 1 100: the smallest length past both start-up thresholds (totCount 512 and 1 024)
SEEDS = tuple(range(100, 100 + N_STREAMS))
RATES = tuple(16000 if s % 2 == 0 else 8000 for s in range(N_STREAMS))
CONFIGS = tuple(stream_config(s) for s in range(N_STREAMS))
# include/aecm_batch.h: AecmBlockTrace -- (field, offset)
LAYOUT = (("tot_count", 0), ("delay", 4), ("startup_state", 6), ("vad", 8), ("vad_update_count", 10), ("far_log_energy", 12),
          ("far_energy_min", 14), ("far_energy_max", 16), ("far_energy_vad", 18), ("sup_gain", 20), ("near_q", 22),
          ("delay_min_probability", 24), ("delay_last_probability", 28))


def checker_class():
    return pyoracle.RefCoreStream if checker_name() == "reference" else pyoracle.OracleStream


def records_of_digests(d):
    """digests [..., 24] uint32 -> BLOCK_TRACE_DTYPE records [...] by the table of include/aecm_batch.h."""
    d = np.asarray(d, dtype=np.uint32)
    lo = lambda w: (d[..., w] & 0xffff).astype(np.uint16).view(np.int16)
    hi = lambda w: (d[..., w] >> 16).astype(np.uint16).view(np.int16)
    r = np.zeros(d.shape[:-1], dtype=BLOCK_TRACE_DTYPE)
    r["tot_count"] = d[..., 0]
    r["delay"] = lo(13)
    r["startup_state"] = lo(2)
    r["vad"], r["vad_update_count"] = lo(7), hi(7)
    r["far_log_energy"], r["far_energy_min"] = lo(4), hi(4)
    r["far_energy_max"] = lo(5)
    r["far_energy_vad"] = lo(6)
    r["sup_gain"] = lo(12)
    r["near_q"] = lo(3)
    r["delay_min_probability"] = d[..., 14].view(np.int32)
    r["delay_last_probability"] = d[..., 15].view(np.int32)
    return r


def _track(fs, cfg, far, near, clean=None):
    """(out, digests [T, 24]) of one stream on the CPU checker, driven one block at a time."""
    o = checker_class()(fs, *cfg)
    T = far.size // 64
    out, dig = np.empty(T * 64, np.int16), np.empty((T, 24), np.uint32)
    for b in range(T):
        sl = slice(b * 64, (b + 1) * 64)
        out[sl] = o.process(far[sl], near[sl]) if clean is None else o.process_block_clean(far[sl], near[sl], clean[sl])
        dig[b] = o.digest()
    return out, dig


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def main_inputs():
    """(far, near) [6, 1100 * 64]: seeds 100..105, rates alternating 16 000 / 8 000."""
    pairs = [synth_pair(seed, N_BLOCKS, fs) for seed, fs in zip(SEEDS, RATES)]
    return _frozen(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))


@functools.lru_cache(maxsize=None)
def main_tracks():
    """(out [6, 1100 * 64], digests [6, 1100, 24], records [6, 1100]) of the main inputs on the CPU checker."""
    far, near = main_inputs()
    with ThreadPoolExecutor() as ex:
        res = list(ex.map(lambda s: _track(RATES[s], CONFIGS[s], far[s], near[s]), range(N_STREAMS)))
    out, dig = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    return _frozen(out, dig, records_of_digests(dig))


def assert_tracks_are_alive(rec):
    """What the issue demands of the REFERENCE track before anything is compared with it: a trace of constants cannot pass."""
    for s in range(rec.shape[0]):
        assert {0, 1, 2} <= set(rec["startup_state"][s].tolist()), s
        assert {0, 1} <= set(rec["vad"][s].tolist()), s
        assert rec["delay"][s, 0] == -2, s
    assert sum(len(set(rec["delay"][s].tolist())) >= 4 for s in range(rec.shape[0])) >= 3


CLEAN_STREAMS, CLEAN_BLOCKS = 4, 64


@functools.lru_cache(maxsize=None)
def clean_tracks():
    """Four streams x 64 blocks with a clean near-end input (synth_clean), 16 kHz: (far, near, clean, out, digests, records)."""
    pairs = [synth_pair(200 + s, CLEAN_BLOCKS, 16000) for s in range(CLEAN_STREAMS)]
    far, near = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    clean = synth_clean(near)
    res = [_track(16000, stream_config(s), far[s], near[s], clean[s]) for s in range(CLEAN_STREAMS)]
    out, dig = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    return _frozen(far, near, clean, out, dig, records_of_digests(dig))


def first_record_difference(got, want):
    """None, or (index tuple, field, got, want) of the first differing field."""
    for name in BLOCK_TRACE_DTYPE.names:
        bad = np.argwhere(got[name] != want[name])
        if bad.size:
            i = tuple(int(x) for x in bad[0])
            return i, name, got[name][i].item(), want[name][i].item()
    return None

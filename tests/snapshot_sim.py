"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_snapshot.so -- tests/sim/sim_snapshot.cpp: the routines of the bulk session-snapshot
kernels (webrtc_aecm_amd/csrc/aecm_session_snapshot.h) on a host image of an object's arrays, against a restatement of
ExportSession / ImportSession.  Header-only on the product's side: it needs nothing of the lane simulator."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_snapshot.cpp"
SO = simlib.SIM_SO.parent / ("libaecm_sim_snapshot_san.so" if simlib.SANITIZE else "libaecm_sim_snapshot.so")
_lib = None


def build():
    deps = [SRC] + [simlib.CSRC / h for h in ("aecm_session_snapshot.h", "aecm_flow_plan.h", "aecm_state.h", "aecm_state_check.h")]
    if SO.exists() and all(SO.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return
    SO.parent.mkdir(parents=True, exist_ok=True)
    flags = [*(simlib.SAN_FLAGS if simlib.SANITIZE else ["-O2"]), "-std=c++17", "-fwrapv", "-fPIC", f"-I{simlib.CSRC}"]
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.check_call(["g++", *flags, "-shared", str(SRC), "-o", str(tmp)])
    os.replace(tmp, SO)


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(str(SO))
        l.sim_snapshot_bytes.restype = C.c_size_t
        l.sim_snapshot_gather.restype = C.c_int64
        l.sim_snapshot_gather.argtypes = [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int, C.c_int]
        l.sim_snapshot_scatter.restype = C.c_int64
        l.sim_snapshot_scatter.argtypes = [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_uint32,
                                           C.c_int32, C.c_int, C.c_int]
        l.sim_snapshot_scatter_coverage.restype = C.c_int64
        l.sim_snapshot_scatter_coverage.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int32, C.c_int]
        l.sim_snapshot_defect_run.restype = C.c_int64
        l.sim_snapshot_defect_run.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_void_p]
        l.sim_snapshot_defect_case.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        _lib = l
    return _lib


def gather(seed, session, blk_pos, near_pos, lag, deferred_lag, has_clean, wide=True):
    """-1, or the first byte at which SessionGatherPart's snapshot differs from the restatement of ExportSession."""
    return lib().sim_snapshot_gather(seed, session, blk_pos & 0xffffffff, near_pos & 0xffffffff, lag, deferred_lag, int(has_clean), int(wide))


def scatter(seed, session, blk_pos, near_pos_a, lag, deferred_a, clean_a, s2, slot, near_pos_b, deferred_b, clean_b, wide=True):
    """0; 1: the scattered image differs from the restatement of ImportSession; 2 + byte: the slot gathered again differs."""
    return lib().sim_snapshot_scatter(seed, session, blk_pos & 0xffffffff, near_pos_a & 0xffffffff, lag, deferred_a, int(clean_a), s2, slot,
                                      near_pos_b & 0xffffffff, deferred_b, int(clean_b), int(wide))


def scatter_coverage(seed, blk_pos, near_pos_b, deferred_b, wide=True):
    return lib().sim_snapshot_scatter_coverage(seed, blk_pos & 0xffffffff, near_pos_b & 0xffffffff, deferred_b, int(wide))


def defect_run(seed, fs, n_ticks):
    """(first refused tick or -1, {defect, states, after_burst})."""
    detail = np.zeros(3, dtype=np.int64)
    tick = lib().sim_snapshot_defect_run(seed, fs, n_ticks, detail.ctypes.data)
    return tick, dict(zip(("defect", "states", "after_burst"), detail.tolist()))


def defect_case(which, fs_blob=16000, fs_object=16000, any_rate=False):
    return lib().sim_snapshot_defect_case(which, fs_blob, fs_object, int(any_rate))

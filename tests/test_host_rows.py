"""The host-audio staging layer (webrtc_aecm_amd/csrc/aecm_host_rows.h) without a GPU: PackRows / UnpackRows between a caller's strided
rows and dense planes, the far | near | [clean] | out view and the stream offset of StatePtrs.  The checks are tests/sim/sim_host_rows.cpp's:
seeded layouts (dense, padded stream stride, tick-major, both padded) x lengths (none, all T, mixed with zeros, all zero) x S = 1, 3, 8
x T = 1, 3, 5, every buffer allocated to its exact extent and pre-filled with a sentinel, against a sample-by-sample restatement.
The program is built with AddressSanitizer and UBSan and run as a child process: nothing sanitized is loaded into python."""
import os
import subprocess

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_host_rows.cpp"
EXE = simlib.SIM_SO.parent / "sim_host_rows_main_san"
DEPS = [SRC, simlib.CSRC / "aecm_host_rows.h", simlib.CSRC / "aecm_state.h"]


def standalone():
    if not (EXE.exists() and all(EXE.stat().st_mtime >= d.stat().st_mtime for d in DEPS)):
        EXE.parent.mkdir(parents=True, exist_ok=True)
        tmp = EXE.with_suffix(f".{os.getpid()}.tmp")
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-fwrapv",
                               f"-I{simlib.CSRC}", str(SRC), "-o", str(tmp)])
        os.replace(tmp, EXE)
    return EXE


def test_header_needs_no_hip():
    """The staging layer is host logic: neither header it is made of names a HIP header."""
    for h in DEPS[1:]:
        assert "hip/" not in h.read_text(), h


def test_pack_unpack_and_views_under_sanitizers():
    run = subprocess.run([str(standalone())], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
    assert "180 cases, 0 failures" in run.stdout, run.stdout      # 3 sizes of S x 3 of T x 5 layouts x 4 kinds of lengths

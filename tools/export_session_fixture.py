#!/usr/bin/env python3
"""Write tests/golden/sesssnap_parent_fs16000.npz (run ON THE GPU BOX, from a checkout of the commit whose snapshot layout is to
be kept importable -- the fixture in the tree was written by commit b09b76d, the last one before sessions could sit out ticks):
one session of a one-session object makes 33 ticks of 160 samples (msInSndCardBuf 40; the signal of session 3 of
tests/sparse_helpers.py: signals(800, 9, ...)), then WebRtcAecmSessions_ExportSession.  Arrays only: the recipe and the blob.

    python tools/export_session_fixture.py OUT.npz [TESTS_DIR]      # TESTS_DIR: where sparse_helpers.py lives (default: tests/)
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.append(sys.argv[2] if len(sys.argv) > 2 else str(ROOT / "tests"))

import sparse_helpers as sh  # noqa: E402
import webrtc_aecm_amd as aecm  # noqa: E402

FS, N, TICKS, SEED, SESSION = 16000, 160, 33, 800, 3


def main():
    far, near, _ = sh.signals(SEED, 9, 70 * N, FS)
    sb = aecm.AecmSessions(1, FS, 1, 3)
    for t in range(TICKS):
        sl = slice(t * N, (t + 1) * N)
        rc, _, _ = sb.tick_host_per_session(far[SESSION:SESSION + 1, sl], near[SESSION:SESSION + 1, sl], np.array([40], dtype=np.int16))
        assert rc == 0
    rc, snap = sb.export_session(0)
    assert rc == 0
    np.savez_compressed(sys.argv[1], fs=FS, frame=N, ticks=TICKS, seed=SEED, session=SESSION, snapshot=np.frombuffer(snap, dtype=np.uint8))
    print("wrote", sys.argv[1], len(snap), "bytes of snapshot; library", aecm.library_path())


if __name__ == "__main__":
    main()

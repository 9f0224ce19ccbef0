"""Bulk session snapshots without a GPU: the routines the gather / scatter / validation kernels run (aecm_session_snapshot.h), on a
host image of an object's device arrays (tests/sim/sim_snapshot.cpp), against a restatement of ExportSession / ImportSession; and
the new calls' place in the C ABI."""
import itertools

import pytest

import snapshot_sim as sim

RING = 8192
BLK_POS = [0, 64, 128, 192, 8128]                         # F_BLK_POS mod 8192: the out tail ends at / wraps round the ring's end
NEAR_POS = [0, 16, 32, 48, 80]                            # near_pos mod 8192: the near tail wraps round the ring's end
EPOCHS = [5 * RING, 2 ** 32 - RING, 2 ** 32]              # somewhere, just below 2^32 (the tails cross it), just above (wrapped)
LAGS = [0, 80, 160, 40880]
DEFERRED = [0, 160]


def test_layout():
    assert sim.lib().sim_snapshot_bytes() == 34304


@pytest.mark.parametrize("has_clean", [False, True])
@pytest.mark.parametrize("wide", [True, False])
def test_gather_equals_the_restatement(has_clean, wide):
    """SessionGatherPart, 256 workers in a shuffled order, writes ExportSession's bytes: every F_BLK_POS and near position at
    which a tail crosses the ring's end, positions on both sides of 2^32, every lag with and without deferred all-idle ticks, each
    of the three sessions of the image, into a 16-byte-aligned buffer and into one that is only 4-byte aligned."""
    seed = 0
    for epoch, b, n in itertools.product(EPOCHS, BLK_POS, NEAR_POS):
        for lag, deferred in itertools.product(LAGS, DEFERRED):
            seed += 1
            if (seed % 4) and not (b in (64, 8128) and n == 16):      # every position pair with one lag pair in four, two pairs with all
                continue
            got = sim.gather(seed, seed % 3, epoch + b, epoch * 3 + n, lag, deferred, has_clean, wide)
            assert got == -1, (epoch, b, n, lag, deferred, "first differing byte", got)


@pytest.mark.parametrize("clean_a,clean_b", [(False, False), (True, True), (False, True)])
@pytest.mark.parametrize("wide", [True, False])
def test_scatter_equals_the_restatement(clean_a, clean_b, wide):
    """SessionScatterPart into an image of another S, near position and deferred lag leaves what ImportSession leaves in every
    row of every session (untouched near-ring samples kept, the out row zero but for the tail, no other slot written), and the slot
    gathered again is the snapshot."""
    seed = 1000
    for epoch, b, n in itertools.product(EPOCHS, BLK_POS, NEAR_POS):
        seed += 1
        lag, deferred_a = LAGS[seed % 4], DEFERRED[seed % 2]
        s2 = 1 + seed % 5
        for deferred_b in DEFERRED:
            got = sim.scatter(seed, seed % 3, epoch + b, epoch + 7 * 80, lag, deferred_a, clean_a, s2, (seed // 3) % s2, epoch * 5 + n, deferred_b, clean_b, wide)
            assert got == 0, (epoch, b, n, lag, deferred_a, deferred_b, s2, got)


@pytest.mark.parametrize("wide", [True, False])
def test_scatter_writes_every_element_once(wide):
    for b, n in ((0, 0), (64, 16), (8128, 48), (2 ** 32 - 64, 2 ** 32 - 16), (77, 5)):      # (77: a tail that starts inside a 16-byte group)
        assert sim.scatter_coverage(5 + b, b, n, 160, wide) == 0, (b, n)


@pytest.mark.parametrize("fs", [8000, 16000])
def test_every_state_of_a_run_is_accepted(fs):
    """SessionBlobDefect accepts every state of a 200-tick run with far-end bursts between the ticks -- the state right after a
    burst and before the next Process included, a legal export point -- with lag words as after idle ticks among them."""
    for seed in range(6):
        tick, d = sim.defect_run(seed, fs, 200)
        assert tick == -1, (seed, tick, d)
        assert d["after_burst"] >= 30 and d["states"] == 200 + d["after_burst"], d


def test_defect_matrix():
    assert sim.defect_case(0) == 0
    for which, what in ((1, "magic"), (2, "version"), (3, "lag 81"), (4, "an unused wrapper word"), (5, "pending 64"), (6, "a core scalar"),
                        (7, "a core state of another rate than the header's")):
        assert sim.defect_case(which) != 0, what
        assert sim.defect_case(which, 8000, 8000, True) != 0, what
    # the rate rule: ImportSession's without any_rate, ImportSessionAnyRate's with
    assert sim.defect_case(0, 8000, 16000, False) != 0 and sim.defect_case(0, 16000, 8000, False) != 0
    assert sim.defect_case(0, 8000, 16000, True) == 0 and sim.defect_case(0, 16000, 8000, True) == 0
    assert sim.defect_case(0, 8000, 8000, False) == 0
    # which rule fires: the codes of aecm_session_snapshot.h
    assert sim.defect_case(1) == 1 and sim.defect_case(0, 8000, 16000) == 2 and sim.defect_case(7) == 3
    assert sim.defect_case(3) == 0x100 + 26 and sim.defect_case(4) == 0x100 + 32 and sim.defect_case(5) == 0x100 + 17 and sim.defect_case(6) >= 0x200


def test_the_four_calls_are_declared_exported_and_bound():
    import ctypes
    from webrtc_aecm_amd import build, ffi
    lib = ctypes.CDLL(str(build.build()))
    header = (sim.simlib.ROOT / "include" / "aecm_batch.h").read_text()
    for name in ("ExportSessions", "ImportSessions", "ExportSessionsDevice", "ImportSessionsDevice"):
        sym = "WebRtcAecmSessions_" + name
        assert sym in ffi.SESSIONS_SYMBOLS and hasattr(lib, sym) and f"int32_t {sym}(" in header, sym
    for method in ("export_sessions", "import_sessions", "export_sessions_device", "import_sessions_device"):
        assert callable(getattr(ffi.AecmSessions, method))
    assert "256 snapshots" in header                       # the host forms' stage is documented like the Batch forms' 8 192
    # a null handle is refused before anything else, as everywhere in the ABI
    ffi.load()
    assert ffi.load().WebRtcAecmSessions_ExportSessions(None, None, 0, None, 0) == -1


def test_the_new_kernel_unit_is_built_like_the_others():
    """aecm_session_snapshot_kernels.hip is a kernel unit of both recipes (test_capi compares what they build), with no flags of its
    own; the gather / scatter kernels exist for both alignments and move 16 bytes per lane in the wide form."""
    import re
    from webrtc_aecm_amd import build, isa_census
    assert "aecm_session_snapshot_kernels.hip" in build.KERNEL_SOURCES and "aecm_session_snapshot_kernels.hip" not in build.SOURCE_FLAGS
    assert "aecm_session_snapshot_kernels.hip" in (sim.simlib.ROOT / "CMakeLists.txt").read_text()
    text = isa_census.disassemble(build.build())
    kernels = isa_census.census_of_text(text)
    for sub in (r"aecm_gather_sessions_kernelILb1E", r"aecm_gather_sessions_kernelILb0E", r"aecm_scatter_sessions_kernelILb1E",
                r"aecm_scatter_sessions_kernelILb0E", r"aecm_validate_sessions_kernel"):
        hits = [k for k in kernels if re.search(sub, k)]
        assert len(hits) == 1, sub
        ops = kernels[hits[0]]["opcodes"]
        assert not any(op.startswith("scratch_") for op in ops), sub
        if "ILb1E" in sub:
            assert ops.get("global_load_dwordx4", 0) >= 6 and ops.get("global_store_dwordx4", 0) >= 6, (sub, ops)
        elif "ILb0E" in sub:
            assert "global_load_dwordx4" not in ops or "gather" in sub, (sub, ops)

"""The block trace without a device: the traced block loop (BlockEngine::run_stream_traced, aecm_wave.h) on the lane simulator
against the CPU checker's state after every block, the record's layout, the launch rule of a traced batch, and the C ABI's
device-free doors.  The GPU side is tests/test_gpu_block_trace.py."""
import ctypes

import numpy as np
import pytest

import launch_table as lt
import simlib
import trace_helpers as th
import trace_sim
import webrtc_aecm_amd as aecm
from helpers import describe_digest_diff
from webrtc_aecm_amd import ffi


def _sim_streams():
    return [simlib.SimStream(th.RATES[s], *th.CONFIGS[s]) for s in range(th.N_STREAMS)]


def _untraced_sim():
    far, near = th.main_inputs()
    streams = _sim_streams()
    out = np.stack([streams[s].process(far[s], near[s]) for s in range(th.N_STREAMS)])
    return out, np.stack([s.digest() for s in streams])


@pytest.mark.parametrize("chunk", [0, 48], ids=["one run per stream", "chunks of 48"])
def test_traced_block_loop_on_the_lane_simulator(chunk):
    """Six streams x 1 100 blocks through run_stream_traced -- whole, and in runs of 48 blocks with the state stored and reloaded
    in between (1 100 = 22 x 48 + 44), as the queue kernels run it.  Every field of every record equals the checker's state after
    that block; audio and final digests equal the untraced simulator's (and the checker's)."""
    far, near = th.main_inputs()
    ref_out, ref_dig, ref_rec = th.main_tracks()
    th.assert_tracks_are_alive(ref_rec)
    streams = _sim_streams()
    out, rec, n = trace_sim.traced_launch(streams, far, near, chunk_blocks=chunk)
    assert n == th.N_STREAMS * th.N_BLOCKS
    assert th.first_record_difference(rec, ref_rec) is None, th.first_record_difference(rec, ref_rec)
    plain_out, plain_dig = _untraced_sim()
    assert np.array_equal(out, plain_out) and np.array_equal(out, ref_out)
    for s, st in enumerate(streams):
        d = st.digest()
        assert np.array_equal(d, plain_dig[s]) and np.array_equal(d, ref_dig[s, -1]), (s, describe_digest_diff(d, ref_dig[s, -1]))


def test_traced_block_loop_ragged_layouts_and_continuity():
    """The index arithmetic on the simulator: ragged lengths write records 0 .. L - 1 and nothing else (0xA5 fill, stream stride
    44 for 41 blocks); a tick-major layout holds the same records as a stream-major one; two launches of 30 + 34 blocks give the
    records of one of 64, with k restarting at 0 and tot_count running on."""
    far, near = th.main_inputs()
    _, _, ref_rec = th.main_tracks()
    lens = np.array([0, 1, 7, 8, 9, 41], dtype=np.int32)
    T, stride = 41, 44
    for chunk in (0, 8):
        raw = np.full(th.N_STREAMS * stride * 32, 0xA5, np.uint8)
        trace = raw.view(ffi.BLOCK_TRACE_DTYPE)
        out, _, n = trace_sim.traced_launch(_sim_streams(), far[:, :T * 64], near[:, :T * 64], lens=lens, chunk_blocks=chunk, trace=trace,
                                            trace_strides=(stride, 1))
        assert n == int(lens.sum())
        rows = raw.reshape(th.N_STREAMS, stride, 32)
        for s, L in enumerate(lens):
            assert th.first_record_difference(trace.reshape(th.N_STREAMS, stride)[s, :L], ref_rec[s, :L]) is None, (chunk, s)
            assert (rows[s, L:] == 0xA5).all(), (chunk, s)
            assert (out[s, L * 64:] == 0x5A5A).all()
    S = th.N_STREAMS
    tick_major = np.zeros(64 * S, dtype=ffi.BLOCK_TRACE_DTYPE)
    trace_sim.traced_launch(_sim_streams(), far[:, :64 * 64], near[:, :64 * 64], trace=tick_major, trace_strides=(1, S))
    assert th.first_record_difference(tick_major.reshape(64, S).T, ref_rec[:, :64]) is None
    streams = _sim_streams()
    _, a, _ = trace_sim.traced_launch(streams, far[:, :30 * 64], near[:, :30 * 64])
    _, b, _ = trace_sim.traced_launch(streams, far[:, 30 * 64:64 * 64], near[:, 30 * 64:64 * 64])
    both = np.concatenate([a, b], axis=1)
    assert th.first_record_difference(both, ref_rec[:, :64]) is None
    assert (both["tot_count"] == np.arange(1, 65, dtype=np.uint32)[None, :]).all()


def test_traced_block_loop_with_a_clean_input():
    far, near, clean, ref_out, ref_dig, ref_rec = th.clean_tracks()
    for chunk in (0, 24):
        streams = [simlib.SimStream(16000, *th.stream_config(s)) for s in range(th.CLEAN_STREAMS)]
        out, rec, _ = trace_sim.traced_launch(streams, far, near, clean=clean, chunk_blocks=chunk)
        assert th.first_record_difference(rec, ref_rec) is None, (chunk, th.first_record_difference(rec, ref_rec))
        assert np.array_equal(out, ref_out)
        assert all(np.array_equal(st.digest(), ref_dig[s, -1]) for s, st in enumerate(streams))


def test_record_layout():
    dt = ffi.BLOCK_TRACE_DTYPE
    assert aecm.block_trace_size_bytes() == 32 == dt.itemsize
    assert tuple((n, dt.fields[n][1]) for n in dt.names) == th.LAYOUT
    assert dt.fields["tot_count"][0] == np.dtype("<u4")
    assert all(dt.fields[n][0] == np.dtype("<i4") for n in ("delay_min_probability", "delay_last_probability"))
    assert all(dt.fields[n][0] == np.dtype("<i2") for n in dt.names[1:11])
    # the digest words the table of include/aecm_batch.h names, on a digest whose every half word is its own index
    d = (np.arange(24, dtype=np.uint32) * 2 + 1) << 16 | np.arange(24, dtype=np.uint32) * 2
    r = th.records_of_digests(d)
    assert (r["tot_count"], r["delay"], r["startup_state"], r["vad"], r["vad_update_count"]) == (d[0], 26, 4, 14, 15)
    assert (r["far_log_energy"], r["far_energy_min"], r["far_energy_max"], r["far_energy_vad"], r["sup_gain"], r["near_q"]) == (8, 9, 10, 12, 24, 6)
    assert (r["delay_min_probability"], r["delay_last_probability"]) == (d[14], d[15])


def test_describe_traced_launch_over_the_launch_table():
    """Never pipelined; DescribeLaunchDetail's answer wherever that is not form 3, the answer of a policy that never pipelines --
    one wavefront per stream -- where it is.  (The untraced descriptions themselves: tests/test_launch_table.py, unchanged.)"""
    n_pipelined = 0
    for cus in lt.CUS:
        never = aecm.default_launch_policy(cus)
        never.pipelined_min_streams = 0
        for S in lt.stream_counts(cus):
            for T in lt.BLOCKS:
                for clean in (False, True):
                    traced = aecm.describe_traced_launch(S, T, cus, clean)
                    plain = aecm.describe_launch_detail(S, T, cus, clean)
                    one_wave = aecm.describe_launch_detail(S, T, 0, clean, policy=never)
                    assert traced["form"] in (0, 1, 2), (cus, S, T, clean, traced)
                    assert traced == one_wave, (cus, S, T, clean)
                    if plain["form"] != 3:
                        assert traced == plain, (cus, S, T, clean)
                    else:
                        n_pipelined += 1
                        assert traced["form"] in (0, 1) and traced["waves_per_workgroup"] == 4 and traced["workgroups"] == -(-S // 4), (cus, S, T, traced)
        for wishes in lt.POLICIES:
            pol = lt._policy(aecm, cus, wishes)
            for S in (2, 4 * cus, 16 * cus, 16 * cus + 1, 28 * cus + 1):
                for T in (2, 3, 64, 300):
                    traced = aecm.describe_traced_launch(S, T, 0, False, policy=pol)
                    plain = aecm.describe_launch_detail(S, T, 0, False, policy=pol)
                    assert traced["form"] != 3 and (plain["form"] == 3 or traced == plain), (cus, wishes, S, T)
    assert n_pipelined > 100


def test_entry_points_that_need_no_device():
    lib = aecm.load()
    for name in ("WebRtcAecmBatch_block_trace_size_bytes", "WebRtcAecmBatch_SetBlockTrace", "WebRtcAecmBatch_DescribeTracedLaunch"):
        assert name in ffi.BATCH_SYMBOLS and hasattr(lib, name)
    buf = ctypes.create_string_buffer(64)
    assert lib.WebRtcAecmBatch_SetBlockTrace(None, ctypes.addressof(buf), 1, 1) == ffi.AECM_BAD_PARAMETER_ERROR
    assert lib.WebRtcAecmBatch_SetBlockTrace(None, None, 0, 0) == ffi.AECM_BAD_PARAMETER_ERROR
    d = ffi.AecmLaunchDescription()
    assert lib.WebRtcAecmBatch_DescribeTracedLaunch(None, 256, 8, 96, 0, None) == ffi.AECM_NULL_POINTER_ERROR
    assert lib.WebRtcAecmBatch_DescribeTracedLaunch(None, 0, 8, 96, 0, ctypes.byref(d)) == ffi.AECM_BAD_PARAMETER_ERROR
    assert lib.WebRtcAecmBatch_DescribeTracedLaunch(None, 256, 0, 96, 0, ctypes.byref(d)) == ffi.AECM_BAD_PARAMETER_ERROR
    assert lib.WebRtcAecmBatch_DescribeTracedLaunch(None, 256, 8, 96, 0, ctypes.byref(d)) == 0 and d.form == 0
    assert aecm.describe_launch_detail(8, 96, 256)["form"] == 3

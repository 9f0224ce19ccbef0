"""The block trace on the device (include/aecm_batch.h: WebRtcAecmBatch_SetBlockTrace; aecm_trace_kernels.hip): every record of
every traced launch form against the CPU checker's state after that block (tests/trace_helpers.py), with audio and digests
bit-exact against an untraced batch; ragged lengths, a clean input, both layouts, launch continuity, the launch-form rule, the
refusals, the decision corpus and the audit build.  The CPU side is tests/test_block_trace.py."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import trace_helpers as th
import webrtc_aecm_amd as aecm
from helpers import GOLDEN, describe_digest_diff, stream_config, synth_streams
from webrtc_aecm_amd import ffi

pytestmark = pytest.mark.gpu
REC = ffi.BLOCK_TRACE_DTYPE
FILL = 0xA5
SENTINEL = 0x5A5A


def _batch(rates, configs):
    """One batch whose stream s runs at rates[s] with configs[s]: a 16 kHz batch; the 8 kHz streams take the initial state of an
    8 kHz batch (ExportState / ImportState) before their configuration is set."""
    b = aecm.AecmBatch(len(rates), 16000)
    if 8000 in rates:
        donor = aecm.AecmBatch(1, 8000)
        init = donor.export_state(0)
        donor.close()
        for s, fs in enumerate(rates):
            if fs == 8000:
                b.import_state(s, init)
    for s, (cng, em) in enumerate(configs):
        b.set_config(cng, em, s, 1)
    return b


def _main_batch():
    return _batch(th.RATES, th.CONFIGS)


def _launch(b, far, near, clean=None, lens=None, records=None, strides=None, traced=True, want_form=None):
    """One device-pointer launch of all of far's blocks (ragged by lens).  traced: a trace buffer of `records` records (default:
    stream-major [S, T]) filled with 0xA5 is attached for the launch.  Returns (out -- 0x5A5A where nothing was written --, the
    trace as a flat BLOCK_TRACE_DTYPE array or None).  want_form: what describe_launch must say of this launch with the trace attached."""
    import torch
    dev = torch.device("cuda", 0)
    S, T = far.shape[0], far.shape[1] // 64
    tf, tn = torch.from_numpy(np.array(far, dtype=np.int16)).to(dev), torch.from_numpy(np.array(near, dtype=np.int16)).to(dev)      # (copies: the shared tracks are read-only)
    tc = torch.from_numpy(np.array(clean, dtype=np.int16)).to(dev) if clean is not None else None
    out = torch.full_like(tn, SENTINEL)
    trace = None
    if traced:
        records, strides = (S * T, (T, 1)) if records is None else (records, strides)
        assert (S - 1) * strides[0] + (T - 1) * strides[1] < records, "the launch's records do not fit the buffer"
        trace = torch.full((records * REC.itemsize,), FILL, dtype=torch.uint8, device=dev)
        b.set_block_trace(trace.data_ptr(), *strides)
        if want_form is not None:
            assert b.describe_launch(T, clean=clean is not None)[0] == want_form, (want_form, b.describe_launch(T, clean=clean is not None))
    torch.cuda.synchronize()
    cp = tc.data_ptr() if tc is not None else None
    if lens is None:
        b.process_device(tf.data_ptr(), tn.data_ptr(), out.data_ptr(), far.shape[1], 64, T, cp)
    else:
        b.process_ragged_device(tf.data_ptr(), tn.data_ptr(), out.data_ptr(), far.shape[1], 64, T, lens, cp)
    b.synchronize()
    if traced:
        b.clear_block_trace()
    return out.cpu().numpy(), (trace.cpu().numpy().view(REC) if traced else None)


def _digests(b):
    return np.stack([b.digest(s) for s in range(b.num_streams)])


def _assert_records(got, want, what):
    diff = th.first_record_difference(got, want)
    assert diff is None, f"{what}: first difference at (stream, block) {diff[0]}, field {diff[1]}: {diff[2]} != {diff[3]}"


def _untraced_main():
    far, near = th.main_inputs()
    b = _main_batch()
    out, _ = _launch(b, far, near, traced=False)
    dig = _digests(b)
    b.close()
    return out, dig


def _main_parity(chunk, want_form):
    far, near = th.main_inputs()
    ref_out, ref_dig, ref_rec = th.main_tracks()
    th.assert_tracks_are_alive(ref_rec)
    plain_out, plain_dig = _untraced_main()
    b = _main_batch()
    if chunk:
        b.set_launch_chunking(chunk, 1)
    import torch
    probe = torch.zeros(8, dtype=torch.int32, device="cuda")
    b.set_block_trace(probe.data_ptr(), 1, 1)
    assert b.describe_launch(th.N_BLOCKS) == want_form
    b.clear_block_trace()
    out, trace = _launch(b, far, near)
    _assert_records(trace.reshape(th.N_STREAMS, th.N_BLOCKS), ref_rec, f"traced launch, form {want_form}")
    assert np.array_equal(out, plain_out) and np.array_equal(out, ref_out)
    dig = _digests(b)
    for s in range(th.N_STREAMS):
        assert np.array_equal(dig[s], plain_dig[s]), (s, describe_digest_diff(dig[s], plain_dig[s]))
        assert np.array_equal(dig[s], ref_dig[s, -1]), (s, describe_digest_diff(dig[s], ref_dig[s, -1]))
    b.close()


def test_parity_one_wave_per_stream():
    """Six streams x 1 100 blocks (16 and 8 kHz alternating), stream-major trace, aecm_trace_process_kernel: records == the
    checker's track, audio and all 24 digest words == an untraced batch on the same inputs."""
    _main_parity(0, (0, 0))


def test_parity_chunk_queue():
    """The same through aecm_trace_queue_kernel in chunks of 48 blocks: 1 100 = 22 x 48 + 44, a partial last chunk and every
    hand-over of a stream's state between waves."""
    _main_parity(48, (2, 48))


@pytest.mark.parametrize("chunking", [None, (8, 1)], ids=["default chunking", "chunks of 8"])
def test_ragged(chunking):
    """Nine streams of lengths 0, 1, 7, 8, 9, 16, 40, 41, 3 in a launch of 41 blocks, the trace pre-filled with 0xA5 at a stream
    stride of 44 records: records 0 .. L - 1 are the first L blocks of each track, every other byte is still 0xA5."""
    lens = np.array([0, 1, 7, 8, 9, 16, 40, 41, 3], dtype=np.int32)
    S, T, stride = lens.size, 41, 44
    src = [s % th.N_STREAMS for s in range(S)]                     # streams 6..8: the inputs and configurations of streams 0..2 again
    far, near = th.main_inputs()
    _, _, ref_rec = th.main_tracks()
    b = _batch([th.RATES[k] for k in src], [th.CONFIGS[k] for k in src])
    if chunking:
        b.set_launch_chunking(*chunking)
    import torch
    probe = torch.zeros(8, dtype=torch.int32, device="cuda")
    b.set_block_trace(probe.data_ptr(), 1, 1)
    d = b.describe_ragged_launch(lens)
    b.clear_block_trace()
    assert d["form"] == (2 if chunking else 0) and (not chunking or d["chunk_blocks"] == 8), d
    out, trace = _launch(b, far[src, :T * 64], near[src, :T * 64], lens=lens, records=S * stride, strides=(stride, 1))
    raw = trace.view(np.uint8).reshape(S, stride, REC.itemsize)
    rec = trace.reshape(S, stride)
    for s, L in enumerate(lens):
        _assert_records(rec[s, :L], ref_rec[src[s], :L], f"ragged stream {s} of length {L}")
        assert (raw[s, L:] == FILL).all(), f"stream {s} of length {L}: bytes beyond its records were written"
        assert (out[s, L * 64:] == SENTINEL).all()
    b.close()


@pytest.mark.parametrize("chunk", [0, 24], ids=["one wave per stream", "chunk queue"])
def test_clean_input(chunk):
    """Four streams x 64 blocks with a clean near-end input: records == the checker's digests after each process_block_clean."""
    far, near, clean, ref_out, ref_dig, ref_rec = th.clean_tracks()
    b = _batch([16000] * th.CLEAN_STREAMS, [stream_config(s) for s in range(th.CLEAN_STREAMS)])
    if chunk:
        b.set_launch_chunking(chunk, 1)
    out, trace = _launch(b, far, near, clean=clean, want_form=2 if chunk else 0)
    _assert_records(trace.reshape(th.CLEAN_STREAMS, th.CLEAN_BLOCKS), ref_rec, f"clean input, chunk {chunk}")
    assert np.array_equal(out, ref_out)
    assert np.array_equal(_digests(b), ref_dig[:, -1])
    b.close()


def test_would_be_pipelined_size():
    """Eight streams x 96 blocks under the default policy: pipelined before a trace is attached, not while one is, again after
    clear_block_trace(); audio and digests of the three runs (fresh batches) are identical."""
    import torch
    S, T = 8, 96
    far, near = synth_streams(list(range(300, 300 + S)), T, 16000)
    cfgs = [stream_config(s) for s in range(S)]
    runs = []
    for mode in ("before", "attached", "after"):
        b = _batch([16000] * S, cfgs)
        assert b.describe_launch(T)[0] == 3
        if mode != "before":
            probe = torch.zeros(8, dtype=torch.int32, device="cuda")
            b.set_block_trace(probe.data_ptr(), 1, 1)
            assert b.describe_launch(T) == (0, 0)
            b.clear_block_trace()
            assert b.describe_launch(T)[0] == 3
        out, trace = _launch(b, far, near, traced=mode == "attached")
        assert b.describe_launch(T)[0] == 3
        runs.append((out, _digests(b)))
        if trace is not None:
            assert (trace["tot_count"].reshape(S, T) == np.arange(1, T + 1, dtype=np.uint32)).all()
        b.close()
    for out, dig in runs[1:]:
        assert np.array_equal(out, runs[0][0]) and np.array_equal(dig, runs[0][1])


def test_launch_continuity_and_layout():
    """30 + 34 blocks in two launches give the records of one 64-block launch (tot_count runs on, k restarts at 0); a tick-major
    layout (stream stride 1, block stride S) holds the same records as the stream-major one."""
    far, near = th.main_inputs()
    _, _, ref_rec = th.main_tracks()
    S = th.N_STREAMS
    b = _main_batch()
    _, a = _launch(b, far[:, :30 * 64], near[:, :30 * 64])
    _, c = _launch(b, far[:, 30 * 64:64 * 64], near[:, 30 * 64:64 * 64])
    two = np.concatenate([a.reshape(S, 30), c.reshape(S, 34)], axis=1)
    b.close()
    b = _main_batch()
    _, one = _launch(b, far[:, :64 * 64], near[:, :64 * 64])
    b.close()
    _assert_records(two, one.reshape(S, 64), "two launches against one")
    _assert_records(two, ref_rec[:, :64], "two launches against the checker")
    assert (two["tot_count"] == np.arange(1, 65, dtype=np.uint32)).all()
    for chunk in (0, 16):
        b = _main_batch()
        if chunk:
            b.set_launch_chunking(chunk, 1)
        _, tick_major = _launch(b, far[:, :64 * 64], near[:, :64 * 64], records=64 * S, strides=(1, S))
        b.close()
        _assert_records(tick_major.reshape(64, S).T, ref_rec[:, :64], f"tick-major layout, chunk {chunk}")


def test_refusals():
    """A misaligned pointer and a stride of 0 are refused with nothing changed; while a trace is attached the host-pointer forms
    and the ProcessRecordings family answer AECM_UNSUPPORTED_FUNCTION_ERROR with nothing run; digests are unchanged each time."""
    import torch
    S, T = 8, 16
    far, near = synth_streams(list(range(400, 400 + S)), T, 16000)
    b = _batch([16000] * S, [stream_config(s) for s in range(S)])
    b.process_host(far, near)                                     # some state to keep
    before = _digests(b)
    buf = torch.zeros(S * T * 8 + 8, dtype=torch.int32, device="cuda")

    def refused(code, fn):
        with pytest.raises(aecm.AecmError) as e:
            fn()
        assert e.value.code == code
        assert np.array_equal(_digests(b), before)

    refused(ffi.AECM_BAD_PARAMETER_ERROR, lambda: b.set_block_trace(buf.data_ptr() + 2, T, 1))
    refused(ffi.AECM_BAD_PARAMETER_ERROR, lambda: b.set_block_trace(buf.data_ptr(), 0, 1))
    refused(ffi.AECM_BAD_PARAMETER_ERROR, lambda: b.set_block_trace(buf.data_ptr(), T, 0))
    refused(ffi.AECM_BAD_PARAMETER_ERROR, lambda: b.set_block_trace(buf.data_ptr(), -1, 1))
    assert b.describe_launch(96)[0] == 3                          # nothing was attached
    b.set_block_trace(buf.data_ptr(), T, 1)
    assert b.describe_launch(96) == (0, 0)
    refused(ffi.AECM_BAD_PARAMETER_ERROR, lambda: b.set_block_trace(buf.data_ptr() + 1, T, 1))
    assert b.describe_launch(96) == (0, 0)                        # ... and the attached one stays
    refused(ffi.AECM_UNSUPPORTED_FUNCTION_ERROR, lambda: b.process_host(far, near))
    refused(ffi.AECM_UNSUPPORTED_FUNCTION_ERROR, lambda: b.process_ragged_host(far, near, np.full(S, T, np.int32)))
    out = np.full_like(near, SENTINEL)
    rc = b.lib.WebRtcAecmBatch_ProcessRecordingsHost(b.h, far.ctypes.data, near.ctypes.data, None, out.ctypes.data, far.shape[1], 80, far.shape[1] // 80, 40)
    assert rc == ffi.AECM_UNSUPPORTED_FUNCTION_ERROR and (out == SENTINEL).all()
    calls = np.full(S, far.shape[1] // 80, np.int32)
    codes = np.zeros(S, np.int32)
    rc = b.lib.WebRtcAecmBatch_ProcessRecordingsRaggedHost(b.h, far.ctypes.data, near.ctypes.data, None, out.ctypes.data, far.shape[1], 80, far.shape[1] // 80,
                                                           calls.ctypes.data, 40, codes.ctypes.data)
    assert rc == ffi.AECM_UNSUPPORTED_FUNCTION_ERROR and (out == SENTINEL).all()
    tf, tn = torch.from_numpy(far).cuda(), torch.from_numpy(near).cuda()
    to = torch.full_like(tn, SENTINEL)
    assert b.process_recordings_device(tf.data_ptr(), tn.data_ptr(), to.data_ptr(), far.shape[1], 80, far.shape[1] // 80) == ffi.AECM_UNSUPPORTED_FUNCTION_ERROR
    rc = b.lib.WebRtcAecmBatch_ProcessRecordingsRagged(b.h, tf.data_ptr(), tn.data_ptr(), None, to.data_ptr(), far.shape[1], 80, far.shape[1] // 80,
                                                       calls.ctypes.data, 40, codes.ctypes.data)
    b.synchronize()
    assert rc == ffi.AECM_UNSUPPORTED_FUNCTION_ERROR and (to.cpu().numpy() == SENTINEL).all()
    assert np.array_equal(_digests(b), before) and (buf.cpu().numpy() == 0).all()
    b.clear_block_trace()
    b.process_host(far, near)                                     # and the host form runs again
    assert not np.array_equal(_digests(b), before)
    b.close()


@pytest.mark.parametrize("fs,clean", [(16000, False), (16000, True), (8000, False), (8000, True)], ids=["16000", "16000-clean", "8000", "8000-clean"])
@pytest.mark.parametrize("chunk", [0, 32], ids=["one wave per stream", "chunk queue"])
def test_decision_corpus(chunk, fs, clean):
    """The cases of tests/block_corpus.py through the traced one-wave and queue kernels: audio and digests equal the corpus'
    expected values (as tests/test_gpu_block_corpus.py checks for the other families), and the last record of each case is its
    final digest's words."""
    import test_gpu_block_corpus as BC
    exp = BC._expected()
    for n, cases, far, near, cl in BC._groups(fs, clean):
        b = BC._batch(cases, fs)
        if chunk:
            b.set_launch_chunking(chunk, 0)
        else:
            b.set_launch_pipelining(0)
        out, trace = _launch(b, far, near, clean=cl, want_form=2 if chunk else 0)
        BC._check_out(cases, out, 0, exp, f"traced, chunk {chunk}, {n} blocks")
        BC._check_digests(cases, b, exp, 2, f"traced, chunk {chunk}, {n} blocks")
        last = trace.reshape(len(cases), n)[:, -1]
        want = th.records_of_digests(np.stack([exp[c["name"]][2] for c in cases]))
        _assert_records(last[:, None], want[:, None], f"last record, chunk {chunk}, {n} blocks")
        b.close()


def test_checked_build_counts_nothing(tmp_path):
    """One traced chunk-queue launch of the main inputs (chunks of 48) and one traced one-wave launch on the audit build
    (-DAECM_CHECKED), in a child process: the check counters stay zero, the records are the checker's."""
    from webrtc_aecm_amd import build
    assert build.LIB_CHECKED.exists()
    script = tmp_path / "audit_trace.py"
    script.write_text(textwrap.dedent("""
        import numpy as np
        import webrtc_aecm_amd as aecm
        import test_gpu_block_trace as T
        import trace_helpers as th
        assert aecm.check_counters(0, reset=True) is not None
        far, near = th.main_inputs()
        _, _, ref_rec = th.main_tracks()
        for chunk in (48, 0):
            b = T._main_batch()
            if chunk:
                b.set_launch_chunking(chunk, 1)
            out, trace = T._launch(b, far, near)
            T._assert_records(trace.reshape(th.N_STREAMS, th.N_BLOCKS), ref_rec, "checked build")
            b.close()
        c = aecm.check_counters(0)
        print("AUDIT", int(c[0]), int(c[1]))
    """))
    env = dict(os.environ, AECM_LIB_PATH=str(build.LIB_CHECKED),
               PYTHONPATH=os.pathsep.join([str(GOLDEN.parent.parent), str(GOLDEN.parent), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("AUDIT")]
    assert line and line[-1].split()[1:] == ["0", "0"], r.stdout[-500:]

"""ctypes bindings of libaecm_mi355x.so.

`Aecm` mirrors the reference's session interface (aecm/echo_control_mobile.h: Create / Init /
BufferFarend / Process / set_config / InitEchoPath / GetEchoPath / Free, same argument meaning and
return codes); `AecmBatch` is the batch extension (include/aecm_batch.h).  There is no Python or CPU
implementation of the DSP here: without the HIP library and a GPU these classes raise.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import build as _build

BLOCK = 64
BINS = 65
DIGEST_WORDS = 24
KERNEL_SAFE, KERNEL_FAST = 0, 1

AECM_UNSPECIFIED_ERROR = 12000
AECM_UNSUPPORTED_FUNCTION_ERROR = 12001
AECM_UNINITIALIZED_ERROR = 12002
AECM_NULL_POINTER_ERROR = 12003
AECM_BAD_PARAMETER_ERROR = 12004
AECM_BAD_PARAMETER_WARNING = 12100

SESSION_SYMBOLS = [
    "WebRtcAecm_Create", "WebRtcAecm_Free", "WebRtcAecm_Init", "WebRtcAecm_BufferFarend",
    "WebRtcAecm_GetBufferFarendError", "WebRtcAecm_Process", "WebRtcAecm_set_config",
    "WebRtcAecm_InitEchoPath", "WebRtcAecm_GetEchoPath", "WebRtcAecm_echo_path_size_bytes",
]
BATCH_SYMBOLS = [
    "WebRtcAecmBatch_Create", "WebRtcAecmBatch_Free", "WebRtcAecmBatch_num_streams", "WebRtcAecmBatch_Init",
    "WebRtcAecmBatch_set_config", "WebRtcAecmBatch_Control", "WebRtcAecmBatch_ProcessBlocks",
    "WebRtcAecmBatch_ProcessBlocksHost", "WebRtcAecmBatch_ProcessRecordings", "WebRtcAecmBatch_ProcessRecordingsHost",
    "WebRtcAecmBatch_Synchronize", "WebRtcAecmBatch_GetLastLaunchMs",
    "WebRtcAecmBatch_GetTimers", "WebRtcAecmBatch_ResetTimers", "WebRtcAecmBatch_InitEchoPath",
    "WebRtcAecmBatch_GetEchoPath", "WebRtcAecmBatch_state_size_bytes", "WebRtcAecmBatch_ExportState",
    "WebRtcAecmBatch_ImportState", "WebRtcAecmBatch_ExportStates", "WebRtcAecmBatch_ImportStates", "WebRtcAecmBatch_ExportStatesDevice",
    "WebRtcAecmBatch_ImportStatesDevice", "WebRtcAecmBatch_GetDigest", "WebRtcAecmBatch_SetKernelVariant", "WebRtcAecmBatch_SetLaunchChunking", "WebRtcAecmBatch_SetLaunchPipelining", "WebRtcAecmBatch_DescribeLaunch", "WebRtcAecmBatch_DescribeLaunchFor",
    "WebRtcAecmBatch_SelfTest", "WebRtcAecmBatch_DebugFft128", "WebRtcAecmBatch_DeviceInfo", "WebRtcAecmBatch_GetCheckCounters",
    "WebRtcAecmBatch_RegisterHostBuffer", "WebRtcAecmBatch_UnregisterHostBuffer",
    "WebRtcAecmBatch_DefaultLaunchPolicy", "WebRtcAecmBatch_GetLaunchPolicy", "WebRtcAecmBatch_SetLaunchPolicy", "WebRtcAecmBatch_DescribeLaunchDetail",
    "WebRtcAecm_SetDefaultDevice", "WebRtcAecmBatch_DevicePciBusId",
    "WebRtcAecmBatch_ProcessBlocksRagged", "WebRtcAecmBatch_ProcessBlocksRaggedHost", "WebRtcAecmBatch_ProcessRecordingsRagged",
    "WebRtcAecmBatch_ProcessRecordingsRaggedHost", "WebRtcAecmBatch_DescribeRaggedLaunch", "WebRtcAecmBatch_RaggedPlan",
    "WebRtcAecmBatch_SetRaggedPipelining", "WebRtcAecmBatch_DescribeRaggedLaunchEx", "WebRtcAecmBatch_RaggedPipePlan",
    "WebRtcAecmBatch_DescribeRaggedLaunchOf",
    "WebRtcAecmBatch_SetCleanPipelining", "WebRtcAecmBatch_DescribeLaunchDetailEx",
    "WebRtcAecmBatch_SetRaggedCleanPipelining", "WebRtcAecmBatch_DescribeRaggedLaunchEx2",
    "WebRtcAecmBatch_block_trace_size_bytes", "WebRtcAecmBatch_SetBlockTrace", "WebRtcAecmBatch_DescribeTracedLaunch",
    "WebRtcAecmBatch_DebugOps", "WebRtcAecmBatch_DebugOpsCount", "WebRtcAecmBatch_DebugOpName",
]
# include/aecm_batch.h: AecmBlockTrace -- the 32-byte record a block writes while a trace is attached (AecmBatch.set_block_trace)
BLOCK_TRACE_DTYPE = np.dtype([
    ("tot_count", "<u4"), ("delay", "<i2"), ("startup_state", "<i2"), ("vad", "<i2"), ("vad_update_count", "<i2"),
    ("far_log_energy", "<i2"), ("far_energy_min", "<i2"), ("far_energy_max", "<i2"), ("far_energy_vad", "<i2"),
    ("sup_gain", "<i2"), ("near_q", "<i2"), ("delay_min_probability", "<i4"), ("delay_last_probability", "<i4")])
SESSIONS_SYMBOLS = [
    "WebRtcAecmSessions_Create", "WebRtcAecmSessions_Free", "WebRtcAecmSessions_Init", "WebRtcAecmSessions_set_config",
    "WebRtcAecmSessions_Tick", "WebRtcAecmSessions_TickHost", "WebRtcAecmSessions_TickPerSession",
    "WebRtcAecmSessions_TickPerSessionHost", "WebRtcAecmSessions_TickFlags", "WebRtcAecmSessions_TickFlagsHost",
    "WebRtcAecmSessions_InitSession", "WebRtcAecmSessions_set_config_session", "WebRtcAecmSessions_InitEchoPath",
    "WebRtcAecmSessions_GetEchoPath", "WebRtcAecmSessions_TickAsync", "WebRtcAecmSessions_Synchronize",
    "WebRtcAecmSessions_SetKernelVariant", "WebRtcAecmSessions_session_size_bytes", "WebRtcAecmSessions_ExportSession",
    "WebRtcAecmSessions_ImportSession", "WebRtcAecmSessions_BufferFarend", "WebRtcAecmSessions_BufferFarendHost",
    "WebRtcAecmSessions_BufferFarendAsync", "WebRtcAecmSessions_Process", "WebRtcAecmSessions_ProcessHost", "WebRtcAecmSessions_DescribeTick",
    "WebRtcAecmSessions_DescribeTickLive", "WebRtcAecmSessions_ForceSparseTicks",
    "WebRtcAecmSessions_InitRates", "WebRtcAecmSessions_InitSessionRate", "WebRtcAecmSessions_GetSessionRate",
    "WebRtcAecmSessions_ImportSessionAnyRate",
    "WebRtcAecmSessions_ExportSessions", "WebRtcAecmSessions_ImportSessions", "WebRtcAecmSessions_ExportSessionsDevice",
    "WebRtcAecmSessions_ImportSessionsDevice",
    "WebRtcAecmSessions_TickCalls", "WebRtcAecmSessions_TickCallsHost", "WebRtcAecmSessions_TickCallsAsync",
    "WebRtcAecmSessions_TickPackets", "WebRtcAecmSessions_TickPacketsHost", "WebRtcAecmSessions_TickPacketsAsync",
    "WebRtcAecmSessions_GetSessionCleanMode", "WebRtcAecmSessions_SplitCleanTwoLaunches",
    "WebRtcAecmSessions_session_trace_size_bytes", "WebRtcAecmSessions_SetSessionTrace", "WebRtcAecmSessions_GetSessionTraceTicks",
    "WebRtcAecmSessions_SetCallTrace", "WebRtcAecmSessions_GetCallTraceCalls",
    "WebRtcAecmSessions_SetSplitCallTicks",
]
# include/aecm_batch.h: AecmSessionTrace -- the 64-byte record a session writes per tick while a trace is attached
# (AecmSessions.set_session_trace); `core` is the block trace's record of the core state after the tick's last block
SESSION_TRACE_DTYPE = np.dtype([
    ("tick", "<u4"), ("blocks", "<i2"), ("samp_khz", "<i2"), ("ms_in_snd_card_buf", "<i2"), ("known_delay", "<i2"),
    ("filt_delay", "<i2"), ("buf_size_start", "<i2"), ("ec_startup", "<i2"), ("check_buff_size", "<i2"), ("delay_change", "<i2"),
    ("last_delay_diff", "<i2"), ("far_buffered", "<i4"), ("time_for_delay_change", "<i4"), ("core", BLOCK_TRACE_DTYPE)])
SESSION_NO_FAREND = 1
SESSION_SPLIT_CALLS = 2
SESSION_IDLE = 4
SESSION_HALF_CALL = 8
SESSION_NO_CLEAN = 16
SESSION_MAX_TICK_CALLS = 6


class AecmConfig(C.Structure):
    _fields_ = [("cngMode", C.c_int16), ("echoMode", C.c_int16)]


_lib = None


class AecmLaunchPolicy(C.Structure):
    """include/aecm_batch.h: AecmLaunchPolicy (every threshold and wish that decides how a ProcessBlocks launch is scheduled)."""
    _fields_ = [(n, C.c_int32) for n in (
        "struct_size", "compute_units", "queue_chunk_blocks", "queue_chunk_explicit", "queue_min_streams", "pipelined_min_streams",
        "pipelined_min_blocks", "pipelined_max_streams", "resident_waves", "rotation_stream_limit", "pipe_tail_waves", "pipe_front_waves",
        "pipe_raw", "pipe_delay_waves", "pipe_gain_waves", "pipe_spread", "pipe_wgs_per_cu", "pipe_rot", "pipe_prio")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class AecmLaunchDescription(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("form", "chunk_blocks", "shape", "workgroups", "waves_per_workgroup", "workgroups_per_cu", "rounds_x1000", "cu_load_evenness_x1000")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def library_path() -> Path:
    """The library load() binds: $AECM_LIB_PATH (kernel A/B experiments) or the in-tree build."""
    return Path(os.environ["AECM_LIB_PATH"]) if os.environ.get("AECM_LIB_PATH") else _build.LIB


def load():
    """Load the HIP library (building it first if the sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own libamdhip64; two HIP runtimes in one process do not both see the
    # GPU.  Importing torch first makes this library bind to the runtime torch already loaded, so
    # torch tensors (device memory, streams) and this engine share one runtime.  Without torch
    # installed the system ROCm runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    # AECM_LIB_PATH: load a specific prebuilt library (kernel A/B experiments) instead of (re)building.
    path = os.environ.get("AECM_LIB_PATH") or _build.build()
    lib = C.CDLL(str(path))
    vp, i16p = C.c_void_p, C.c_void_p
    lib.WebRtcAecm_Create.restype = vp
    lib.WebRtcAecm_Free.argtypes = [vp]
    lib.WebRtcAecm_Free.restype = None
    lib.WebRtcAecm_Init.argtypes = [vp, C.c_int32]
    lib.WebRtcAecm_BufferFarend.argtypes = [vp, i16p, C.c_size_t]
    lib.WebRtcAecm_GetBufferFarendError.argtypes = [vp, i16p, C.c_size_t]
    lib.WebRtcAecm_Process.argtypes = [vp, i16p, i16p, i16p, C.c_size_t, C.c_int16]
    lib.WebRtcAecm_set_config.argtypes = [vp, AecmConfig]
    lib.WebRtcAecm_InitEchoPath.argtypes = [vp, vp, C.c_size_t]
    lib.WebRtcAecm_GetEchoPath.argtypes = [vp, vp, C.c_size_t]
    lib.WebRtcAecm_echo_path_size_bytes.restype = C.c_size_t
    lib.WebRtcAecmBatch_Create.restype = vp
    lib.WebRtcAecmBatch_Create.argtypes = [C.c_int32, C.c_int32]
    lib.WebRtcAecmBatch_Free.argtypes = [vp]
    lib.WebRtcAecmBatch_Free.restype = None
    lib.WebRtcAecmBatch_num_streams.argtypes = [vp]
    lib.WebRtcAecmBatch_Init.argtypes = [vp, C.c_int32]
    lib.WebRtcAecmBatch_set_config.argtypes = [vp, AecmConfig, C.c_int32, C.c_int32]
    lib.WebRtcAecmBatch_Control.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.WebRtcAecmBatch_ProcessBlocks.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int64, C.c_int32]
    lib.WebRtcAecmBatch_ProcessBlocksHost.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int64, C.c_int32]
    lib.WebRtcAecmBatch_ProcessRecordings.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_int16]
    lib.WebRtcAecmBatch_ProcessRecordingsHost.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_int16]
    lib.WebRtcAecmBatch_ProcessBlocksRagged.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int64, C.c_int32, vp]
    lib.WebRtcAecmBatch_ProcessBlocksRaggedHost.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int64, C.c_int32, vp]
    lib.WebRtcAecmBatch_ProcessRecordingsRagged.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, vp, C.c_int16, vp]
    lib.WebRtcAecmBatch_ProcessRecordingsRaggedHost.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, vp, C.c_int16, vp]
    lib.WebRtcAecmBatch_DescribeRaggedLaunch.argtypes = [C.POINTER(AecmLaunchPolicy), C.c_int32, C.c_int32, vp, C.c_int32,
                                                         C.POINTER(AecmLaunchDescription), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                                         C.POINTER(C.c_int32)]
    lib.WebRtcAecmBatch_RaggedPlan.argtypes = [C.c_int32, vp, C.c_int32, vp, vp, C.c_int32, C.POINTER(C.c_int32)]
    # (a library built from an older tree -- tools/bench_ragged.py --parent -- lacks these: calling one on it raises AttributeError)
    if hasattr(lib, "WebRtcAecmBatch_SetRaggedPipelining"):
        lib.WebRtcAecmBatch_DescribeRaggedLaunchOf.argtypes = [vp, vp, C.c_int32, C.POINTER(AecmLaunchDescription), C.POINTER(C.c_int64),
                                                               C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        lib.WebRtcAecmBatch_SetRaggedPipelining.argtypes = [vp, C.c_int32]
        lib.WebRtcAecmBatch_DescribeRaggedLaunchEx.argtypes = [C.POINTER(AecmLaunchPolicy), C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32,
                                                               C.POINTER(AecmLaunchDescription), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                                               C.POINTER(C.c_int32)]
        lib.WebRtcAecmBatch_RaggedPipePlan.argtypes = [C.POINTER(AecmLaunchPolicy), C.c_int32, C.c_int32, vp, vp, C.c_int32, C.POINTER(C.c_int32)]
    if hasattr(lib, "WebRtcAecmBatch_SetCleanPipelining"):      # (as above: absent from a library built from an older tree)
        lib.WebRtcAecmBatch_SetCleanPipelining.argtypes = [vp, C.c_int32]
        lib.WebRtcAecmBatch_DescribeLaunchDetailEx.argtypes = [C.POINTER(AecmLaunchPolicy), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                               C.POINTER(AecmLaunchDescription)]
    if hasattr(lib, "WebRtcAecmBatch_SetRaggedCleanPipelining"):      # (as above)
        lib.WebRtcAecmBatch_SetRaggedCleanPipelining.argtypes = [vp, C.c_int32]
        lib.WebRtcAecmBatch_DescribeRaggedLaunchEx2.argtypes = [C.POINTER(AecmLaunchPolicy), C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32,
                                                                C.POINTER(AecmLaunchDescription), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                                                C.POINTER(C.c_int32)]
    if hasattr(lib, "WebRtcAecmBatch_SetBlockTrace"):      # (as above)
        lib.WebRtcAecmBatch_block_trace_size_bytes.restype = C.c_size_t
        lib.WebRtcAecmBatch_block_trace_size_bytes.argtypes = []
        lib.WebRtcAecmBatch_SetBlockTrace.argtypes = [vp, vp, C.c_int64, C.c_int64]
        lib.WebRtcAecmBatch_DescribeTracedLaunch.argtypes = [C.POINTER(AecmLaunchPolicy), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                             C.POINTER(AecmLaunchDescription)]
    lib.WebRtcAecmBatch_Synchronize.argtypes = [vp]
    lib.WebRtcAecmBatch_GetLastLaunchMs.argtypes = [vp, C.POINTER(C.c_float)]
    lib.WebRtcAecmBatch_GetTimers.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.WebRtcAecmBatch_ResetTimers.argtypes = [vp]
    lib.WebRtcAecmBatch_InitEchoPath.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    lib.WebRtcAecmBatch_GetEchoPath.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    lib.WebRtcAecmBatch_state_size_bytes.restype = C.c_size_t
    lib.WebRtcAecmBatch_ExportState.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    lib.WebRtcAecmBatch_ImportState.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    lib.WebRtcAecmBatch_GetDigest.argtypes = [vp, C.c_int32, vp]
    for name in ("ExportStates", "ImportStates", "ExportStatesDevice", "ImportStatesDevice"):
        getattr(lib, "WebRtcAecmBatch_" + name).argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_size_t]
    lib.WebRtcAecmSessions_session_size_bytes.restype = C.c_size_t
    lib.WebRtcAecmSessions_ExportSession.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    lib.WebRtcAecmSessions_ImportSession.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    lib.WebRtcAecmBatch_SetKernelVariant.argtypes = [vp, C.c_int32]
    lib.WebRtcAecmBatch_SetLaunchChunking.argtypes = [vp, C.c_int32, C.c_int32]
    lib.WebRtcAecmBatch_DescribeLaunch.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    lib.WebRtcAecmBatch_SetLaunchPipelining.argtypes = [vp, C.c_int32]
    lib.WebRtcAecmBatch_DescribeLaunchFor.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    lib.WebRtcAecmBatch_DefaultLaunchPolicy.argtypes = [C.c_int32, C.POINTER(AecmLaunchPolicy)]
    lib.WebRtcAecmBatch_GetLaunchPolicy.argtypes = [vp, C.POINTER(AecmLaunchPolicy)]
    lib.WebRtcAecmBatch_SetLaunchPolicy.argtypes = [vp, C.POINTER(AecmLaunchPolicy)]
    lib.WebRtcAecmBatch_DescribeLaunchDetail.argtypes = [C.POINTER(AecmLaunchPolicy), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                         C.POINTER(AecmLaunchDescription)]
    lib.WebRtcAecmSessions_DescribeTick.argtypes = [C.c_int32, C.c_int32, C.POINTER(AecmLaunchDescription)]
    lib.WebRtcAecmSessions_DescribeTickLive.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(AecmLaunchDescription)]
    lib.WebRtcAecmSessions_ForceSparseTicks.argtypes = [vp, C.c_int32]
    lib.WebRtcAecmSessions_GetSessionCleanMode.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32)]
    lib.WebRtcAecmSessions_SplitCleanTwoLaunches.argtypes = [vp, C.c_int32]
    if hasattr(lib, "WebRtcAecmSessions_SetSplitCallTicks"):    # (a library of an older tree, loaded for an A/B run, has none)
        lib.WebRtcAecmSessions_SetSplitCallTicks.argtypes = [vp, C.c_int32]
    if hasattr(lib, "WebRtcAecmSessions_SetSessionTrace"):      # (a library of an older tree, loaded for an A/B run, has none)
        lib.WebRtcAecmSessions_session_trace_size_bytes.restype = C.c_size_t
        lib.WebRtcAecmSessions_session_trace_size_bytes.argtypes = []
        lib.WebRtcAecmSessions_SetSessionTrace.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int32]
        lib.WebRtcAecmSessions_GetSessionTraceTicks.argtypes = [vp, C.POINTER(C.c_int64)]
    if hasattr(lib, "WebRtcAecmSessions_SetCallTrace"):         # (likewise)
        lib.WebRtcAecmSessions_SetCallTrace.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int32]
        lib.WebRtcAecmSessions_GetCallTraceCalls.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.WebRtcAecmSessions_InitRates.argtypes = [vp, C.c_int32, vp]
    lib.WebRtcAecmSessions_InitSessionRate.argtypes = [vp, C.c_int32, C.c_int32]
    lib.WebRtcAecmSessions_GetSessionRate.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32)]
    lib.WebRtcAecmSessions_ImportSessionAnyRate.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    lib.WebRtcAecmSessions_ExportSessions.argtypes = [vp, vp, C.c_int32, vp, C.c_size_t]
    lib.WebRtcAecmSessions_ExportSessionsDevice.argtypes = [vp, vp, C.c_int32, vp, C.c_size_t]
    lib.WebRtcAecmSessions_ImportSessions.argtypes = [vp, vp, C.c_int32, vp, C.c_size_t, C.c_int32]
    lib.WebRtcAecmSessions_ImportSessionsDevice.argtypes = [vp, vp, C.c_int32, vp, C.c_size_t, C.c_int32]
    lib.WebRtcAecm_SetDefaultDevice.argtypes = [C.c_int32]
    lib.WebRtcAecmSessions_Create.restype = vp
    lib.WebRtcAecmSessions_Create.argtypes = [C.c_int32, C.c_int32]
    lib.WebRtcAecmSessions_Free.argtypes = [vp]
    lib.WebRtcAecmSessions_Free.restype = None
    lib.WebRtcAecmSessions_Init.argtypes = [vp, C.c_int32]
    lib.WebRtcAecmSessions_set_config.argtypes = [vp, AecmConfig]
    lib.WebRtcAecmSessions_Tick.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, C.c_int16]
    lib.WebRtcAecmSessions_TickHost.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, C.c_int16]
    lib.WebRtcAecmSessions_TickPerSession.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, vp, vp]
    lib.WebRtcAecmSessions_TickPerSessionHost.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, vp, vp]
    lib.WebRtcAecmSessions_TickFlags.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, vp, vp, vp]
    lib.WebRtcAecmSessions_TickFlagsHost.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, vp, vp, vp]
    lib.WebRtcAecmSessions_InitSession.argtypes = [vp, C.c_int32]
    lib.WebRtcAecmSessions_set_config_session.argtypes = [vp, C.c_int32, AecmConfig]
    lib.WebRtcAecmSessions_InitEchoPath.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    lib.WebRtcAecmSessions_GetEchoPath.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    lib.WebRtcAecmSessions_TickAsync.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, C.c_int16, vp, vp, vp, vp, vp]
    lib.WebRtcAecmSessions_TickCalls.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, C.c_int32, C.c_int16, vp, vp, vp]
    lib.WebRtcAecmSessions_TickCallsHost.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, C.c_int32, C.c_int16, vp, vp, vp]
    lib.WebRtcAecmSessions_TickCallsAsync.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, C.c_int32, C.c_int16, vp, vp, vp, vp, vp]
    lib.WebRtcAecmSessions_TickPackets.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, C.c_int32, C.c_int16, vp, vp, vp]
    lib.WebRtcAecmSessions_TickPacketsHost.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, C.c_int32, C.c_int16, vp, vp, vp]
    lib.WebRtcAecmSessions_TickPacketsAsync.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_size_t, C.c_int32, C.c_int16, vp, vp, vp, vp, vp]
    lib.WebRtcAecmSessions_BufferFarend.argtypes = [vp, vp, C.c_int64, C.c_size_t, C.c_int32, vp]
    lib.WebRtcAecmSessions_BufferFarendHost.argtypes = [vp, vp, C.c_int64, C.c_size_t, C.c_int32, vp]
    lib.WebRtcAecmSessions_BufferFarendAsync.argtypes = [vp, vp, C.c_int64, C.c_size_t, C.c_int32, vp, vp, vp]
    lib.WebRtcAecmSessions_Process.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_size_t, C.c_int16, vp, vp]
    lib.WebRtcAecmSessions_ProcessHost.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_size_t, C.c_int16, vp, vp]
    lib.WebRtcAecmSessions_Synchronize.argtypes = [vp]
    lib.WebRtcAecmSessions_SetKernelVariant.argtypes = [vp, C.c_int32]
    lib.WebRtcAecmBatch_RegisterHostBuffer.argtypes = [C.c_int32, vp, C.c_size_t, C.POINTER(C.c_void_p)]
    lib.WebRtcAecmBatch_UnregisterHostBuffer.argtypes = [C.c_int32, vp]
    lib.WebRtcAecmBatch_GetCheckCounters.argtypes = [C.c_int32, vp, C.c_int32]
    lib.WebRtcAecmBatch_SelfTest.argtypes = [C.c_int32, C.c_int32, vp]
    lib.WebRtcAecmBatch_DebugFft128.argtypes = [C.c_int32, vp, vp, C.c_int32, C.c_int32, C.c_int32]
    lib.WebRtcAecmBatch_DebugOps.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, C.c_int32]
    lib.WebRtcAecmBatch_DebugOpsCount.argtypes = []
    lib.WebRtcAecmBatch_DebugOpName.argtypes = [C.c_int32]
    lib.WebRtcAecmBatch_DebugOpName.restype = C.c_char_p
    lib.WebRtcAecmBatch_DeviceInfo.argtypes = [C.c_int32, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.WebRtcAecmBatch_DevicePciBusId.argtypes = [C.c_int32, C.c_char_p, C.c_size_t]
    _lib = lib
    return lib


def _i16(a):
    a = np.ascontiguousarray(a, dtype=np.int16)
    return a, a.ctypes.data


class AecmError(RuntimeError):
    def __init__(self, code, where):
        super().__init__(f"{where} returned {code}")
        self.code = code


class Aecm:
    """One AECM session: the reference's WebRtcAecm_* interface, DSP on the GPU."""

    def __init__(self):
        self.lib = load()
        self.h = self.lib.WebRtcAecm_Create()
        if not self.h:
            raise RuntimeError("WebRtcAecm_Create failed: the HIP engine needs a usable MI355X (no CPU fallback exists)")

    def init(self, samp_freq: int) -> int:
        return self.lib.WebRtcAecm_Init(self.h, samp_freq)

    def set_config(self, cng_mode: int, echo_mode: int) -> int:
        return self.lib.WebRtcAecm_set_config(self.h, AecmConfig(cng_mode, echo_mode))

    def buffer_farend(self, farend) -> int:
        a, p = _i16(farend)
        return self.lib.WebRtcAecm_BufferFarend(self.h, p, a.size)

    def process(self, nearend_noisy, nearend_clean=None, ms_in_snd_card_buf: int = 0):
        """Returns (code, out)."""
        a, p = _i16(nearend_noisy)
        cp = None
        if nearend_clean is not None:
            c, cp = _i16(nearend_clean)
        out = np.empty_like(a)
        rc = self.lib.WebRtcAecm_Process(self.h, p, cp, out.ctypes.data, a.size, ms_in_snd_card_buf)
        return rc, out

    def init_echo_path(self, path) -> int:
        a, p = _i16(path)
        return self.lib.WebRtcAecm_InitEchoPath(self.h, p, a.nbytes)

    def get_echo_path(self):
        out = np.zeros(BINS, dtype=np.int16)
        rc = self.lib.WebRtcAecm_GetEchoPath(self.h, out.ctypes.data, out.nbytes)
        return rc, out

    def run(self, far, near, frame: int, ms: int = 40):
        """The reference CLI's loop (main.cc:105-143): BufferFarend + Process per `frame` samples."""
        far = np.ascontiguousarray(far, dtype=np.int16)
        near = np.ascontiguousarray(near, dtype=np.int16).copy()
        for i in range(near.size // frame):
            sl = slice(i * frame, (i + 1) * frame)
            rc = self.buffer_farend(far[sl])
            if rc != 0:
                raise AecmError(rc, "WebRtcAecm_BufferFarend")
            rc, out = self.process(near[sl], None, ms)
            if rc != 0:
                raise AecmError(rc, "WebRtcAecm_Process")
            near[sl] = out
        return near

    def close(self):
        if getattr(self, "h", None):
            self.lib.WebRtcAecm_Free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AecmBatch:
    """S independent AECM block streams on one GPU (include/aecm_batch.h)."""

    def __init__(self, num_streams: int, fs: int = 16000, cng_mode: int = 1, echo_mode: int = 3, device: int = 0,
                 variant: int = KERNEL_FAST):
        self.lib = load()
        self.num_streams = num_streams
        self.h = self.lib.WebRtcAecmBatch_Create(num_streams, device)
        if not self.h:
            raise RuntimeError("WebRtcAecmBatch_Create failed: the HIP engine needs a usable MI355X (no CPU fallback exists)")
        self._check(self.lib.WebRtcAecmBatch_Init(self.h, fs), "Init")
        self._check(self.lib.WebRtcAecmBatch_set_config(self.h, AecmConfig(cng_mode, echo_mode), 0, -1), "set_config")
        self._check(self.lib.WebRtcAecmBatch_SetKernelVariant(self.h, variant), "SetKernelVariant")

    @staticmethod
    def _check(rc, where):
        if rc != 0:
            raise AecmError(rc, "WebRtcAecmBatch_" + where)

    def set_launch_chunking(self, chunk_blocks, min_streams=-1):
        """Scheduling of large launches (results never depend on it): chunks of chunk_blocks blocks claimed from a queue
        by resident wavefronts; 0 = one wavefront per stream for the whole launch."""
        self._check(self.lib.WebRtcAecmBatch_SetLaunchChunking(self.h, chunk_blocks, min_streams), "SetLaunchChunking")

    def set_launch_pipelining(self, min_streams):
        """Smallest batch whose launches run pipelined (six to sixteen wavefronts per four streams; results never depend on it);
        <= 0: never.  By default launches of one or two blocks keep one wavefront per stream; after this call launches of
        any length do what min_streams says."""
        self._check(self.lib.WebRtcAecmBatch_SetLaunchPipelining(self.h, min_streams), "SetLaunchPipelining")

    def set_ragged_pipelining(self, enable):
        """Ragged launches the chip holds at once take the pipelined form (include/aecm_batch.h: WebRtcAecmBatch_SetRaggedPipelining;
        results never depend on it).  Off by default."""
        self._check(self.lib.WebRtcAecmBatch_SetRaggedPipelining(self.h, 1 if enable else 0), "SetRaggedPipelining")

    def set_clean_pipelining(self, enable=True):
        """Equal-length launches with a clean near-end input that the chip holds at once take the pipelined form
        (include/aecm_batch.h: WebRtcAecmBatch_SetCleanPipelining; results never depend on it).  Off by default."""
        self._check(self.lib.WebRtcAecmBatch_SetCleanPipelining(self.h, 1 if enable else 0), "SetCleanPipelining")

    def set_ragged_clean_pipelining(self, enable=True):
        """Ragged launches with a clean near-end input that the chip holds at once take the pipelined form
        (include/aecm_batch.h: WebRtcAecmBatch_SetRaggedCleanPipelining; results never depend on it).  Off by default."""
        self._check(self.lib.WebRtcAecmBatch_SetRaggedCleanPipelining(self.h, 1 if enable else 0), "SetRaggedCleanPipelining")

    def launch_policy(self) -> AecmLaunchPolicy:
        p = AecmLaunchPolicy()
        self._check(self.lib.WebRtcAecmBatch_GetLaunchPolicy(self.h, C.byref(p)), "WebRtcAecmBatch_GetLaunchPolicy")
        return p

    def set_launch_policy(self, policy=None, **fields):
        """Set the batch's launch policy: a whole AecmLaunchPolicy, or the current one with `fields` changed
        (e.g. pipe_tail_waves=0, queue_min_streams=0)."""
        p = policy if policy is not None else self.launch_policy()
        for k, v in fields.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        self._check(self.lib.WebRtcAecmBatch_SetLaunchPolicy(self.h, C.byref(p)), "WebRtcAecmBatch_SetLaunchPolicy")

    def describe_launch(self, num_blocks, clean=False):
        """(form, chunk_blocks) of a ProcessBlocks launch of num_blocks blocks: form 0 / 1 = one wavefront per stream
        (small-launch variants / issue priority by phase), 2 = chunk queue, 3 = pipelined (chunk_blocks is then the shape: include/aecm_batch.h)."""
        chunk = C.c_int32(0)
        form = self.lib.WebRtcAecmBatch_DescribeLaunch(self.h, num_blocks, 1 if clean else 0, C.byref(chunk))
        if form < 0:
            raise AecmError(form, "WebRtcAecmBatch_DescribeLaunch")
        return form, chunk.value

    def set_block_trace(self, ptr, stream_stride, block_stride):
        """Attach a block trace (include/aecm_batch.h: WebRtcAecmBatch_SetBlockTrace): ptr = device memory for BLOCK_TRACE_DTYPE
        records, strides in records -- block k of a launch, for the stream at position s of it, goes to record
        s * stream_stride + k * block_stride.  From now on process_device / process_ragged_device write one record per block,
        never run pipelined, and the host-pointer forms raise (AECM_UNSUPPORTED_FUNCTION_ERROR).  Results do not change."""
        self._check(self.lib.WebRtcAecmBatch_SetBlockTrace(self.h, ptr, stream_stride, block_stride), "SetBlockTrace")

    def clear_block_trace(self):
        self._check(self.lib.WebRtcAecmBatch_SetBlockTrace(self.h, None, 0, 0), "SetBlockTrace")

    def set_config(self, cng_mode, echo_mode, first=0, count=-1):
        self._check(self.lib.WebRtcAecmBatch_set_config(self.h, AecmConfig(cng_mode, echo_mode), first, count), "set_config")

    def control(self, fixed_delay, nlp_flag, first=0, count=-1):
        self._check(self.lib.WebRtcAecmBatch_Control(self.h, fixed_delay, nlp_flag, first, count), "Control")

    def set_variant(self, variant):
        self._check(self.lib.WebRtcAecmBatch_SetKernelVariant(self.h, variant), "SetKernelVariant")

    def process_host(self, far, near, clean=None, out=None):
        """far/near: [S, T*64] int16 host arrays (stream-major).  Returns out [S, T*64] (written into `out` if given)."""
        far = np.ascontiguousarray(far, dtype=np.int16)
        near = np.ascontiguousarray(near, dtype=np.int16)
        assert far.shape == near.shape and far.shape[0] == self.num_streams and far.shape[1] % BLOCK == 0
        if out is None:
            out = np.empty_like(near)
        assert out.shape == near.shape and out.dtype == np.int16 and out.flags.c_contiguous
        cp = None
        if clean is not None:
            clean = np.ascontiguousarray(clean, dtype=np.int16)
            assert clean.shape == near.shape, "clean must have the shape of near"
            cp = clean.ctypes.data
        t = far.shape[1] // BLOCK
        self._check(self.lib.WebRtcAecmBatch_ProcessBlocksHost(self.h, far.ctypes.data, near.ctypes.data, cp,
                                                               out.ctypes.data, far.shape[1], BLOCK, t), "ProcessBlocksHost")
        return out

    def process_recordings_host(self, far, near, frame: int, ms: int = 40, clean=None):
        """far/near(/clean): [S, N] int16 host arrays, each stream a whole recording driven like the reference
        CLI (BufferFarend + Process per `frame` samples, constant msInSndCardBuf; clean = nearendClean).
        Returns (code, out)."""
        far = np.ascontiguousarray(far, dtype=np.int16)
        near = np.ascontiguousarray(near, dtype=np.int16)
        assert far.shape == near.shape and far.shape[0] == self.num_streams
        cptr = None
        if clean is not None:
            clean = np.ascontiguousarray(clean, dtype=np.int16)
            assert clean.shape == near.shape
            cptr = clean.ctypes.data
        out = near.copy()
        n_calls = far.shape[1] // frame
        rc = self.lib.WebRtcAecmBatch_ProcessRecordingsHost(self.h, far.ctypes.data, near.ctypes.data, cptr, out.ctypes.data,
                                                            far.shape[1], frame, n_calls, ms)
        return rc, out

    def process_recordings_device(self, far_ptr, near_ptr, out_ptr, stream_stride, frame, n_calls, ms=40, clean_ptr=None):
        return self.lib.WebRtcAecmBatch_ProcessRecordings(self.h, far_ptr, near_ptr, clean_ptr, out_ptr, stream_stride, frame,
                                                          n_calls, ms)

    def process_device(self, far_ptr, near_ptr, out_ptr, stream_stride, block_stride, num_blocks, clean_ptr=None):
        """Device pointers (e.g. torch .data_ptr()); asynchronous on the engine's stream."""
        self._check(self.lib.WebRtcAecmBatch_ProcessBlocks(self.h, far_ptr, near_ptr, clean_ptr, out_ptr, stream_stride,
                                                           block_stride, num_blocks), "ProcessBlocks")

    def _lengths(self, lengths):
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        if lengths.shape != (self.num_streams,):
            raise ValueError("one length per stream")
        return lengths

    def process_ragged_device(self, far_ptr, near_ptr, out_ptr, stream_stride, block_stride, num_blocks, blocks_per_stream, clean_ptr=None):
        """process_device with one block count per stream (host array, entries in [0, num_blocks]): stream s runs its first
        blocks_per_stream[s] blocks, its out blocks beyond that are not written.  Asynchronous on the engine's stream."""
        lens = self._lengths(blocks_per_stream)
        self._check(self.lib.WebRtcAecmBatch_ProcessBlocksRagged(self.h, far_ptr, near_ptr, clean_ptr, out_ptr, stream_stride, block_stride,
                                                                 num_blocks, lens.ctypes.data), "ProcessBlocksRagged")

    def process_ragged_host(self, far, near, blocks_per_stream, clean=None, out=None):
        """process_host with one block count per stream: far/near(/clean) [S, T*64] int16; stream s runs its first
        blocks_per_stream[s] <= T blocks.  Returns out [S, T*64]: `out` if given (blocks beyond a stream's length keep what
        they held), else a fresh array with zeros there."""
        far = np.ascontiguousarray(far, dtype=np.int16)
        near = np.ascontiguousarray(near, dtype=np.int16)
        assert far.shape == near.shape and far.shape[0] == self.num_streams and far.shape[1] % BLOCK == 0
        lens = self._lengths(blocks_per_stream)
        if out is None:
            out = np.zeros_like(near)
        assert out.shape == near.shape and out.dtype == np.int16 and out.flags.c_contiguous
        cp = None
        if clean is not None:
            clean = np.ascontiguousarray(clean, dtype=np.int16)
            assert clean.shape == near.shape, "clean must have the shape of near"
            cp = clean.ctypes.data
        self._check(self.lib.WebRtcAecmBatch_ProcessBlocksRaggedHost(self.h, far.ctypes.data, near.ctypes.data, cp, out.ctypes.data, far.shape[1],
                                                                     BLOCK, far.shape[1] // BLOCK, lens.ctypes.data), "ProcessBlocksRaggedHost")
        return out

    def process_recordings_ragged_host(self, far, near, frame: int, calls_per_stream, ms: int = 40, clean=None):
        """process_recordings_host with one call count per stream (entries in [0, N // frame]): stream s is a session of
        calls_per_stream[s] call pairs; its out row is 0 behind them.  Returns (code, out, codes[S])."""
        far = np.ascontiguousarray(far, dtype=np.int16)
        near = np.ascontiguousarray(near, dtype=np.int16)
        assert far.shape == near.shape and far.shape[0] == self.num_streams
        calls = self._lengths(calls_per_stream)
        cptr = None
        if clean is not None:
            clean = np.ascontiguousarray(clean, dtype=np.int16)
            assert clean.shape == near.shape
            cptr = clean.ctypes.data
        out = near.copy()
        codes = np.zeros(self.num_streams, dtype=np.int32)
        rc = self.lib.WebRtcAecmBatch_ProcessRecordingsRaggedHost(self.h, far.ctypes.data, near.ctypes.data, cptr, out.ctypes.data, far.shape[1],
                                                                  frame, far.shape[1] // frame, calls.ctypes.data, ms, codes.ctypes.data)
        if rc in (-1, AECM_UNSPECIFIED_ERROR, AECM_UNINITIALIZED_ERROR, AECM_NULL_POINTER_ERROR):      # the library's failure, not a session's code
            raise AecmError(rc, "WebRtcAecmBatch_ProcessRecordingsRaggedHost")
        return rc, out, codes

    def describe_ragged_launch(self, blocks_per_stream, clean=False) -> dict:
        """describe_ragged_launch (module level) as the engine decides it for this batch: under its launch policy, its kernel
        variant and its set_ragged_pipelining and set_ragged_clean_pipelining switches."""
        lens = self._lengths(blocks_per_stream)
        d = AecmLaunchDescription()
        items, total, longest = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._check(self.lib.WebRtcAecmBatch_DescribeRaggedLaunchOf(self.h, lens.ctypes.data, 1 if clean else 0, C.byref(d), C.byref(items),
                                                                    C.byref(total), C.byref(longest)), "DescribeRaggedLaunchOf")
        return dict(d.as_dict(), items=items.value, sum_blocks=total.value, max_blocks=longest.value)

    def synchronize(self):
        self._check(self.lib.WebRtcAecmBatch_Synchronize(self.h), "Synchronize")

    def last_launch_ms(self) -> float:
        ms = C.c_float()
        self._check(self.lib.WebRtcAecmBatch_GetLastLaunchMs(self.h, C.byref(ms)), "GetLastLaunchMs")
        return ms.value

    def timers(self):
        total, n = C.c_double(), C.c_int64()
        self._check(self.lib.WebRtcAecmBatch_GetTimers(self.h, C.byref(total), C.byref(n)), "GetTimers")
        return total.value, n.value

    def reset_timers(self):
        self._check(self.lib.WebRtcAecmBatch_ResetTimers(self.h), "ResetTimers")

    def digest(self, stream: int):
        d = np.zeros(DIGEST_WORDS, dtype=np.uint32)
        self._check(self.lib.WebRtcAecmBatch_GetDigest(self.h, stream, d.ctypes.data), "GetDigest")
        return d

    def export_state(self, stream: int) -> bytes:
        buf = C.create_string_buffer(self.lib.WebRtcAecmBatch_state_size_bytes())
        self._check(self.lib.WebRtcAecmBatch_ExportState(self.h, stream, buf, len(buf)), "ExportState")
        return buf.raw

    def import_state(self, stream: int, state: bytes):
        self._check(self.lib.WebRtcAecmBatch_ImportState(self.h, stream, state, len(state)), "ImportState")

    def export_states(self, first: int, count: int) -> np.ndarray:
        """Snapshots of streams [first, first + count) as a [count, state_size] uint8 array (one gather launch + chunked copies)."""
        n = self.lib.WebRtcAecmBatch_state_size_bytes()
        buf = np.empty((count, n), dtype=np.uint8)
        self._check(self.lib.WebRtcAecmBatch_ExportStates(self.h, first, count, buf.ctypes.data, buf.nbytes), "ExportStates")
        return buf

    def import_states(self, first: int, states: np.ndarray):
        states = np.ascontiguousarray(states, dtype=np.uint8)
        self._check(self.lib.WebRtcAecmBatch_ImportStates(self.h, first, states.shape[0], states.ctypes.data, states.nbytes), "ImportStates")

    def export_states_device(self, first: int, count: int, dev_ptr: int):
        n = self.lib.WebRtcAecmBatch_state_size_bytes()
        self._check(self.lib.WebRtcAecmBatch_ExportStatesDevice(self.h, first, count, dev_ptr, count * n), "ExportStatesDevice")

    def import_states_device(self, first: int, count: int, dev_ptr: int):
        n = self.lib.WebRtcAecmBatch_state_size_bytes()
        self._check(self.lib.WebRtcAecmBatch_ImportStatesDevice(self.h, first, count, dev_ptr, count * n), "ImportStatesDevice")

    def init_echo_path(self, stream, path):
        a, p = _i16(path)
        self._check(self.lib.WebRtcAecmBatch_InitEchoPath(self.h, stream, p, a.nbytes), "InitEchoPath")

    def get_echo_path(self, stream):
        out = np.zeros(BINS, dtype=np.int16)
        self._check(self.lib.WebRtcAecmBatch_GetEchoPath(self.h, stream, out.ctypes.data, out.nbytes), "GetEchoPath")
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.WebRtcAecmBatch_Free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AecmSessions:
    """S streaming sessions on a common clock (include/aecm_batch.h, WebRtcAecmSessions_*).  rates: None (every session at fs), or
    one rate per session (8000 / 16000; fs stays the object's own rate: WebRtcAecmSessions_InitRates)."""

    def __init__(self, num_streams: int, fs: int = 16000, cng_mode: int = 1, echo_mode: int = 3, device: int = 0, rates=None):
        self.lib = load()
        self.num_streams = num_streams
        self.h = self.lib.WebRtcAecmSessions_Create(num_streams, device)
        if not self.h:
            raise RuntimeError("WebRtcAecmSessions_Create failed: the HIP engine needs a usable MI355X (no CPU fallback exists)")
        rc = self.lib.WebRtcAecmSessions_Init(self.h, fs) if rates is None else self.init_rates(fs, rates)
        if rc != 0:
            raise AecmError(rc, "WebRtcAecmSessions_Init" if rates is None else "WebRtcAecmSessions_InitRates")
        rc = self.lib.WebRtcAecmSessions_set_config(self.h, AecmConfig(cng_mode, echo_mode))
        if rc != 0:
            raise AecmError(rc, "WebRtcAecmSessions_set_config")

    def _rows(self, far, near, clean):
        """Validated contiguous [S, n] int16 rows (the C side strides by far.shape[1] and reads S rows)."""
        far = np.ascontiguousarray(far, dtype=np.int16)
        near = np.ascontiguousarray(near, dtype=np.int16)
        if far.ndim != 2 or far.shape[0] != self.num_streams or far.shape[1] not in (80, 160):
            raise ValueError(f"far must be [{self.num_streams}, 80 or 160] int16, got {far.shape}")
        if near.shape != far.shape:
            raise ValueError(f"near {near.shape} must have the shape of far {far.shape}")
        cptr = None
        if clean is not None:
            clean = np.ascontiguousarray(clean, dtype=np.int16)
            if clean.shape != far.shape:
                raise ValueError(f"clean {clean.shape} must have the shape of far {far.shape}")
            cptr = clean.ctypes.data
        return far, near, clean, cptr

    def tick_host(self, far, near, ms: int = 40, clean=None):
        """far/near(/clean): [S, n] int16 (n = 80 or 160).  Returns (code, out)."""
        far, near, clean, cptr = self._rows(far, near, clean)
        out = np.empty_like(near)
        rc = self.lib.WebRtcAecmSessions_TickHost(self.h, far.ctypes.data, near.ctypes.data, cptr, out.ctypes.data, far.shape[1],
                                                  far.shape[1], ms)
        return rc, out

    def tick_device(self, far_ptr, near_ptr, out_ptr, stream_stride, n, ms=40, clean_ptr=None):
        return self.lib.WebRtcAecmSessions_Tick(self.h, far_ptr, near_ptr, clean_ptr, out_ptr, stream_stride, n, ms)

    def tick_host_per_session(self, far, near, ms_per_session, clean=None, flags=None):
        """far/near(/clean): [S, n] int16; ms_per_session: S msInSndCardBuf values; flags: S uint8 (SESSION_NO_FAREND,
        SESSION_SPLIT_CALLS, SESSION_IDLE, SESSION_HALF_CALL, SESSION_NO_CLEAN) or None.  Returns (code, out, codes[S]); the out row of a session
        that carries SESSION_IDLE is zeros, its code 0; so is the second half of the row of one that carries SESSION_HALF_CALL."""
        far, near, clean, cptr = self._rows(far, near, clean)
        ms = np.ascontiguousarray(ms_per_session, dtype=np.int16)
        if ms.shape != (self.num_streams,):
            raise ValueError("ms_per_session must have one entry per session")
        out = np.empty_like(near)
        codes = np.zeros(far.shape[0], dtype=np.int32)
        if flags is None:
            rc = self.lib.WebRtcAecmSessions_TickPerSessionHost(self.h, far.ctypes.data, near.ctypes.data, cptr, out.ctypes.data,
                                                                far.shape[1], far.shape[1], ms.ctypes.data, codes.ctypes.data)
        else:
            fl = np.ascontiguousarray(flags, dtype=np.uint8)
            if fl.shape != (self.num_streams,):
                raise ValueError("flags must have one entry per session")
            rc = self.lib.WebRtcAecmSessions_TickFlagsHost(self.h, far.ctypes.data, near.ctypes.data, cptr, out.ctypes.data,
                                                           far.shape[1], far.shape[1], ms.ctypes.data, fl.ctypes.data,
                                                           codes.ctypes.data)
        return rc, out, codes

    def buffer_farend_host(self, far, n: int, calls: int, calls_per_session=None) -> int:
        """Far-end burst (include/aecm_batch.h: WebRtcAecmSessions_BufferFarendHost): far [S, >= calls * n] int16; session s
        makes calls_per_session[s] (or `calls`) WebRtcAecm_BufferFarend calls of n samples."""
        far = np.ascontiguousarray(far, dtype=np.int16)
        if far.ndim != 2 or far.shape[0] != self.num_streams:
            raise ValueError(f"far must be [{self.num_streams}, >= calls * n] int16, got {far.shape}")
        cp = None
        if calls_per_session is not None:
            calls_per_session = np.ascontiguousarray(calls_per_session, dtype=np.uint8)
            if calls_per_session.shape != (self.num_streams,):
                raise ValueError("calls_per_session must have one entry per session")
            cp = calls_per_session.ctypes.data
        return self.lib.WebRtcAecmSessions_BufferFarendHost(self.h, far.ctypes.data, far.shape[1], n, calls, cp)

    def buffer_farend_device(self, far_ptr, stream_stride, n, calls, calls_per_session=None, asynchronous=False, wait_event=None, done_event=None):
        cp = None
        if calls_per_session is not None:
            calls_per_session = np.ascontiguousarray(calls_per_session, dtype=np.uint8)
            cp = calls_per_session.ctypes.data
        if asynchronous:
            return self.lib.WebRtcAecmSessions_BufferFarendAsync(self.h, far_ptr, stream_stride, n, calls, cp, wait_event, done_event)
        return self.lib.WebRtcAecmSessions_BufferFarend(self.h, far_ptr, stream_stride, n, calls, cp)

    def process_host(self, near, ms=40, clean=None, ms_per_session=None):
        """Every session's WebRtcAecm_Process without a WebRtcAecm_BufferFarend (WebRtcAecmSessions_ProcessHost).
        Returns (code, out, codes[S])."""
        near = np.ascontiguousarray(near, dtype=np.int16)
        if near.ndim != 2 or near.shape[0] != self.num_streams:
            raise ValueError(f"near must be [{self.num_streams}, n] int16, got {near.shape}")
        cptr = msp = None
        if clean is not None:
            clean = np.ascontiguousarray(clean, dtype=np.int16)
            if clean.shape != near.shape:
                raise ValueError("clean must have the shape of near")
            cptr = clean.ctypes.data
        if ms_per_session is not None:
            ms_per_session = np.ascontiguousarray(ms_per_session, dtype=np.int16)
            if ms_per_session.shape != (self.num_streams,):
                raise ValueError("ms_per_session must have one entry per session")
            msp = ms_per_session.ctypes.data
        out = np.empty_like(near)
        codes = np.zeros(self.num_streams, dtype=np.int32)
        rc = self.lib.WebRtcAecmSessions_ProcessHost(self.h, near.ctypes.data, cptr, out.ctypes.data, near.shape[1], near.shape[1], ms, msp,
                                                     codes.ctypes.data)
        return rc, out, codes

    def process_device(self, near_ptr, out_ptr, stream_stride, n, ms=40, clean_ptr=None, ms_per_session=None):
        msp = None
        if ms_per_session is not None:
            ms_per_session = np.ascontiguousarray(ms_per_session, dtype=np.int16)
            msp = ms_per_session.ctypes.data
        return self.lib.WebRtcAecmSessions_Process(self.h, near_ptr, clean_ptr, out_ptr, stream_stride, n, ms, msp, None)

    def init_session(self, session: int) -> int:
        return self.lib.WebRtcAecmSessions_InitSession(self.h, session)

    def init_rates(self, fs: int, rates) -> int:
        """WebRtcAecmSessions_InitRates: Init(fs), then session k a fresh instance at rates[k] where that differs (config: the
        default, as after WebRtcAecm_Init)."""
        rates = np.ascontiguousarray(rates, dtype=np.int32)
        if rates.shape != (self.num_streams,):
            raise ValueError("rates must have one entry per session")
        return self.lib.WebRtcAecmSessions_InitRates(self.h, fs, rates.ctypes.data)

    def init_session_rate(self, session: int, fs: int) -> int:
        return self.lib.WebRtcAecmSessions_InitSessionRate(self.h, session, fs)

    def get_session_rate(self, session: int):
        """(code, the session's own sampling rate)."""
        fs = C.c_int32(0)
        rc = self.lib.WebRtcAecmSessions_GetSessionRate(self.h, session, C.byref(fs))
        return rc, fs.value

    def import_session_any_rate(self, session: int, snapshot: bytes) -> int:
        return self.lib.WebRtcAecmSessions_ImportSessionAnyRate(self.h, session, snapshot, len(snapshot))

    def set_config_session(self, session: int, cng_mode: int, echo_mode: int) -> int:
        return self.lib.WebRtcAecmSessions_set_config_session(self.h, session, AecmConfig(cng_mode, echo_mode))

    def init_echo_path(self, session: int, path) -> int:
        a, p = _i16(path)
        return self.lib.WebRtcAecmSessions_InitEchoPath(self.h, session, p, a.nbytes)

    def get_echo_path(self, session: int):
        out = np.zeros(BINS, dtype=np.int16)
        rc = self.lib.WebRtcAecmSessions_GetEchoPath(self.h, session, out.ctypes.data, out.nbytes)
        return rc, out

    def export_session(self, session: int):
        """(code, snapshot bytes) of one live session (include/aecm_batch.h: WebRtcAecmSessions_ExportSession)."""
        buf = C.create_string_buffer(self.lib.WebRtcAecmSessions_session_size_bytes())
        rc = self.lib.WebRtcAecmSessions_ExportSession(self.h, session, buf, len(buf))
        return rc, buf.raw

    def import_session(self, session: int, snapshot: bytes) -> int:
        return self.lib.WebRtcAecmSessions_ImportSession(self.h, session, snapshot, len(snapshot))

    def _session_list(self, sessions, count=None):
        """(keep-alive array or None, pointer or None, count) of a session list; None: sessions 0 .. count-1 (all without a count)."""
        if sessions is None:
            return None, None, self.num_streams if count is None else count
        lst = np.ascontiguousarray(sessions, dtype=np.int32).reshape(-1)
        return lst, lst.ctypes.data, lst.size

    def export_sessions(self, sessions=None):
        """(code, snapshots as bytes: one per listed session, back to back, in list order; None: all) --
        WebRtcAecmSessions_ExportSessions."""
        lst, ptr, count = self._session_list(sessions)
        buf = np.zeros(count * self.lib.WebRtcAecmSessions_session_size_bytes(), dtype=np.uint8)
        rc = self.lib.WebRtcAecmSessions_ExportSessions(self.h, ptr, count, buf.ctypes.data, buf.nbytes)
        return rc, buf.tobytes()

    def import_sessions(self, sessions, snapshots, any_rate: bool = False) -> int:
        """WebRtcAecmSessions_ImportSessions: snapshots (bytes or a uint8 array) into the listed slots (None: 0 .. count-1), all or nothing."""
        n = self.lib.WebRtcAecmSessions_session_size_bytes()
        blob = np.frombuffer(snapshots, dtype=np.uint8) if isinstance(snapshots, (bytes, bytearray, memoryview)) else np.ascontiguousarray(snapshots, dtype=np.uint8).reshape(-1)
        lst, ptr, count = self._session_list(sessions, blob.size // n)
        return self.lib.WebRtcAecmSessions_ImportSessions(self.h, ptr, count, blob.ctypes.data, blob.size, 1 if any_rate else 0)

    def export_sessions_device(self, ptr: int, sessions=None) -> int:
        """WebRtcAecmSessions_ExportSessionsDevice into device memory (or a registered host buffer's alias) at ptr."""
        lst, lptr, count = self._session_list(sessions)
        return self.lib.WebRtcAecmSessions_ExportSessionsDevice(self.h, lptr, count, ptr, count * self.lib.WebRtcAecmSessions_session_size_bytes())

    def import_sessions_device(self, ptr: int, sessions, count: int, any_rate: bool = False) -> int:
        """WebRtcAecmSessions_ImportSessionsDevice: count snapshots at ptr into the listed slots (None: 0 .. count-1)."""
        lst, lptr, _ = self._session_list(sessions, count)
        return self.lib.WebRtcAecmSessions_ImportSessionsDevice(self.h, lptr, count, ptr, count * self.lib.WebRtcAecmSessions_session_size_bytes(),
                                                                1 if any_rate else 0)

    def tick_device_per_session(self, far_ptr, near_ptr, out_ptr, stream_stride, n, ms_per_session, clean_ptr=None):
        ms = np.ascontiguousarray(ms_per_session, dtype=np.int16)
        if ms.shape != (self.num_streams,):
            raise ValueError("ms_per_session must have one entry per session")
        return self.lib.WebRtcAecmSessions_TickPerSession(self.h, far_ptr, near_ptr, clean_ptr, out_ptr, stream_stride, n,
                                                          ms.ctypes.data, None)

    def tick_async(self, far_ptr, near_ptr, out_ptr, stream_stride, n, ms=40, clean_ptr=None, ms_per_session=None, flags=None,
                   wait_event=None, done_event=None):
        """Enqueue one tick and return without waiting for it (device pointers); see include/aecm_batch.h."""
        msp = flp = None
        if ms_per_session is not None:
            ms_per_session = np.ascontiguousarray(ms_per_session, dtype=np.int16)
            msp = ms_per_session.ctypes.data
        if flags is not None:
            flags = np.ascontiguousarray(flags, dtype=np.uint8)
            flp = flags.ctypes.data
        return self.lib.WebRtcAecmSessions_TickAsync(self.h, far_ptr, near_ptr, clean_ptr, out_ptr, stream_stride, n, ms, msp, flp, None,
                                                     wait_event, done_event)

    def tick_device_flags(self, far_ptr, near_ptr, out_ptr, stream_stride, n, ms_per_session, flags, clean_ptr=None):
        """WebRtcAecmSessions_TickFlags (device pointers).  Returns (code, codes[S]); the out row of a session that carries
        SESSION_IDLE is not written."""
        ms = np.ascontiguousarray(ms_per_session, dtype=np.int16)
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        if ms.shape != (self.num_streams,) or fl.shape != (self.num_streams,):
            raise ValueError("ms_per_session and flags must have one entry per session")
        codes = np.zeros(self.num_streams, dtype=np.int32)
        rc = self.lib.WebRtcAecmSessions_TickFlags(self.h, far_ptr, near_ptr, clean_ptr, out_ptr, stream_stride, n, ms.ctypes.data,
                                                   fl.ctypes.data, codes.ctypes.data)
        return rc, codes

    def tick_calls_host(self, far, near, calls: int, ms_per_session, clean=None, flags=None):
        """WebRtcAecmSessions_TickCallsHost: `calls` call pairs per session in one tick.  far/near(/clean): [S, calls * n] int16
        (n = 80 or 160; call c is columns [c n, (c + 1) n)); ms_per_session: S msInSndCardBuf values, or one int for everybody;
        flags: S uint8 (SESSION_NO_FAREND, SESSION_IDLE) or None.  Returns (code, out, codes[S]); an idle session's out row is zeros."""
        return self._tick_k_host(self.lib.WebRtcAecmSessions_TickCallsHost, far, near, calls, ms_per_session, clean, flags)

    def tick_packets_host(self, far, near, calls: int, ms_per_session, clean=None, flags=None):
        """WebRtcAecmSessions_TickPacketsHost: one packet of `calls` 10 ms calls per session, every session at its own rate and call
        size, rows packed.  far/near(/clean): [S, calls * n] int16 (n = 80 or 160: the object's tick); a session flagged
        SESSION_HALF_CALL (n = 160) makes calls of 80 samples on columns [c 80, (c + 1) 80), everybody else calls of n on
        [c n, (c + 1) n); flags: S uint8 (SESSION_NO_FAREND, SESSION_IDLE, SESSION_HALF_CALL) or None.  Returns (code, out, codes[S]);
        an idle session's out row and a half-call session's columns [calls * 80, calls * 160) are zeros."""
        return self._tick_k_host(self.lib.WebRtcAecmSessions_TickPacketsHost, far, near, calls, ms_per_session, clean, flags)

    def _tick_k_host(self, fn, far, near, calls, ms_per_session, clean, flags):
        far = np.ascontiguousarray(far, dtype=np.int16)
        near = np.ascontiguousarray(near, dtype=np.int16)
        if far.ndim != 2 or far.shape[0] != self.num_streams or near.shape != far.shape:
            raise ValueError(f"far and near must be [{self.num_streams}, calls * n] int16, got {far.shape} and {near.shape}")
        if calls < 1 or far.shape[1] % calls != 0:
            raise ValueError("the rows must hold `calls` calls of n samples")
        cptr = None
        if clean is not None:
            clean = np.ascontiguousarray(clean, dtype=np.int16)
            if clean.shape != far.shape:
                raise ValueError(f"clean {clean.shape} must have the shape of far {far.shape}")
            cptr = clean.ctypes.data
        ms, msp, fl, flp = self._calls_args(ms_per_session, flags)
        out = np.empty_like(near)
        codes = np.zeros(self.num_streams, dtype=np.int32)
        rc = fn(self.h, far.ctypes.data, near.ctypes.data, cptr, out.ctypes.data, far.shape[1], far.shape[1] // calls, calls, ms, msp, flp,
                codes.ctypes.data)
        return rc, out, codes

    def _calls_args(self, ms_per_session, flags):
        """(scalar ms, pointer or None, keep-alive flags array, pointer or None) of a K-call tick's per-session arguments."""
        if np.ndim(ms_per_session) == 0:
            ms, msp = int(ms_per_session), None
            self._calls_ms = None
        else:
            self._calls_ms = np.ascontiguousarray(ms_per_session, dtype=np.int16)
            if self._calls_ms.shape != (self.num_streams,):
                raise ValueError("ms_per_session must have one entry per session")
            ms, msp = 0, self._calls_ms.ctypes.data
        fl = flp = None
        if flags is not None:
            fl = np.ascontiguousarray(flags, dtype=np.uint8)
            if fl.shape != (self.num_streams,):
                raise ValueError("flags must have one entry per session")
            flp = fl.ctypes.data
        return ms, msp, fl, flp

    def tick_calls_device(self, far_ptr, near_ptr, out_ptr, stream_stride, n, calls: int, ms_per_session, clean_ptr=None, flags=None,
                          asynchronous=False, wait_event=None, done_event=None):
        """WebRtcAecmSessions_TickCalls / TickCallsAsync (device pointers; rows of stream_stride >= calls * n samples).  Returns
        (code, codes[S]); the out row of a session that carries SESSION_IDLE is not written."""
        ms, msp, fl, flp = self._calls_args(ms_per_session, flags)
        codes = np.zeros(self.num_streams, dtype=np.int32)
        if asynchronous:
            rc = self.lib.WebRtcAecmSessions_TickCallsAsync(self.h, far_ptr, near_ptr, clean_ptr, out_ptr, stream_stride, n, calls, ms, msp, flp,
                                                            codes.ctypes.data, wait_event, done_event)
        else:
            rc = self.lib.WebRtcAecmSessions_TickCalls(self.h, far_ptr, near_ptr, clean_ptr, out_ptr, stream_stride, n, calls, ms, msp, flp,
                                                       codes.ctypes.data)
        return rc, codes

    def tick_packets_device(self, far_ptr, near_ptr, out_ptr, stream_stride, n, calls: int, ms_per_session, clean_ptr=None, flags=None,
                            asynchronous=False, wait_event=None, done_event=None):
        """WebRtcAecmSessions_TickPackets / TickPacketsAsync (device pointers; rows of stream_stride >= calls * n samples, packed per
        session: see tick_packets_host).  Returns (code, codes[S]); the out row of a session that carries SESSION_IDLE and the samples
        [calls * 80, calls * 160) of one that carries SESSION_HALF_CALL are not written."""
        ms, msp, fl, flp = self._calls_args(ms_per_session, flags)
        codes = np.zeros(self.num_streams, dtype=np.int32)
        if asynchronous:
            rc = self.lib.WebRtcAecmSessions_TickPacketsAsync(self.h, far_ptr, near_ptr, clean_ptr, out_ptr, stream_stride, n, calls, ms, msp, flp,
                                                              codes.ctypes.data, wait_event, done_event)
        else:
            rc = self.lib.WebRtcAecmSessions_TickPackets(self.h, far_ptr, near_ptr, clean_ptr, out_ptr, stream_stride, n, calls, ms, msp, flp,
                                                         codes.ctypes.data)
        return rc, codes

    def get_session_clean_mode(self, session: int):
        """(code, 0 no Process call since the session's last initialisation / 1 all with a clean input / 2 none / 3 both)."""
        mode = C.c_int32(-1)
        rc = self.lib.WebRtcAecmSessions_GetSessionCleanMode(self.h, session, C.byref(mode))
        return rc, mode.value

    def split_clean_two_launches(self, on=True) -> int:
        """Diagnostics: the tick launch of a tick with SESSION_NO_CLEAN sessions and others -- True: always one launch per list,
        False: always the fused launch, None: by the size of the tick (the default of a new object)."""
        return self.lib.WebRtcAecmSessions_SplitCleanTwoLaunches(self.h, -1 if on is None else 1 if on else 0)

    def set_split_call_ticks(self, on: bool = True) -> int:
        """K-call and packet ticks (calls > 1) with a clean plane and SESSION_NO_CLEAN sessions among the callers: accepted while on,
        AECM_UNSUPPORTED_FUNCTION_ERROR while off, the default (WebRtcAecmSessions_SetSplitCallTicks).  The object's switch: it
        survives init()."""
        return self.lib.WebRtcAecmSessions_SetSplitCallTicks(self.h, 1 if on else 0)

    def set_session_trace(self, ptr, session_stride, tick_stride, ring_ticks) -> int:
        """Attach a session trace (include/aecm_batch.h: WebRtcAecmSessions_SetSessionTrace): ptr = device memory for
        SESSION_TRACE_DTYPE records; tick j since attachment writes session s's record at record index
        s * session_stride + (j % ring_ticks) * tick_stride.  Returns the code."""
        return self.lib.WebRtcAecmSessions_SetSessionTrace(self.h, ptr, session_stride, tick_stride, ring_ticks)

    def clear_session_trace(self) -> int:
        return self.lib.WebRtcAecmSessions_SetSessionTrace(self.h, None, 0, 0, 0)

    def session_trace_ticks(self) -> int:
        """Ticks accepted since the trace was attached (0 while none is)."""
        ticks = C.c_int64(-1)
        rc = self.lib.WebRtcAecmSessions_GetSessionTraceTicks(self.h, C.byref(ticks))
        if rc != 0:
            raise RuntimeError(f"WebRtcAecmSessions_GetSessionTraceTicks: {rc}")
        return ticks.value

    def set_call_trace(self, ptr, session_stride, call_stride, ring_calls) -> int:
        """Attach a call trace (include/aecm_batch.h: WebRtcAecmSessions_SetCallTrace): ptr = device memory for SESSION_TRACE_DTYPE
        records, one per session and call pair -- K-call and packet ticks too; call slot j since attachment writes session s's
        record at record index s * session_stride + (j % ring_calls) * call_stride.  Returns the code."""
        return self.lib.WebRtcAecmSessions_SetCallTrace(self.h, ptr, session_stride, call_stride, ring_calls)

    def clear_call_trace(self) -> int:
        return self.lib.WebRtcAecmSessions_SetCallTrace(self.h, None, 0, 0, 0)

    def call_trace_calls(self) -> int:
        """Call slots counted since the call trace was attached (0 while none is)."""
        calls = C.c_int64(-1)
        rc = self.lib.WebRtcAecmSessions_GetCallTraceCalls(self.h, C.byref(calls))
        if rc != 0:
            raise RuntimeError(f"WebRtcAecmSessions_GetCallTraceCalls: {rc}")
        return calls.value

    def force_sparse_ticks(self, on: bool = True) -> int:
        """Diagnostics: every tick through the live list and the sparse tick kernel (WebRtcAecmSessions_ForceSparseTicks)."""
        return self.lib.WebRtcAecmSessions_ForceSparseTicks(self.h, 1 if on else 0)

    def synchronize(self):
        return self.lib.WebRtcAecmSessions_Synchronize(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.WebRtcAecmSessions_Free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def register_host_buffer(array, device: int = 0) -> int:
    """Pin + map a caller-owned numpy array (zero-copy host audio); returns its device alias for the *_dev arguments."""
    lib = load()
    dev = C.c_void_p()
    rc = lib.WebRtcAecmBatch_RegisterHostBuffer(device, array.ctypes.data, array.nbytes, C.byref(dev))
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_RegisterHostBuffer")
    return dev.value


def unregister_host_buffer(array, device: int = 0) -> None:
    rc = load().WebRtcAecmBatch_UnregisterHostBuffer(device, array.ctypes.data)
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_UnregisterHostBuffer")


def self_test(device: int = 0, exhaustive: bool = False):
    """Device self test of the wave primitives; returns the 8 failure counters (all must be 0)."""
    lib = load()
    f = np.zeros(8, dtype=np.uint64)
    rc = lib.WebRtcAecmBatch_SelfTest(device, 1 if exhaustive else 0, f.ctypes.data)
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_SelfTest")
    return f


def check_counters(device: int = 0, reset: bool = False):
    """Precondition-violation counters of the audit build (AECM_LIB_PATH=.../libaecm_mi355x_checked.so):
    [mul24 operands, as_i16 arguments].  Raises AecmError(12001) on the shipped library."""
    lib = load()
    c = np.zeros(2, dtype=np.uint64)
    rc = lib.WebRtcAecmBatch_GetCheckCounters(device, c.ctypes.data, 1 if reset else 0)
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_GetCheckCounters")
    return c


def debug_fft128(re, im, variant: int, kernel_variant: int = KERNEL_FAST, device: int = 0):
    """Run the block kernel's own 128-point transform on (count, 128) int16 arrays; returns (re, im, scales).
    variant: 0 forward of real input, 1 forward complex, 2 inverse (see include/aecm_batch.h)."""
    lib = load()
    re = np.ascontiguousarray(re, dtype=np.int16).reshape(-1, 128)
    im = np.ascontiguousarray(im, dtype=np.int16).reshape(-1, 128)
    data = np.ascontiguousarray(np.concatenate([re, im], axis=1))
    scales = np.zeros(re.shape[0], dtype=np.int32)
    rc = lib.WebRtcAecmBatch_DebugFft128(device, data.ctypes.data, scales.ctypes.data, variant, kernel_variant, re.shape[0])
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_DebugFft128")
    return data[:, :128].copy(), data[:, 128:].copy(), scales


def debug_ops_names():
    """The names of the ops probe's entries, in id order (webrtc_aecm_amd/csrc/aecm_ops_table.inc, as the library was built with it)."""
    lib = load()
    return [lib.WebRtcAecmBatch_DebugOpName(k).decode() for k in range(lib.WebRtcAecmBatch_DebugOpsCount())]


def debug_ops(op, a, b=None, c=None, form: int = 0, device: int = 0):
    """One primitive of aecm_ops.h / plain-integer helper of aecm_wave.h on the device, alone (include/aecm_batch.h:
    WebRtcAecmBatch_DebugOps).  op: an id or a name of debug_ops_names(); a, b, c: int32 arrays of one length (b, c where the
    op takes them); form 0 = one tuple per lane, 1 = one tuple per wave with wave-uniform operands.  Returns (out, nonuniform)."""
    lib = load()
    if isinstance(op, str):
        op = debug_ops_names().index(op)
    a = np.ascontiguousarray(a, dtype=np.int32).ravel()
    ops = [a] + [None if x is None else np.ascontiguousarray(x, dtype=np.int32).ravel() for x in (b, c)]
    if any(x is not None and x.size != a.size for x in ops):
        raise ValueError("debug_ops: operand arrays of different lengths")
    out = np.zeros(a.size, dtype=np.int32)
    nonuniform = np.zeros(a.size, dtype=np.int32)
    rc = lib.WebRtcAecmBatch_DebugOps(device, op, form, *[None if x is None else x.ctypes.data for x in ops], out.ctypes.data,
                                      nonuniform.ctypes.data, a.size)
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_DebugOps")
    return out, nonuniform


def describe_launch_for(num_streams: int, compute_units: int, num_blocks: int, clean: bool = False):
    """(form, chunk_blocks / shape) a default-configured batch of num_streams streams would launch num_blocks blocks with on a
    device of compute_units CUs (AecmBatch.describe_launch without a device: the launch-form rules are host logic)."""
    chunk = C.c_int32(0)
    form = load().WebRtcAecmBatch_DescribeLaunchFor(num_streams, compute_units, num_blocks, 1 if clean else 0, C.byref(chunk))
    if form < 0:
        raise AecmError(form, "WebRtcAecmBatch_DescribeLaunchFor")
    return form, chunk.value


def default_launch_policy(compute_units: int) -> AecmLaunchPolicy:
    p = AecmLaunchPolicy()
    rc = load().WebRtcAecmBatch_DefaultLaunchPolicy(compute_units, C.byref(p))
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_DefaultLaunchPolicy")
    return p


def describe_launch_detail(num_streams: int, num_blocks: int, compute_units: int = 0, clean: bool = False, policy=None,
                           clean_pipelining: bool = False) -> dict:
    """Form, shape, grid and chip quantisation of a launch (include/aecm_batch.h: AecmLaunchDescription), without a device:
    under `policy` (an AecmLaunchPolicy) or the default policy of compute_units.  clean_pipelining: as on a batch that has
    opted in (AecmBatch.set_clean_pipelining)."""
    d = AecmLaunchDescription()
    pol = C.byref(policy) if policy is not None else None
    if clean_pipelining:
        rc = load().WebRtcAecmBatch_DescribeLaunchDetailEx(pol, compute_units, num_streams, num_blocks, 1 if clean else 0, 1, C.byref(d))
    else:
        rc = load().WebRtcAecmBatch_DescribeLaunchDetail(pol, compute_units, num_streams, num_blocks, 1 if clean else 0, C.byref(d))
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_DescribeLaunchDetail")
    return d.as_dict()


def block_trace_size_bytes() -> int:
    return load().WebRtcAecmBatch_block_trace_size_bytes()


def session_trace_size_bytes() -> int:
    return load().WebRtcAecmSessions_session_trace_size_bytes()


def describe_traced_launch(num_streams: int, num_blocks: int, compute_units: int = 0, clean: bool = False, policy=None) -> dict:
    """describe_launch_detail for a batch with a block trace attached (AecmBatch.set_block_trace), without a device: never the
    pipelined form -- such a size runs one wavefront per stream -- and describe_launch_detail's answer everywhere else."""
    d = AecmLaunchDescription()
    pol = C.byref(policy) if policy is not None else None
    rc = load().WebRtcAecmBatch_DescribeTracedLaunch(pol, compute_units, num_streams, num_blocks, 1 if clean else 0, C.byref(d))
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_DescribeTracedLaunch")
    return d.as_dict()


def describe_ragged_launch(blocks_per_stream, compute_units: int = 0, clean: bool = False, policy=None, ragged_pipelining: bool = False,
                           ragged_clean_pipelining: bool = False) -> dict:
    """describe_launch_detail for a ragged launch (one block count per stream), without a device: the AecmLaunchDescription
    fields plus items (the chunk queue's (chunk, stream) items; 0 for the other forms), sum_blocks (the useful work) and
    max_blocks (the critical path).  ragged_pipelining / ragged_clean_pipelining: the answer for a batch that has opted in
    (AecmBatch.set_ragged_pipelining / set_ragged_clean_pipelining)."""
    lens = np.ascontiguousarray(blocks_per_stream, dtype=np.int32)
    d = AecmLaunchDescription()
    items, total, longest = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    pol = C.byref(policy) if policy is not None else None
    if ragged_clean_pipelining:
        name = "WebRtcAecmBatch_DescribeRaggedLaunchEx2"
        rc = load().WebRtcAecmBatch_DescribeRaggedLaunchEx2(pol, compute_units, lens.size, lens.ctypes.data, 1 if clean else 0,
                                                            1 if ragged_pipelining else 0, 1, C.byref(d), C.byref(items), C.byref(total),
                                                            C.byref(longest))
    elif ragged_pipelining:
        name = "WebRtcAecmBatch_DescribeRaggedLaunchEx"
        rc = load().WebRtcAecmBatch_DescribeRaggedLaunchEx(pol, compute_units, lens.size, lens.ctypes.data, 1 if clean else 0, 1, C.byref(d),
                                                           C.byref(items), C.byref(total), C.byref(longest))
    else:
        name = "WebRtcAecmBatch_DescribeRaggedLaunch"
        rc = load().WebRtcAecmBatch_DescribeRaggedLaunch(pol, compute_units, lens.size, lens.ctypes.data, 1 if clean else 0, C.byref(d),
                                                         C.byref(items), C.byref(total), C.byref(longest))
    if rc != 0:
        raise AecmError(rc, name)
    return dict(d.as_dict(), items=items.value, sum_blocks=total.value, max_blocks=longest.value)


def ragged_pipe_plan(blocks_per_stream, compute_units: int = 0, policy=None):
    """slot_stream[workgroups][4] of the plan a ragged pipelined launch runs by (include/aecm_batch.h: WebRtcAecmBatch_RaggedPipePlan):
    the stream in each slot of each workgroup, -1 = empty; workgroups i, i + compute units, ... share a compute unit."""
    lens = np.ascontiguousarray(blocks_per_stream, dtype=np.int32)
    cap = 4 * max(int((lens > 0).sum()), 1)              # a workgroup of the plan holds at least one stream
    slots = np.full(cap, -1, dtype=np.int32)
    n_wg = C.c_int32(0)
    rc = load().WebRtcAecmBatch_RaggedPipePlan(C.byref(policy) if policy is not None else None, compute_units, lens.size, lens.ctypes.data,
                                               slots.ctypes.data, cap, C.byref(n_wg))
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_RaggedPipePlan")
    return slots[:4 * n_wg.value].reshape(n_wg.value, 4)


def ragged_plan(blocks_per_stream, chunk_blocks: int):
    """(order, first_item) of the plan a ragged chunk-queue launch runs by (include/aecm_batch.h: WebRtcAecmBatch_RaggedPlan)."""
    lens = np.ascontiguousarray(blocks_per_stream, dtype=np.int32)
    order = np.zeros(lens.size, dtype=np.int32)
    cap = (int(lens.max(initial=0)) + chunk_blocks - 1) // max(chunk_blocks, 1) + 1 if chunk_blocks > 0 else 1
    first_item = np.zeros(cap, dtype=np.int32)
    n_chunks = C.c_int32(0)
    rc = load().WebRtcAecmBatch_RaggedPlan(lens.size, lens.ctypes.data, chunk_blocks, order.ctypes.data, first_item.ctypes.data, cap, C.byref(n_chunks))
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_RaggedPlan")
    return order, first_item[:n_chunks.value + 1]


def describe_tick(num_sessions: int, compute_units: int) -> dict:
    d = AecmLaunchDescription()
    rc = load().WebRtcAecmSessions_DescribeTick(num_sessions, compute_units, C.byref(d))
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmSessions_DescribeTick")
    return d.as_dict()


def describe_tick_live(num_sessions: int, live_sessions: int, compute_units: int) -> dict:
    """WebRtcAecmSessions_DescribeTickLive: the tick launch of an object of num_sessions sessions of which live_sessions call."""
    d = AecmLaunchDescription()
    rc = load().WebRtcAecmSessions_DescribeTickLive(num_sessions, live_sessions, compute_units, C.byref(d))
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmSessions_DescribeTickLive")
    return d.as_dict()


def set_default_device(device: int) -> int:
    return load().WebRtcAecm_SetDefaultDevice(device)


def device_pci_bus_id(device: int = 0) -> str:
    buf = C.create_string_buffer(32)
    rc = load().WebRtcAecmBatch_DevicePciBusId(device, buf, 32)
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_DevicePciBusId")
    return buf.value.decode()


def device_info(device: int = 0):
    lib = load()
    name = C.create_string_buffer(64)
    cu, clk = C.c_int32(), C.c_int32()
    rc = lib.WebRtcAecmBatch_DeviceInfo(device, name, 64, C.byref(cu), C.byref(clk))
    if rc != 0:
        raise AecmError(rc, "WebRtcAecmBatch_DeviceInfo")
    return name.value.decode(), cu.value, clk.value

"""The recorded launch table: every field the planning ABI returns (no device needed) for a fixed grid of launches.

tests/golden/launch_table.json.gz was recorded from the library of the commit BEFORE the launch rule moved into one plan-making
function (aecm_engine.cpp: PlanLaunch / PlanRaggedLaunch); tests/test_launch_table.py replays the grid against the built
library and compares every field.  The engine launches the plan these calls describe, so the table pins what runs, not only
what is reported.  Re-record (only when a launch rule is changed on purpose):

    python tests/launch_table.py --record   # writes the fixture from the library load() binds (AECM_LIB_PATH: another one)
"""
from __future__ import annotations

import gzip
import json
import sys
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
FIXTURE = ROOT / "tests" / "golden" / "launch_table.json.gz"

CUS = (64, 256, 304)
BLOCKS = (1, 2, 3, 63, 64, 127, 128, 255, 256, 300)
DESCRIPTION = ("form", "chunk_blocks", "shape", "workgroups", "waves_per_workgroup", "workgroups_per_cu", "rounds_x1000", "cu_load_evenness_x1000")
PATTERNS = ("equal", "one_long", "uniform", "mostly_zero")
# wishes on top of the default policy of a CU count
POLICIES = (dict(queue_min_streams=0), dict(queue_chunk_blocks=16, queue_chunk_explicit=1), dict(queue_min_streams=0, queue_chunk_blocks=48, queue_chunk_explicit=1),
            dict(pipe_gain_waves=0), dict(pipe_spread=0, pipe_wgs_per_cu=1), dict(pipelined_min_streams=0), dict(pipelined_min_blocks=1, pipe_tail_waves=0),
            dict(queue_chunk_blocks=0))


def stream_counts(cus):
    """On and on either side of every boundary tests/test_capi.py::test_launch_form_rules_without_a_device names: one stream | two;
    4, 8, 12 (tail_max), 16 (pipe_max), 24 (rotation) and 28 (resident) streams per CU."""
    return [1, 2, 3] + [k * cus + d for k in (4, 8, 12, 16, 24, 28) for d in (-1, 0, 1)]


def lengths(pattern, S, longest, seed):
    rng = np.random.default_rng(seed)
    if pattern == "equal":
        return np.full(S, longest, dtype=np.int32)
    if pattern == "one_long":
        lens = np.full(S, max(longest // 8, 1), dtype=np.int32)
        lens[int(rng.integers(S))] = longest
        return lens
    if pattern == "uniform":
        lens = rng.integers(0, longest + 1, S).astype(np.int32)
        lens[int(rng.integers(S))] = longest
        return lens
    lens = np.zeros(S, dtype=np.int32)                       # mostly zero, a few live
    live = rng.choice(S, size=max(1, min(S, S // 16 + 2)), replace=False)
    lens[live] = rng.integers(1, longest + 1, live.size)
    lens[live[0]] = longest
    return lens


def _policy(aecm, cus, wishes):
    if not wishes:
        return None
    p = aecm.default_launch_policy(cus)
    for k, v in wishes.items():
        setattr(p, k, v)
    return p


def _crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.int32).tobytes())


def _call(aecm, fn):
    try:
        return fn()
    except aecm.AecmError as e:
        return ["error", e.code]


def record():
    """{table name: [[inputs ..., outputs ...], ...]} from the library load() binds."""
    import webrtc_aecm_amd as aecm
    table = {"equal": [], "ragged": [], "pipe_plan": [], "ragged_plan": []}
    # equal-length launches: DescribeLaunchDetailEx
    for cus in CUS:
        for S in stream_counts(cus):
            for T in BLOCKS:
                for clean, opt_in in ((0, 0), (1, 0), (1, 1), (0, 1)):
                    d = aecm.describe_launch_detail(S, T, cus, bool(clean), clean_pipelining=bool(opt_in))
                    table["equal"].append([cus, -1, S, T, clean, opt_in] + [d[k] for k in DESCRIPTION])
        for n, wishes in enumerate(POLICIES):
            for S in (2, 4 * cus, 8 * cus + 1, 16 * cus, 16 * cus + 1, 28 * cus + 1):
                for T in (2, 3, 64, 300):
                    for clean, opt_in in ((0, 0), (1, 1)):
                        d = aecm.describe_launch_detail(S, T, 0, bool(clean), policy=_policy(aecm, cus, wishes), clean_pipelining=bool(opt_in))
                        table["equal"].append([cus, n, S, T, clean, opt_in] + [d[k] for k in DESCRIPTION])
    # ragged launches: DescribeRaggedLaunchEx, and the plans the queue and the pipelined form run by
    seed = 0
    for cus in CUS:
        for S in (2, 3, 8 * cus + 1, 16 * cus - 1, 16 * cus, 16 * cus + 1, 28 * cus, 28 * cus + 1):
            for longest in (2, 3, 64, 256, 300):
                for pattern in PATTERNS:
                    seed += 1
                    lens = lengths(pattern, S, longest, seed)
                    for n in (-1, 0, 1) if pattern != "equal" else (-1,):
                        for clean, opt_in in ((0, 0), (0, 1), (1, 1)):
                            pol = _policy(aecm, cus, POLICIES[n] if n >= 0 else None)
                            d = _call(aecm, lambda: aecm.describe_ragged_launch(lens, 0 if pol is not None else cus, bool(clean), pol, bool(opt_in)))
                            out = d if isinstance(d, list) else [d[k] for k in DESCRIPTION + ("items", "sum_blocks", "max_blocks")]
                            table["ragged"].append([cus, n, S, longest, PATTERNS.index(pattern), seed, clean, opt_in] + out)
                    if longest in (3, 300):
                        p = _call(aecm, lambda: aecm.ragged_pipe_plan(lens, cus))
                        table["pipe_plan"].append([cus, S, longest, PATTERNS.index(pattern), seed] + (p if isinstance(p, list) else [int(p.shape[0]), _crc(p)]))
                    if longest in (64, 300) and cus == 256:
                        for chunk in (8, 32, 128):
                            p = _call(aecm, lambda: aecm.ragged_plan(lens, chunk))
                            table["ragged_plan"].append([S, longest, PATTERNS.index(pattern), seed, chunk] +
                                                        (p if isinstance(p, list) else [int(p[1].size) - 1, _crc(p[0]), _crc(p[1])]))
    return table


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/launch_table.py --record   (overwrites tests/golden/launch_table.json.gz)")
    from webrtc_aecm_amd import build as hip_build
    table = record()
    table["recorded_from"] = hip_build.build_info()
    FIXTURE.write_bytes(gzip.compress(json.dumps(table, separators=(",", ":")).encode(), mtime=0))
    print({k: len(v) for k, v in table.items()}, FIXTURE.stat().st_size, "bytes")

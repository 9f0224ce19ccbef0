"""The launch rule against the table recorded before it moved into one plan-making function (tests/launch_table.py has the grid and
the recorder): CU counts 64 / 256 / 304, stream counts on and either side of every form boundary, block counts 1 .. 300, with and
without a clean input, both opt-in switches, policies with wishes, four ragged length patterns.  No device needed."""
import gzip
import json

import launch_table


def test_every_planning_call_returns_what_the_recorded_table_holds():
    want = json.loads(gzip.decompress(launch_table.FIXTURE.read_bytes()))
    got = launch_table.record()
    for name, rows in got.items():
        assert len(rows) == len(want[name]) and len(rows) >= 190, (name, len(rows), len(want[name]))
        differ = [(w, g) for w, g in zip(want[name], rows) if w != g]
        assert not differ, (name, len(differ), differ[:5])

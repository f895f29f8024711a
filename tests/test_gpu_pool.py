"""examples/pool_example.cpp: the device allocator's events order real work on the device (the
allocator's logic itself is tested on the CPU, test_pool_model.py).  A block above kChunk and
kSlackMin is filled FILLS times on stream A, freed on A and handed to stream B while A still runs
(`overlapped`: required, otherwise nothing was shown); B's zero fill must not be overtaken by A's
fills.  Then reuse after a drain, small blocks kept from another stream while the freeing stream is
busy, and the teardown of a stream.  FILLS = 64 whole-block fills keep A busy long enough."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "pool_example")
FILLS = 64


def test_pool_example():
    out = subprocess.run([BIN, str(FILLS)], capture_output=True, text=True, timeout=100)
    print(out.stdout, out.stderr[-2000:])
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0, (rows, out.stderr[-2000:])
    got = {r["check"]: r for r in rows if "check" in r}
    cross = got["cross_stream_reuse"]
    assert cross["fills"] == FILLS and cross["bytes"] > (2 << 30)
    assert cross["overlapped"] is True, cross
    assert cross["same_pointer"] and cross["held_unchanged"] and cross["nonzero_bytes"] == 0, cross
    assert got["reuse_after_drain"]["ok"]
    small = got["small_blocks"]
    assert small["overlapped"] and small["kept_from_b_while_busy"] and small["handed_to_b_after_sync"], small
    tear = got["stream_teardown"]
    assert tear["blocks_reused"] and tear["no_growth"] and tear["live_after"] == 0, tear
    assert rows[-1] == {"done": "pool_example", "ok": True}

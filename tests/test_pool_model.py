"""CPU model test of the caching device allocator (phantom::DevicePool, host/buffer.cpp) through
phantom-fhe-boot_amd/pooltest/pool_model.cpp: buffer.cpp compiled unchanged by the host compiler
against a fake HIP runtime in which streams advance only when the test says so.  No GPU is touched.

random:    200,000 random allocations, frees (some retagged to another stream behind a wait, some
           `completed` after a drain), stream advances, stream creations and OwnedStream-style
           teardowns over the null stream and 1..6 others.  After every step no two live blocks
           overlap, stats() equals the model, and every range handed to a stream is ordered behind
           its last use on any other stream (completed, or a happens-before edge).  At least 1,000
           reuses per seed must have been of a range whose last use on another stream was still
           incomplete, or the run showed nothing (2,452 .. 8,005 for seeds 1..5).
scenarios: coalescing, the slack rule, the out-of-memory ladder (rungs counted in the fake runtime),
           the small path, stream teardown with reuse of the handle value.
threads:   4 threads, one stream each, hipMalloc of a chunk sleeping 1 ms (the window in which
           grow() has released the pool's mutex); overlap and statistics.
doublefree: a second free of a block ends the process by abort() with the pool's message."""
import json
import os
import signal
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "phantom-fhe-boot_amd", "bin", "pool_model")


def run(*args):
    out = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr[-2000:])
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0 and res["ok"], (res, out.stderr[-2000:])
    assert res["failures"] == 0 and res["runtime_errors"] == 0, res
    return res


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_pool_random(seed):
    res = run("random", str(seed), "200000")
    assert res["seed"] == seed and res["steps"] == 200000
    assert res["violations"] == 0
    assert res["incomplete_cross_stream_reuses"] >= 1000, res
    assert res["cross_stream_reuses"] >= res["incomplete_cross_stream_reuses"]
    # every kind of step happened, and no genuine out-of-memory was involved
    assert res["retags"] > 0 and res["completed_frees"] > 0 and res["streams_destroyed"] > 0
    assert res["malloc_failures"] == 0


def test_pool_coalesce():
    res = run("scenario", "coalesce")
    assert res["mallocs"] == 2 and res["held"] == (1 << 30) + 512  # one chunk and one small block


def test_pool_slack_rule():
    res = run("scenario", "slack")
    assert res["waits_above_slack"] == 1 and res["waits_below_slack"] == 0


def test_pool_out_of_memory_ladder():
    """Rungs: release of the cache (2 blocks returned, then 3 after the synchronise), wait-carve (once
    in the ladder, once after the throw), device synchronise (rungs 3 and 4), the thrown error."""
    res = run("scenario", "ladder")
    assert res["malloc_failures"] == 10
    assert res["released_to_runtime"] == 5
    assert res["wait_carves"] == 2
    assert res["device_syncs"] == 2
    assert res["oom_thrown"] == 1


def test_pool_small_path():
    run("scenario", "small")


def test_pool_forget_stream():
    run("scenario", "forget")


def test_pool_threads():
    res = run("threads", "1", "20000")
    assert res["threads"] == 4 and res["mallocs"] > 8  # (chunks were added while other threads ran)


@pytest.mark.parametrize("kind", ["arena", "small"])
def test_pool_double_free_aborts(kind):
    out = subprocess.run([BIN, "doublefree", kind], capture_output=True, text=True, timeout=60)
    assert out.returncode == -signal.SIGABRT, (out.returncode, out.stdout, out.stderr)
    assert json.loads(out.stdout.strip().splitlines()[-1]) == {"mode": "doublefree", "freed_once": True}
    assert "DevicePool: free of" in out.stderr and "double free?" in out.stderr

"""Hardware-queue placement on the GPU (engine.cpp place_streams, rtp_debug_stream_queues): with batches of 2 and seven frames in flight on
the runtime's default four hardware queues, the four busy contexts' conv streams sit on four different queues, every chain stream shares
its own context's queue, the spare context is never opened by an in-order caller, and the joints do not depend on any of it.

Every leg is a fresh child process (tools/hwq_map.py, net 160 x 96): the HIP runtime reads GPU_MAX_HW_QUEUES once per process."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "hwq_map.py")
APART, SHARED = 1.35, 1.65     # pair / single: below = side by side, above = one hardware queue, between = inconclusive
_legs = {}


def _leg(queues, exec_mode, frames, reps):
    """one child: the measured map (reps pair timings per pair, median), `frames` frames in bench.py's loop order, the opened-context counters"""
    key = (queues, exec_mode, frames, reps)
    if key not in _legs:
        env = {k: v for k, v in os.environ.items() if not k.startswith("RTP_")}
        env["GPU_MAX_HW_QUEUES"] = str(queues)
        if exec_mode == "eager":
            env["RTP_EXEC"] = "eager"
        out = subprocess.run([sys.executable, TOOL, "2", "7", str(frames), str(reps)], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        _legs[key] = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    return _legs[key]


def _check_map(leg, chains):
    owner = [tuple(o) for o in leg["owner"]]
    ratio = leg["ratio"]
    idx = {o: k for k, o in enumerate(owner)}
    convs = [idx[(c, 0)] for c in range(4)]
    for i, a in enumerate(convs):                       # the busy contexts' conv streams: pairwise side by side
        for b in convs[:i]:
            assert ratio[a][b] < APART, (owner[a], owner[b], ratio[a][b])
    assert ((4, 0) in idx) and {o[0] for o in owner} == {-1, 0, 1, 2, 3, 4}      # the spare context exists; -1 = the legacy stream
    if not chains:
        assert all(f == 0 for _, f in owner)            # one stream per context: every chain runs on its context's conv stream
        return
    for c in range(4):
        k = idx[(c, 1)]
        assert ratio[k][convs[c]] > SHARED, (owner[k], ratio[k][convs[c]])          # a chain waits behind its OWN context's stack only
        for c2 in range(4):
            if c2 != c:
                assert ratio[k][convs[c2]] < APART, (owner[k], owner[convs[c2]], ratio[k][convs[c2]])
                assert ratio[k][idx[(c2, 1)]] < APART, (owner[k], (c2, 1), ratio[k][idx[(c2, 1)]])


@pytest.mark.gpu
def test_busy_contexts_own_their_queues_on_four_queues():
    leg = _leg(4, "graph", 40, 5)
    assert len(leg["owner"]) == 11                      # per_frame_chains: a conv stream and a chain stream per context, and the legacy stream
    _check_map(leg, chains=True)


@pytest.mark.gpu
def test_one_stream_per_context_on_eight_queues():
    leg = _leg(8, "graph", 40, 5)
    assert len(leg["owner"]) == 6                       # five contexts and the legacy stream
    _check_map(leg, chains=False)
    ratio = leg["ratio"]
    assert all(ratio[4][b] < APART for b in range(4))   # enough queues: the spare context has one too


@pytest.mark.gpu
@pytest.mark.parametrize("queues", [4, 8])
def test_the_spare_context_is_never_opened_in_bench_order(queues):
    leg = _leg(queues, "graph", 40, 5)
    assert leg["opens"] == [5, 5, 5, 5, 0]              # 40 frames = 20 batches over the four busy contexts


@pytest.mark.gpu
@pytest.mark.parametrize("exec_mode", ["graph", "eager"])
def test_joints_do_not_depend_on_the_queue_count(exec_mode):
    """23 frames (full batches and a trailing partial one): the same hash on four queues (placed streams) and on eight (one stream per context)"""
    four, eight = _leg(4, exec_mode, 23, 0), _leg(8, exec_mode, 23, 0)
    assert len(four["hash"]) == 24 and four["hash"] == eight["hash"]

"""Hardware-queue placement, the host side (plan.cpp plan_busy_contexts / plan_queue_placement / plan_pick_queue_groups, describe_plan's
`streams` line): which contexts an in-order caller ever opens, when the engine places the busy contexts' streams on queues of their own,
and how it reads the measured "these two streams share a queue" map.  No GPU."""
import ctypes as C

import numpy as np

import caffe_rtpose_amd as r
from caffe_rtpose_amd import _lib

lib = _lib.lib


def _rules(F, B, Q=4, pad=0):
    out = (C.c_int * 4)()
    assert lib.rtp_internal_stream_rules(F, B, Q, pad, out) == 0
    return dict(contexts=out[0], busy=out[1], one_per_context=bool(out[2]), placement=bool(out[3]))


def _ceil(a, b):
    return -(-a // b)


def test_busy_contexts_match_the_closed_form():
    """min(plan_contexts(F, B), ceil((F + B - 1) / B)) for F = 1..16, B = 1..5; the flagship shape (7 in flight, batches of 2) keeps four
    contexts busy, eight in flight need all five."""
    for F in range(1, 17):
        for B in range(1, 6):
            contexts = _ceil(F, B) + (1 if B > 1 else 0)
            got = _rules(F, B)
            assert got["contexts"] == contexts, (F, B)
            assert got["busy"] == min(contexts, _ceil(F + B - 1, B)), (F, B)
    assert _rules(7, 2)["busy"] == 4 and _rules(7, 2)["contexts"] == 5
    assert _rules(8, 2)["busy"] == 5


def _simulate_open_slot(F, B, nframes):
    """engine.cpp open_slot / commit_slot / collect_impl on the host, driven in bench.py's order (fill the pipeline, collect one): returns how
    often every context was opened"""
    nctx = _ceil(F, B) + (1 if B > 1 else 0)
    filled, launched = [0] * nctx, [False] * nctx
    busy = [[False] * B for _ in range(nctx)]
    opens = [0] * nctx
    fifo = []
    open_ctx = -1
    sub = col = 0
    while col < nframes:
        while sub < nframes and len(fifo) < F:
            if open_ctx < 0:                                  # open_slot: the LOWEST idle context
                idle = [i for i in range(nctx) if not launched[i] and filled[i] == 0 and not any(busy[i])]
                assert idle, "all contexts busy"
                open_ctx = idle[0]
                opens[open_ctx] += 1
            ci, sj = open_ctx, filled[open_ctx]
            busy[ci][sj] = True                               # commit_slot
            filled[ci] = sj + 1
            fifo.append((ci, sj))
            if filled[ci] == B:
                launched[ci] = True
                open_ctx = -1
            sub += 1
        ci, sj = fifo.pop(0)                                  # collect_impl
        if not launched[ci]:                                  # the oldest frame sits in a partial batch: launch_open
            assert open_ctx == ci
            launched[ci] = True
            open_ctx = -1
        busy[ci][sj] = False
        if not any(busy[ci]):
            launched[ci] = False
            filled[ci] = 0
        col += 1
    return opens


def test_the_bench_loop_never_opens_a_context_beyond_the_busy_count():
    for F in range(1, 17):
        for B in range(1, 6):
            rules = _rules(F, B)
            opens = _simulate_open_slot(F, B, 12 * F + 1)
            assert len(opens) == rules["contexts"]
            assert all(n == 0 for n in opens[rules["busy"]:]), (F, B, opens)
            if F >= B:                                        # ... and the bound is tight: every busy context is opened
                assert all(n > 0 for n in opens[:rules["busy"]]), (F, B, opens)
    assert _simulate_open_slot(7, 2, 40) == [5, 5, 5, 5, 0]


def _streams_line(monkeypatch, queues, **kw):
    if queues is None:
        monkeypatch.delenv("GPU_MAX_HW_QUEUES", raising=False)
    else:
        monkeypatch.setenv("GPU_MAX_HW_QUEUES", str(queues))
    ln = [l for l in r.plan_summary(r.Config(**kw)).splitlines() if l.startswith("streams ")]
    assert len(ln) == 1
    return ln[0].split()


def test_streams_line_keeps_its_first_seven_words_and_names_the_busy_count(monkeypatch):
    w = _streams_line(monkeypatch, None, batch_frames=2, frames_in_flight=7)
    assert w == "streams contexts 5 hw_queues 4 arrangement per_frame_chains busy 4".split()
    w = _streams_line(monkeypatch, 8, batch_frames=2, frames_in_flight=7)
    assert w == "streams contexts 5 hw_queues 8 arrangement one_per_context busy 4".split()
    w = _streams_line(monkeypatch, 4, batch_frames=2, frames_in_flight=5)
    assert w == "streams contexts 4 hw_queues 4 arrangement one_per_context busy 3".split()
    w = _streams_line(monkeypatch, 4, batch_frames=2, frames_in_flight=8)
    assert w == "streams contexts 5 hw_queues 4 arrangement per_frame_chains busy 5".split()
    w = _streams_line(monkeypatch, 4, batch_frames=1, frames_in_flight=6)
    assert w == "streams contexts 6 hw_queues 4 arrangement one_per_context busy 6".split()


def test_placement_applies_where_the_busy_contexts_fit_the_queues_and_the_contexts_do_not():
    assert _rules(7, 2, 4) == dict(contexts=5, busy=4, one_per_context=False, placement=True)      # the flagship shape on the runtime's default
    assert not _rules(7, 2, 8)["placement"] and _rules(7, 2, 8)["one_per_context"]                 # enough queues: one stream per context, as before
    assert not _rules(7, 2, 5)["placement"] and _rules(7, 2, 5)["one_per_context"]
    assert not _rules(5, 2, 4)["placement"] and _rules(5, 2, 4)["one_per_context"]
    assert not _rules(8, 2, 4)["placement"] and not _rules(8, 2, 4)["one_per_context"]             # five busy contexts on four queues: round 5's streams
    assert not _rules(7, 2, 3)["placement"]
    assert not _rules(7, 2, 4, pad=2)["placement"]                                                 # unused pad streams in between: not placed
    for F in range(1, 17):
        assert not _rules(F, 1, 4)["placement"] and _rules(F, 1, 4)["one_per_context"]             # batches of 1 keep what they have
        for B in range(1, 6):
            for Q in (1, 2, 4, 5, 8):
                got = _rules(F, B, Q)
                if got["placement"]:
                    assert got["busy"] <= Q < got["contexts"] and not got["one_per_context"]


def _pick(queue_of, busy, per, unknown=(), flip=()):
    """queue_of: the queue of every candidate stream -> the share map the probe would measure -> the chosen candidates, or None"""
    n = len(queue_of)
    share = np.array([[1 if queue_of[a] == queue_of[b] else 0 for b in range(n)] for a in range(n)], np.int32)
    for a, b in unknown:
        share[a, b] = share[b, a] = -1
    for a, b in flip:
        share[a, b] = share[b, a] = 1 - share[a, b]
    pick = (C.c_int * (busy * per))(*([-1] * (busy * per)))
    rc = lib.rtp_internal_pick_queue_groups(share.ctypes.data_as(C.POINTER(C.c_int)), n, busy, per, pick)
    assert rc in (0, 1)
    return list(pick) if rc else None


def test_pick_queue_groups_reads_the_measured_map():
    # what the runtime does on four queues when its legacy stream already sits on queue 0 (profiles/hwq_four_queues.txt): 1 2 3 3 2 1 0 3 2 1 0
    measured = [1, 2, 3, 3, 2, 1, 0, 3, 2, 1, 0]
    got = _pick(measured, 4, 2)
    assert got == [0, 5, 1, 4, 2, 3, 6, 10]
    groups = [got[i:i + 2] for i in range(0, 8, 2)]
    assert all(measured[a] == measured[b] for a, b in groups) and len({measured[g[0]] for g in groups}) == 4
    assert _pick(measured[:10], 4, 2) is None                   # queue 0 has one candidate only: keep creating
    assert _pick(measured[:8], 4, 2) is None
    assert _pick(measured[:8], 3, 2) == [0, 5, 1, 4, 2, 3]
    assert _pick([0, 1, 2, 3, 3, 2, 1, 0], 4, 2) == [0, 7, 1, 6, 2, 5, 3, 4]      # no legacy stream: eight candidates suffice
    assert _pick([0, 0, 0, 0, 0, 0, 0, 0], 4, 2) is None        # everything on one queue
    assert _pick([0, 1, 2, 3], 4, 1) == [0, 1, 2, 3]
    # a pair the probe could not classify, or a map that is no equivalence relation (a mis-measurement): no placement
    assert _pick(measured, 4, 2, unknown=[(7, 2)]) is None
    assert _pick(measured, 4, 2, flip=[(5, 1)]) is None
    assert _pick(measured, 4, 2, flip=[(10, 6)]) is None


def test_the_queue_tap_is_exported_and_refuses_a_null_engine():
    assert hasattr(lib, "rtp_debug_stream_queues") and "rtp_debug_stream_queues" in _lib.SIGNATURES
    assert hasattr(r.Engine, "stream_queues")
    assert lib.rtp_debug_stream_queues(None, 0, None, None, 0, None, 0) == r.RTP_EINVAL

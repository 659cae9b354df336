"""CPU tests of the five native predictor entries (ga3c_pq_serve*, include/ga3c_host.h), entry by entry and
GA3C_RESPONDER mode by mode: what the engine's callbacks are given, who is answered when, what the counters count, and
that nothing is held when a call returns -- on a failing engine too.  The engine is stood in for by ctypes callbacks, as in
test_host_plumbing.py; every batch is queued before the slice starts, so the batching is exact."""
import ctypes as C

import numpy as np
import pytest

EINVAL, ECLOSED = -1, -4
A = 6

ROWS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.POINTER(C.c_float),
                      C.POINTER(C.c_float), C.POINTER(C.c_float))
BEGIN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.POINTER(C.c_int32))
BEGIN_CACHED_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                              C.c_int32, C.c_int32, C.POINTER(C.c_int32))
END_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float))
FRAMES_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_int32,
                        C.POINTER(C.c_float), C.POINTER(C.c_float))
FRAMES_BEGIN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                              C.c_int32, C.POINTER(C.c_int32))
FRAMES_END_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(C.c_float),
                            C.POINTER(C.c_float))


@pytest.fixture(scope="module")
def mods():
    import ga3c_amd  # noqa: F401
    import _native
    import Transport
    return _native, Transport


def addr(fn):
    return C.cast(fn, C.c_void_p).value


def set_mode(monkeypatch, mode):
    monkeypatch.delenv("GA3C_PIPELINE_MIN_QUEUED", raising=False)
    monkeypatch.delenv("GA3C_RESPONDER_SPIN_US", raising=False)
    if mode is None:
        monkeypatch.delenv("GA3C_RESPONDER", raising=False)
    else:
        monkeypatch.setenv("GA3C_RESPONDER", mode)


def idle(t, n):
    return [a for a in range(n) if t.agent_idle(a)]


def fill(p, v, i, agent, predict=True):
    """The answer of row i: the agent's own id in every probability, 100 + id as the value."""
    v[i] = 100.0 + agent
    for a in range(A):
        p[i * A + a] = float(agent) if predict else -1.0


def offset_of(t, agent):
    return int(t.state_offsets(np.array([agent], np.uint32))[0])


@pytest.mark.parametrize("mode", [None, "0", "1", "2", "3"])
def test_frames_loop_names_rows_routes_answers_and_counts_predictions(mods, monkeypatch, mode):
    """ga3c_pq_serve_frames, the default loop of the device front-end: 18 requests queued, batches of 8, 8 and 2 (under
    GA3C_RESPONDER = 2 the loop and its helper share the batches of 8).  The callback gets offset, agent and flags of every
    row; `served` counts predictions; without a helper every earlier batch is answered when the next callback runs, with
    one all but the last are; when the call returns everyone has their own answer."""
    nat, tp = mods
    set_mode(monkeypatch, mode)
    n = 18
    flags_of = {a: 0 for a in range(n)}
    flags_of.update({1: tp.REQ_RESET, 3: tp.REQ_RESET | tp.REQ_NO_PREDICT, 4: tp.REQ_NO_PREDICT, 12: tp.REQ_NO_PREDICT,
                     17: tp.REQ_RESET})
    t = tp.Transport.create(tp.unique_name("t_sl_fr"), n, A, 64, 4, 6)
    log = []

    @FRAMES_FN
    def serve(net, offsets, agents, flags, cnt, p, v):
        log.append(([(int(agents[i]), int(flags[i]), int(offsets[i])) for i in range(cnt)], len(idle(t, n))))
        for i in range(cnt):
            fill(p, v, i, int(agents[i]), not flags[i] & tp.REQ_NO_PREDICT)
        return 0

    try:
        for a in range(n):
            assert t.submit(a, flags_of[a]) == 0
        st = nat.ServeStats()
        assert t.serve_frames(addr(serve), None, 8, 30, st) == 0
        assert [[ag for ag, _, _ in rows] for rows, _ in log] == [list(range(0, 8)), list(range(8, 16)), [16, 17]]
        for rows, _ in log:
            assert all(fl == flags_of[ag] and off == offset_of(t, ag) for ag, fl, off in rows)
        assert (st.batches, st.served, st.largest_batch) == (3, n - 3, 8)
        done = 0
        for k, (rows, answered) in enumerate(log):
            if mode in ("1", "2"):
                assert done - (len(log[k - 1][0]) if k else 0) <= answered <= done, (k, answered)
            else:
                assert answered == done, (k, answered)
            done += len(rows)
        assert idle(t, n) == list(range(n))                  # nothing is held, and the helper has finished
        for a in range(n):
            rc, p, v = t.wait(a, 100)
            assert rc == 0 and v == 100.0 + a
            assert p.tolist() == [-1.0 if flags_of[a] & tp.REQ_NO_PREDICT else float(a)] * A
        assert st.ns_pop > 0 and st.ns_predict > 0 and st.ns_respond > 0
    finally:
        t.shutdown()
        t.close()


def frames_halves(t, tp, log, more, n_agents, fail_begin_at=None, fail_end_at=None):
    """`begin` / `end` callbacks of the frames loop that log (kind, agents, idle agents); calls["bad"] counts what `end` was
    given wrongly (an assertion inside a ctypes callback would be swallowed)."""
    held, calls = {}, {"begin": 0, "end": 0, "bad": 0}

    @FRAMES_BEGIN_FN
    def begin(net, offsets, agents, flags, cnt, ticket):
        calls["begin"] += 1
        while more:
            t.submit(more.pop(0))
        rows = [(int(agents[i]), int(flags[i])) for i in range(cnt)]
        log.append(("begin", [ag for ag, _ in rows], idle(t, n_agents)))
        if calls["begin"] == fail_begin_at:
            return -2
        ticket[0] = 40 + calls["begin"]
        held[ticket[0]] = rows
        return 0

    @FRAMES_END_FN
    def end(net, ticket, flags, cnt, p, v):
        calls["end"] += 1
        rows = held.pop(ticket, [])
        if cnt != len(rows) or [int(flags[i]) for i in range(cnt)] != [fl for _, fl in rows]:
            calls["bad"] += 1
        log.append(("end", [ag for ag, _ in rows], idle(t, n_agents)))
        if calls["end"] == fail_end_at:
            return -3
        for i, (ag, fl) in enumerate(rows):
            fill(p, v, i, ag, not fl & tp.REQ_NO_PREDICT)
        return 0

    return begin, end, calls


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_pipelined_frames_loop_has_no_helper_modes(mods, monkeypatch, mode):
    """ga3c_pq_serve_frames_pipelined under GA3C_RESPONDER = 1 and 2 behaves as under 0: with enough queued (two requests, a
    quarter of max_batch) the agent of batch k is still unanswered when batch k+1 is begun, and is answered before its end."""
    nat, tp = mods
    set_mode(monkeypatch, mode)
    t = tp.Transport.create(tp.unique_name("t_sl_fp"), 6, A, 64, 4, 6)
    log, more = [], [2, 4]
    begin, end, calls = frames_halves(t, tp, log, more, 6)
    try:
        st = nat.ServeStats()
        assert t.submit(1) == 0
        assert t.serve_frames_pipelined(addr(begin), addr(end), None, 8, 30, st) == 0
        assert [(k, ags) for k, ags, _ in log] == [("begin", [1]), ("end", [1]), ("begin", [2, 4]), ("end", [2, 4])]
        assert 1 not in log[2][2] and 1 in log[3][2]
        assert idle(t, 6) == list(range(6))
        for a in (1, 2, 4):
            rc, p, v = t.wait(a, 100)
            assert rc == 0 and v == 100.0 + a and p.tolist() == [float(a)] * A
        assert (st.batches, st.served, st.largest_batch) == (2, 3, 2) and calls["bad"] == 0
    finally:
        t.shutdown()
        t.close()


@pytest.mark.parametrize("mode", ["1", "2", "3"])
def test_cached_loop_names_rows_and_routes_answers_in_every_responder_mode(mods, monkeypatch, mode):
    """ga3c_pq_serve_pipelined_cached with a helper thread (1), a shared batch (2: ten requests, batches of 8 and 2) and
    answers at once (3): every row is named by offset, agent and request number, every agent gets its own answer."""
    nat, tp = mods
    set_mode(monkeypatch, mode)
    n = 10
    t = tp.Transport.create(tp.unique_name("t_sl_ca"), n, A, 64, 4, 6)
    seen, held = [], {}

    @BEGIN_CACHED_FN
    def begin(net, offsets, agents, seqs, batch, u8, ticket):
        rows = [(int(agents[i]), int(seqs[i]), int(offsets[i])) for i in range(batch)]
        seen.append((rows, len(idle(t, n))))
        ticket[0] = len(seen)
        held[ticket[0]] = rows
        return 0

    @END_FN
    def end(net, ticket, batch, p, v):
        for i, (ag, sq, _) in enumerate(held.pop(ticket)):
            fill(p, v, i, ag)
            v[i] = float(sq)
        return 0

    try:
        st = nat.ServeStats()
        for round_ in (1, 2):
            del seen[:]
            for a in range(n):
                assert t.submit(a) == 0
            assert t.serve_pipelined_cached(addr(begin), addr(end), None, 1, 8, 30, st) == 0
            assert [[ag for ag, _, _ in rows] for rows, _ in seen] == [list(range(8)), [8, 9]]
            assert all(sq == round_ and off == offset_of(t, ag) for rows, _ in seen for ag, sq, off in rows)
            if mode == "3":
                assert [cnt for _, cnt in seen] == [0, 8]
            else:
                assert seen[0][1] == 0 and 0 <= seen[1][1] <= 8
            assert idle(t, n) == list(range(n))
            for a in range(n):
                rc, p, v = t.wait(a, 100)
                assert rc == 0 and v == float(round_) and p.tolist() == [float(a)] * A
        assert (st.batches, st.served, st.largest_batch) == (4, 2 * n, 8)
    finally:
        t.shutdown()
        t.close()


def test_rows_loop_ignores_the_responder_mode(mods, monkeypatch):
    """ga3c_pq_serve under GA3C_RESPONDER = 1: at every callback all earlier batches are answered."""
    nat, tp = mods
    set_mode(monkeypatch, "1")
    t = tp.Transport.create(tp.unique_name("t_sl_ro"), 6, A, 64, 4, 6)
    log = []

    @ROWS_FN
    def predict(net, offsets, batch, u8, p, v, z):
        ags = [[offset_of(t, a) for a in range(6)].index(int(offsets[i])) for i in range(batch)]
        log.append((ags, len(idle(t, 6))))
        for i, ag in enumerate(ags):
            fill(p, v, i, ag)
        return 0

    try:
        for a in range(6):
            assert t.submit(a) == 0
        st = nat.ServeStats()
        assert t.serve(addr(predict), None, 1, 2, 30, st) == 0
        assert log == [([0, 1], 0), ([2, 3], 2), ([4, 5], 4)]
        assert (st.batches, st.served, st.largest_batch) == (3, 6, 2)
        for a in range(6):
            rc, p, v = t.wait(a, 100)
            assert rc == 0 and v == 100.0 + a and p.tolist() == [float(a)] * A
    finally:
        t.shutdown()
        t.close()


def test_frames_loop_reports_a_failing_engine_and_does_not_answer_its_batch(mods, monkeypatch):
    nat, tp = mods
    set_mode(monkeypatch, None)
    t = tp.Transport.create(tp.unique_name("t_sl_fe"), 6, A, 64, 4, 6)

    @FRAMES_FN
    def failing(net, offsets, agents, flags, cnt, p, v):
        return -2

    try:
        st = nat.ServeStats()
        assert t.serve_frames(addr(failing), None, 8, 20, st) == 0          # idle slice: plain return
        assert t.submit(1) == 0 and t.submit(2) == 0
        with pytest.raises(RuntimeError, match=r"\(-5\).*serve callback failed with -2 on a batch of 2"):
            t.serve_frames(addr(failing), None, 8, 20, st)
        assert not t.agent_idle(1) and not t.agent_idle(2)
        assert (st.batches, st.served) == (0, 0)
    finally:
        t.shutdown()
        t.close()


def test_pipelined_frames_loop_answers_what_it_holds_when_begin_fails(mods, monkeypatch):
    """Batches of one: agent 1 is held when agent 2's `begin` fails -- 1 is answered, 2 is not."""
    nat, tp = mods
    set_mode(monkeypatch, None)
    t = tp.Transport.create(tp.unique_name("t_sl_fb"), 6, A, 64, 4, 6)
    log = []
    begin, end, calls = frames_halves(t, tp, log, [], 6, fail_begin_at=2)
    try:
        st = nat.ServeStats()
        assert t.submit(1) == 0 and t.submit(2) == 0
        with pytest.raises(RuntimeError, match=r"\(-5\).*serve callback \(begin\) failed with -2 on a batch of 1"):
            t.serve_frames_pipelined(addr(begin), addr(end), None, 1, 200, st)
        assert [(k, ags) for k, ags, _ in log] == [("begin", [1]), ("end", [1]), ("begin", [2])]
        assert 1 not in log[2][2]                                           # (held over that begin)
        rc, p, v = t.wait(1, 100)
        assert rc == 0 and v == 101.0 and p.tolist() == [1.0] * A
        assert not t.agent_idle(2)
        assert (st.batches, st.served) == (1, 1) and calls["bad"] == 0
    finally:
        t.shutdown()
        t.close()


@pytest.mark.parametrize("entry", ["serve_pipelined", "serve_frames_pipelined"])
def test_pipelined_loops_answer_what_they_hold_when_end_fails(mods, monkeypatch, entry):
    """Batches of one, `end` fails on the second: GA3C_H_ECALLBACK, and agent 1, held over the second `begin`, is answered."""
    nat, tp = mods
    set_mode(monkeypatch, None)
    t = tp.Transport.create(tp.unique_name("t_sl_ee"), 6, A, 64, 4, 6)
    log, held, calls = [], {}, {"bad": 0}
    if entry == "serve_frames_pipelined":
        begin, end, calls = frames_halves(t, tp, log, [], 6, fail_end_at=2)
        word = "serve"

        def call(st):
            return t.serve_frames_pipelined(addr(begin), addr(end), None, 1, 200, st)
    else:
        word = "predict"

        @BEGIN_FN
        def begin(net, offsets, batch, u8, ticket):
            ags = [[offset_of(t, a) for a in range(6)].index(int(offsets[i])) for i in range(batch)]
            log.append(("begin", ags, idle(t, 6)))
            ticket[0] = len(log)
            held[ticket[0]] = ags
            return 0

        @END_FN
        def end(net, ticket, batch, p, v):
            ags = held.pop(ticket)
            log.append(("end", ags, idle(t, 6)))
            if sum(1 for k in log if k[0] == "end") == 2:
                return -3
            for i, ag in enumerate(ags):
                fill(p, v, i, ag)
            return 0

        def call(st):
            return t.serve_pipelined(addr(begin), addr(end), None, 1, 1, 200, st)

    try:
        st = nat.ServeStats()
        assert t.submit(1) == 0 and t.submit(2) == 0
        with pytest.raises(RuntimeError, match=r"\(-5\).*%s callback \(end\) failed with -3 on a batch of 1" % word):
            call(st)
        assert [(k, ags) for k, ags, _ in log] == [("begin", [1]), ("end", [1]), ("begin", [2]), ("end", [2])]
        assert 1 not in log[2][2] and 1 in log[3][2]
        rc, p, v = t.wait(1, 100)
        assert rc == 0 and v == 101.0 and p.tolist() == [1.0] * A
        assert not t.agent_idle(2)
        assert (st.batches, st.served) == (1, 1) and calls["bad"] == 0
    finally:
        t.shutdown()
        t.close()


def entries(nat, t):
    """name -> (callback slots, call(callbacks, max_batch, slice_ms) -> return code) for the five entries, unchecked."""
    lib, st = nat.host_lib(), nat.ServeStats()
    sp = C.addressof(st)
    return st, {
        "ga3c_pq_serve": (1, lambda cb, mb, ms: lib.ga3c_pq_serve(t._h, cb[0], None, 1, mb, ms, sp)),
        "ga3c_pq_serve_pipelined": (2, lambda cb, mb, ms: lib.ga3c_pq_serve_pipelined(t._h, cb[0], cb[1], None, 1, mb, ms, sp)),
        "ga3c_pq_serve_pipelined_cached": (2, lambda cb, mb, ms: lib.ga3c_pq_serve_pipelined_cached(t._h, cb[0], cb[1], None, 1, mb, ms, sp)),
        "ga3c_pq_serve_frames": (1, lambda cb, mb, ms: lib.ga3c_pq_serve_frames(t._h, cb[0], None, mb, ms, sp)),
        "ga3c_pq_serve_frames_pipelined": (2, lambda cb, mb, ms: lib.ga3c_pq_serve_frames_pipelined(t._h, cb[0], cb[1], None, mb, ms, sp)),
    }


def test_every_entry_refuses_bad_arguments_and_reports_a_closed_segment(mods, monkeypatch):
    nat, tp = mods
    set_mode(monkeypatch, None)
    t = tp.Transport.create(tp.unique_name("t_sl_ba"), 6, A, 64, 4, 6)

    @C.CFUNCTYPE(C.c_int)
    def never():
        raise AssertionError("the callback of a refused or closed call ran")

    try:
        st, table = entries(nat, t)
        assert t.submit(1) == 0                                              # a request is queued: a call that ran would use it
        for name, (slots, call) in table.items():
            good = [addr(never)] * slots
            for k in range(slots):
                assert call(good[:k] + [None] + good[k + 1:], 8, 20) == EINVAL, name
            assert call(good, 0, 20) == EINVAL, name
            assert call(good, 8, 0) == EINVAL, name
            assert lib_null_stats(nat, t, name, good) == EINVAL, name
        assert not t.agent_idle(1) and st.batches == 0
        assert t.pop_batch(np.zeros(8, np.uint32), 0) == 1                   # (what is queued is still served after a shutdown)
        t.shutdown()
        for name, (slots, call) in table.items():
            assert call([addr(never)] * slots, 8, 20) == ECLOSED, name
        assert st.batches == 0
    finally:
        t.close()


def lib_null_stats(nat, t, name, cb):
    fn = getattr(nat.host_lib(), name)
    if name in ("ga3c_pq_serve",):
        return fn(t._h, cb[0], None, 1, 8, 20, None)
    if name == "ga3c_pq_serve_frames":
        return fn(t._h, cb[0], None, 8, 20, None)
    if name == "ga3c_pq_serve_frames_pipelined":
        return fn(t._h, cb[0], cb[1], None, 8, 20, None)
    return fn(t._h, cb[0], cb[1], None, 1, 8, 20, None)

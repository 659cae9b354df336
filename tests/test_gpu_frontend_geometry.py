"""-m gpu: the device frame front-end (ga3c_amd/csrc/ga3c_frontend.hpp) at every frame geometry ga3c_net_frames_config admits,
and the plane history past one pass of gather_history_kernel's grid.  tests/frontend_cases.py builds the cases,
tests/test_frontend_cases_cpu.py asserts what makes them worth running, tests/README.md ("The frame front-end at the geometries
it admits") has the table.  Byte work against a bit-exact oracle: no tolerance anywhere."""
import os

import numpy as np
import pytest

import frame_frontend as ff
import frontend_cases as fc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = len(fc.KINDS)


@pytest.fixture(scope="module")
def net():
    import ga3c_amd  # noqa: F401
    from NetworkVP import Network
    n = Network("gpu:0", "test_frontend_geometry", 6, (84, 84, 4), max_batch=256, predict_lanes=1)
    yield n
    n.close()


@pytest.fixture(scope="module")
def other():
    import ga3c_amd  # noqa: F401
    from NetworkVP import Network
    n = Network("gpu:0", "test_frontend_geometry_ref", 6, (84, 84, 4), max_batch=256, predict_lanes=1)
    yield n
    n.close()


def _same_planes(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8
    diff = fc.first_difference(got, want)
    assert diff is None, "%s: %s" % (what, diff)


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("geom", fc.GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_planes_equal_the_oracle(net, geom, channels):
    H, W = geom
    assert isinstance(fc.admit(H, W, channels), fc.Facts)
    cs = fc.case(H, W)
    rgb = cs.rgb3 if channels == 3 else cs.rgb4
    net.frames_config(K + 5, H, W, channels)
    _same_planes(net.preprocess_frames(rgb), cs.planes, "%dx%dx%d" % (H, W, channels))
    # as many frames as the handle holds: the last workgroup's frame ends where the staging buffers end
    net.frames_config(K, H, W, channels)
    _same_planes(net.preprocess_frames(rgb), cs.planes, "%dx%dx%d, n == max_agents" % (H, W, channels))
    # a single frame, and the frames in another order: nothing depends on a frame's place in the launch
    _same_planes(net.preprocess_frames(rgb[K - 1]), cs.planes[K - 1:], "%dx%dx%d, one frame" % (H, W, channels))
    back = np.ascontiguousarray(rgb[::-1])
    _same_planes(net.preprocess_frames(back)[::-1], cs.planes, "%dx%dx%d, reversed" % (H, W, channels))


@pytest.mark.parametrize("geom", fc.QUEUE_GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_queues_and_history_at_a_geometry_that_is_not_ataris(net, geom):
    import Transport as tp
    H, W = geom
    frame_bytes = H * W * 3
    rng = np.random.default_rng(H + W)
    n_agents, steps, hist = 5, 11, 8
    cs = fc.case(H, W)
    slot_bytes = (frame_bytes + 4095) // 4096 * 4096
    t = tp.Transport.create(tp.unique_name("t_geo"), 8, 6, slot_bytes, 2, 6)
    try:
        net.frames_config(8, H, W, 3, history=hist)
        net.register_transport(t)
        ids = np.array([6, 2, 0, 7, 3], np.int32)                    # queue rows are not the batch rows
        queues = [ff.FrameQueue() for _ in range(n_agents)]
        states = {}
        for step in range(steps):
            # uniform frames and the case's own, in an order that changes from push to push
            rgb = rng.integers(0, 256, size=(n_agents, H, W, 3), dtype=np.uint8)
            pick = rng.permutation(K)[:2]
            rgb[step % n_agents], rgb[(step + 2) % n_agents] = cs.rgb3[pick[0]], cs.rgb3[pick[1]]
            reset = np.zeros(n_agents, np.uint8)
            if step == 0:
                reset[:] = 1
            if step == 5:
                reset[1] = 1                                          # one episode ends: its queue starts over
            if step % 2:                                              # odd steps: frames handed over in the transport's slots
                for k, a in enumerate(ids):
                    t.state_view(a)[:frame_bytes] = rgb[k].reshape(-1)
                seq = net.push_frame_offsets(t.state_offsets(ids.astype(np.uint32)), ids, reset)
            else:
                seq = net.push_frames(rgb, ids, reset)
            assert seq.tolist() == [step] * n_agents
            for k in range(n_agents):
                if reset[k]:
                    queues[k].clear()
                queues[k].push(ff.preprocess_u8(rgb[k]))
                state, depth = net.frame_state(ids[k])
                want = queues[k].state_u8()
                assert depth == len(queues[k].q) and (state is None) == (want is None), (step, k)
                if want is not None:
                    assert np.array_equal(state, want), "push %d, agent %d" % (step, ids[k])
                    states[(int(ids[k]), step)] = want
        x = np.stack([q.state_u8() for q in queues])
        p, v = net.predict_frames(ids)
        p2, v2 = net.predict_p_and_v(x)                               # the same bytes through the host-buffer path
        assert np.array_equal(p, p2) and np.array_equal(v, v2)
        live = [(a, s) for (a, s) in states if steps - (s - 3) <= hist]
        assert len(live) == 4 * 5 + 3 and any(s % hist < 3 for _, s in live)          # rows whose planes wrap the ring
        xs = np.stack([states[k] for k in live])
        y = rng.uniform(-1, 1, len(live))
        act = np.eye(6, dtype=np.float32)[rng.integers(0, 6, len(live))]
        ev_frames = net.evaluate(None, y, act, frames=([a for a, _ in live], [s for _, s in live]))
        ev_states = net.evaluate(xs, y, act)
        for name, got, want in zip(("losses", "d1", "v", "p"), ev_frames, ev_states):
            assert np.array_equal(got, want), name
    finally:
        net.unregister_transport()
        t.shutdown()
        t.close()


def test_refusals_name_their_rule_and_leave_the_handle_usable(net):
    small = fc.case(12, 7)
    for H, W, C, rule in fc.REFUSED:
        r = fc.admit(H, W, C)
        assert r.rule == rule
        net.frames_config(4, 12, 7, 3)
        with pytest.raises(RuntimeError, match=r.text):
            net.frames_config(4, H, W, C)
        if rule in ("channels", "planes"):                  # refused before anything is touched: the geometry in place stays
            _same_planes(net.preprocess_frames(small.rgb3[:4]), small.planes[:4], "12x7 after refusing %dx%dx%d" % (H, W, C))
        else:                                               # refused after the old geometry was let go: none is configured
            with pytest.raises(RuntimeError, match="frames_config first"):
                net.frame_state(0)
    cs = fc.case(210, 160)
    net.frames_config(4, 210, 160, 3)
    seq = net.push_frames(cs.rgb3[:1], np.array([2], np.int32), np.array([1], np.uint8))
    assert seq.tolist() == [0] and net.frame_state(2)[1] == 1
    _same_planes(net.preprocess_frames(cs.rgb3[:4]), cs.planes[:4], "210x160 after the refusals")


def test_one_handle_through_every_geometry(net):
    """Large, small, large: every frames_config re-lays the tables, the staging buffers and the LDS plan."""
    for H, W in fc.order_large_small_large():
        cs = fc.case(H, W)
        C = 4 if (H + W) % 2 else 3
        net.frames_config(3, H, W, C)
        rgb = (cs.rgb3 if C == 3 else cs.rgb4)[[0, 3, 7]]
        _same_planes(net.preprocess_frames(np.ascontiguousarray(rgb)), cs.planes[[0, 3, 7]], "%dx%dx%d in turn" % (H, W, C))
    g = np.load(os.path.join(ROOT, "tests", "golden", "frontend.npz"))
    names = [k[4:] for k in g.files if k.startswith("rgb_")]
    assert names
    for name in names:
        rgb, plane = g["rgb_" + name], g["plane_" + name]
        net.frames_config(4, *rgb.shape)
        assert np.array_equal(net.preprocess_frames(rgb)[0], plane), name


# ---------------------------------------------------------------- the plane history past one pass of the grid
@pytest.fixture(scope="module")
def ring(other):
    """A handle of its own (no other test re-lays its frames): 16 agents x 19 pushes of ready-made planes into a history of
    16, 13 live states each.  It and `other` at the same weights, `ms` at one.  -> (handle, theta)"""
    from NetworkVP import Network
    n = Network("gpu:0", "test_frontend_geometry_ring", 6, (84, 84, 4), max_batch=256, predict_lanes=1)
    try:
        theta = n.get_arena(0)
        for m in (n, other):
            m.set_arena(0, theta)
            m.set_arena(1, np.ones_like(theta))
            m.learning_rate, m.beta = 3e-4, 0.01
        n.frames_config(fc.HIST_AGENTS, 84, 84, 1, history=fc.HIST_DEPTH)
        planes = fc.history_planes()
        ids = np.arange(fc.HIST_AGENTS, dtype=np.int32)[::-1].copy()              # batch row k is agent 15 - k
        for step in range(fc.HIST_PUSHES):
            reset = np.full(fc.HIST_AGENTS, 1 if step == 0 else 0, np.uint8)
            seq = n.push_frames(np.ascontiguousarray(planes[step][ids]), ids, reset)
            assert seq.tolist() == [step] * fc.HIST_AGENTS
        for a in (0, 9, 15):
            state, depth = n.frame_state(a)
            assert depth == 4 and np.array_equal(state, fc.history_state(a, fc.HIST_PUSHES - 1))
        yield n, theta
    finally:
        n.close()


def _rows(B):
    names = fc.history_batch(B)
    rng = np.random.default_rng(900 + B)
    x = np.stack([fc.history_state(a, s) for a, s in names])
    y = rng.uniform(-1, 1, B)
    act = np.eye(6, dtype=np.float32)[rng.integers(0, 6, B)]
    return names, [a for a, _ in names], [s for _, s in names], x, y, act


@pytest.mark.parametrize("B", fc.HIST_SIZES)
def test_rows_from_the_history_past_one_pass_of_the_grid(other, ring, B):
    net, theta = ring
    names, agents, seqs, x, y, act = _rows(B)
    want = other.evaluate(x, y, act)
    # a row fetched from another name's planes must not be able to hide: the d1 rows of different names differ
    d1 = want[1]
    assert len(np.unique(d1, axis=0)) == len(set(names)) and d1.any(axis=1).all()
    got = net.evaluate(None, y, act, frames=(agents, seqs))
    for name, i in (("d1", 1), ("v", 2), ("p", 3)):                       # row by row first: a failure names its rows
        bad = np.nonzero((got[i] != want[i]).reshape(B, -1).any(axis=1))[0]
        assert bad.size == 0, "%s differs in %d of %d rows, first rows %s = names %s" % (
            name, bad.size, B, bad[:6].tolist(), [names[r] for r in bad[:6]])
    assert np.array_equal(got[0], want[0]), "losses"
    assert np.array_equal(net.get_arena(0), theta)                        # nothing trained


def test_train_rows_from_the_history_past_the_launch_argument(other, ring):
    """193 rows, their names read from the pinned arrays.  Both handles start from the fixture's weights and are put back."""
    net, theta = ring
    B = fc.HIST_TRAIN_SIZE
    names, agents, seqs, x, y, act = _rows(B)
    for m in (net, other):
        m.set_arena(0, theta)
        m.set_arena(1, np.ones_like(theta))
    try:
        net.train_frames(agents, seqs, y, act)
        other.train(x, y, act, None, None, 0)
        assert not np.array_equal(net.get_arena(0), theta)
        assert np.array_equal(net.get_arena(0), other.get_arena(0))
        assert np.array_equal(net.get_arena(1), other.get_arena(1))
        assert np.array_equal(net.last_losses, other.last_losses)
    finally:
        for m in (net, other):
            m.set_arena(0, theta)
            m.set_arena(1, np.ones_like(theta))

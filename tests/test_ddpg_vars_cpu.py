"""The DDPG handle's variable table, its initial-value rule and the re-lay of an arena from one table to another
(ga3c_amd/csrc/ga3c_ddpg_vars.hpp) against numpy, without a GPU: tests/native/ddpg_vars_tool.cpp prints the table make_table
builds for a set of options and re-lays five synthetic arenas between two of them.  What is expected is written out here from
the rule as DESIGN.md 8v states it, not read from the header:

  table   the 26 base variables, then critic 2's twelve, then critic_popart/mu, /nu, then actor_soft/log_alpha; contiguous
          from 0 to the arena size; value and target copy are checkpoint members of every variable (arenas 0, 1), a trainable
          one also has its optimizer's two slots (arenas 2, 3) under Adam's names (the actor, log_alpha, the critics with
          GA3C_DDPG_CRITIC_ADAM) or RMSProp's
  rule    a moving variance and nu are 1 in arenas 0 and 1, log_alpha the given value there, a critic's trainable variable 1 in
          arena 2 unless the critic is on Adam, everything else 0
  relay   a variable keeps its elements where the old table has one of the same name and shape, else the rule's value

The relay cases run on the tool as built plainly and as built with -fsanitize=address,undefined (a stand-alone program)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H1, H2 = 400, 300
LOG_ALPHA = np.float32(-0.75)
NARENA = 5
ARENA_STRIDE = 1 << 19            # above every arena size here; element i of arena w holds 2 + i + w * 2^19, exact in f32

# kind -> (atoms, soft head, twin, pop, soft)
KINDS = {"plain": (1, False, False, False, False), "dist2": (2, False, False, False, False),
         "dist51": (51, False, False, False, False), "popart": (1, False, False, True, False),
         "twin": (1, False, True, False, False), "twinsoft": (1, True, True, False, True)}
COUNTS = {"plain": (26, 20), "dist2": (26, 20), "dist51": (26, 20), "popart": (28, 20), "twin": (38, 30), "twinsoft": (39, 31)}
SHAPES = [(3, 1), (7, 3)]
# every transition the ABI allows, create and destroy
PAIRS = [("plain", "twin"), ("twin", "twinsoft"), ("plain", "dist2"), ("plain", "dist51"), ("plain", "popart")]


def expected_table(S, A, kind, adam):
    """-> ([(name, shape, trainable, [(member, arena)], target name)], arena size), from the rule."""
    atoms, soft_head, twin, pop, soft = KINDS[kind]
    head = 2 * A if soft_head else A
    actor = [("fc1/W", (S, H1)), ("fc1/b", (H1,)), ("norm1/beta", (H1,)), ("norm1/gamma", (H1,)), ("fc2/W", (H1, H2)),
             ("fc2/b", (H2,)), ("norm2/beta", (H2,)), ("norm2/gamma", (H2,)), ("output/W", (H2, head)), ("output/b", (head,))]
    critic = [("fc1/W", (S, H1)), ("fc1/b", (H1,)), ("norm1/beta", (H1,)), ("norm1/gamma", (H1,)), ("fc2/W", (H1, H2)),
              ("fc2/b", (H2,)), ("norm2/W", (A, H2)), ("norm2/b", (H2,)), ("output/W", (H2, atoms)), ("output/b", (atoms,))]
    rows = [("actor_" + n, s, "Adam") for n, s in actor]
    rows += [("critic_" + n, s, "Adam" if adam else "RMSProp") for n, s in critic]
    rows += [("actor_norm1/moving_mean", (H1,), None), ("actor_norm1/moving_variance", (H1,), None),
             ("actor_norm2/moving_mean", (H2,), None), ("actor_norm2/moving_variance", (H2,), None),
             ("critic_norm1/moving_mean", (H1,), None), ("critic_norm1/moving_variance", (H1,), None)]
    if twin:
        rows += [("critic2_" + n, s, "Adam" if adam else "RMSProp") for n, s in critic]
        rows += [("critic2_norm1/moving_mean", (H1,), None), ("critic2_norm1/moving_variance", (H1,), None)]
    if pop:
        rows += [("critic_popart/mu", (1,), None), ("critic_popart/nu", (1,), None)]
    if soft:
        rows += [("actor_soft/log_alpha", (1,), "Adam")]
    table = []
    for name, shape, slots in rows:
        scope, rest = name.split("/", 1)
        target = scope + "_1/" + rest
        members = [(name + ":0", 0), (target + ":0", 1)]
        if slots:
            members += [("%s/%s:0" % (name, slots), 2), ("%s/%s_1:0" % (name, slots), 3)]
        table.append((name, shape, slots is not None, members, target))
    return table, sum(int(np.prod(s)) for _, s, _, _, _ in table)


def initial(name, trainable, arena, adam):
    """The rule's value of a new variable in `arena`."""
    if name.endswith("/moving_variance") or name == "critic_popart/nu":
        return np.float32(1.0 if arena <= 1 else 0.0)
    if name == "actor_soft/log_alpha":
        return LOG_ALPHA if arena <= 1 else np.float32(0.0)
    if name.startswith("critic") and trainable and arena == 2 and not adam:
        return np.float32(1.0)
    return np.float32(0.0)


def options(S, A, kind, adam):
    atoms, soft_head, twin, pop, soft = KINDS[kind]
    return [str(int(v)) for v in (S, A, atoms, 2 * A if soft_head else 0, twin, pop, soft, adam)]


def build(out, *flags):
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-o", out,
                           os.path.join(ROOT, "tests", "native", "ddpg_vars_tool.cpp")])
    return out


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("ddpg_vars")
    return {"plain": build(str(d / "ddpg_vars_tool")),
            "sanitized": build(str(d / "ddpg_vars_tool_san"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}


@pytest.mark.parametrize("adam", [False, True])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("S,A", SHAPES)
def test_the_table_is_the_rules(tools, S, A, kind, adam):
    want, n = expected_table(S, A, kind, adam)
    assert (len(want), sum(t for _, _, t, _, _ in want)) == COUNTS[kind]
    lines = subprocess.check_output([tools["plain"], "table"] + options(S, A, kind, adam), text=True).splitlines()
    assert lines[-1] == "n %d" % n and len(lines) == len(want) + 1
    off = 0
    for line, (name, shape, trainable, members, target) in zip(lines, want):
        got = line.split("\t")
        assert got[0] == name
        assert int(got[1]) == off, name                                   # contiguous ...
        assert int(got[2]) == int(np.prod(shape)), name
        assert tuple(int(x) for x in got[3].split(",")) == shape, name
        assert int(got[4]) == int(trainable), name
        assert [(m.rsplit("=", 1)[0], int(m.rsplit("=", 1)[1])) for m in got[5].split(",")] == members, name
        assert got[6] == target, name
        off += int(got[2])
    assert off == n                                                       # ... and ending at the arena size


def synthetic(n):
    return np.stack([np.float32(2 + w * ARENA_STRIDE) + np.arange(n, dtype=np.float32) for w in range(NARENA)])


def run_relay(tool, tmp_path, S, A, old, new, adam, arenas):
    src, dst = str(tmp_path / "in.f32"), str(tmp_path / "out.f32")
    arenas.astype(np.float32).tofile(src)
    run = subprocess.run([tool, "relay"] + options(S, A, old, adam) + options(S, A, new, adam) + [repr(float(LOG_ALPHA)), src, dst],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return np.fromfile(dst, np.float32).reshape(NARENA, -1)


def slices(table):
    """{name: (shape, offset, count, trainable)}"""
    out, off = {}, 0
    for name, shape, trainable, _, _ in table:
        count = int(np.prod(shape))
        out[name] = (shape, off, count, trainable)
        off += count
    return out


def check_relay(got, arenas, S, A, old, new, adam):
    """-> the names of the variables that kept their elements"""
    (t0, n0), (t1, n1) = expected_table(S, A, old, adam), expected_table(S, A, new, adam)
    assert arenas.shape == (NARENA, n0) and got.shape == (NARENA, n1)
    was, kept = slices(t0), []
    for name, (shape, off, count, trainable) in slices(t1).items():
        if name in was and was[name][0] == shape:
            kept.append(name)
            o0 = was[name][1]
            assert np.array_equal(got[:, off:off + count], arenas[:, o0:o0 + count]), name
        else:
            for w in range(NARENA):
                assert np.all(got[w, off:off + count] == initial(name, trainable, w, adam)), (name, w)
    return kept


@pytest.mark.parametrize("build_kind", ["plain", "sanitized"])
@pytest.mark.parametrize("adam", [False, True])
@pytest.mark.parametrize("pair", PAIRS, ids=["%s-%s" % p for p in PAIRS])
@pytest.mark.parametrize("S,A", SHAPES)
def test_relay_keeps_what_has_its_name_and_shape_and_starts_the_rest_by_the_rule(tools, tmp_path, S, A, pair, adam, build_kind):
    tool = tools[build_kind]
    old, new = pair
    n0 = expected_table(S, A, old, adam)[1]
    assert n0 < ARENA_STRIDE and expected_table(S, A, new, adam)[1] < ARENA_STRIDE
    arenas = synthetic(n0)
    # the create ...
    created = run_relay(tool, tmp_path, S, A, old, new, adam, arenas)
    kept = check_relay(created, arenas, S, A, old, new, adam)
    # ... the destroy on its own, from the option's synthetic arenas ...
    full = synthetic(created.shape[1])
    check_relay(run_relay(tool, tmp_path, S, A, new, old, adam, full), full, S, A, new, old, adam)
    # ... and the destroy after the create: the old values everywhere but in the variables whose shape changed on the way
    back = run_relay(tool, tmp_path, S, A, new, old, adam, created)
    table = expected_table(S, A, old, adam)[0]
    reshaped = [name for name in slices(table) if name not in kept]
    assert reshaped == {"dist2": ["critic_output/W", "critic_output/b"], "dist51": ["critic_output/W", "critic_output/b"],
                        "twinsoft": ["actor_output/W", "actor_output/b"]}.get(new, [])
    for name, (shape, off, count, trainable) in slices(table).items():
        for w in range(NARENA):
            want = np.full(count, initial(name, trainable, w, adam)) if name in reshaped else arenas[w, off:off + count]
            assert np.array_equal(back[w, off:off + count], want), (name, w)


@pytest.mark.parametrize("build_kind", ["plain", "sanitized"])
@pytest.mark.parametrize("adam", [False, True])
@pytest.mark.parametrize("kind", ["plain", "twinsoft", "popart"])
def test_a_new_handles_arenas_are_the_rules(tools, tmp_path, kind, adam, build_kind):
    """relay from an empty table, which is what ga3c_ddpg_create uploads: every variable at its initial value."""
    S, A = 7, 3
    dst = str(tmp_path / "fresh.f32")
    subprocess.check_call([tools[build_kind], "fresh"] + options(S, A, kind, adam) + [repr(float(LOG_ALPHA)), dst])
    table, n = expected_table(S, A, kind, adam)
    got = np.fromfile(dst, np.float32).reshape(NARENA, n)
    for name, (shape, off, count, trainable) in slices(table).items():
        for w in range(NARENA):
            assert np.all(got[w, off:off + count] == initial(name, trainable, w, adam)), (name, w)

"""The variable table and the checkpoint path every network handle shares (ga3c_amd/csrc/ga3c_vartable.hpp) against numpy,
without a GPU: tests/native/vartable_tool.cpp holds a small two-optimizer table (two trunk layers, a value head, a policy
head, members by the shared DUAL_RMSPROP rule) over seven synthetic arenas.  What pack_members writes is held to the rule as
DESIGN.md 8c / 8h state it, computed here; what unpack_members reads lands only where a member names it; a file with a
member missing, of another shape, of another type or without a step is refused with the arenas untouched."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the tool's table, in arena order; n elements per arena
SHAPES = [("fc1/w", (3, 4)), ("fc1/b", (4,)), ("fc2/w", (4, 3)), ("fc2/b", (3,)),
          ("head_v/w", (3, 1)), ("head_v/b", (1,)), ("head_p/w", (3, 2)), ("head_p/b", (2,))]
N = sum(int(np.prod(s)) for _, s in SHAPES)
NARENA = 7
SENTINEL = np.float32(-1.0)


def rule(name):
    """[(member, arena)] of one variable, in file order.  The value optimizer is created first: the trunk
    has its slots as /RMSProp (arena 4), _1 (5) and the policy optimizer's as _2 (1), _3 (2); each head has only its own
    optimizer's, as /RMSProp and _1."""
    if name.startswith("head_v/"):
        slots = [("/RMSProp:0", 4), ("/RMSProp_1:0", 5)]
    elif name.startswith("head_p/"):
        slots = [("/RMSProp:0", 1), ("/RMSProp_1:0", 2)]
    else:
        slots = [("/RMSProp:0", 4), ("/RMSProp_1:0", 5), ("/RMSProp_2:0", 1), ("/RMSProp_3:0", 2)]
    return [(name + ":0", 0)] + [(name + s, w) for s, w in slots]


def layout():
    """-> [(variable, shape, offset, count)]"""
    out, off = [], 0
    for name, shape in SHAPES:
        count = int(np.prod(shape))
        out.append((name, shape, off, count))
        off += count
    return out


def synthetic():
    """arena w, element i = i + w / 8 (exact in f32)"""
    return np.stack([np.arange(N, dtype=np.float32) + np.float32(w / 8) for w in range(NARENA)])


def expected_members(arenas):
    """{member: array} of a whole file over `arenas`, insertion order = file order (without the step)."""
    want = {}
    for name, shape, off, count in layout():
        for member, w in rule(name):
            want[member] = arenas[w, off:off + count].reshape(shape)
    return want


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vartable") / "vartable_tool")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "vartable_tool.cpp")])
    return exe


def read_back(tool, path, dump):
    """-> (exit status, stderr, step, arenas [7, N]) of `vartable_tool read`"""
    run = subprocess.run([tool, "read", path, dump], capture_output=True, text=True)
    raw = open(dump, "rb").read()
    assert len(raw) == 8 + 4 * NARENA * N
    return (run.returncode, run.stderr, int(np.frombuffer(raw[:8], np.int64)[0]),
            np.frombuffer(raw[8:], np.float32).reshape(NARENA, N))


def test_the_table_is_the_one_this_test_assumes_and_names_resolve_with_and_without_the_suffix(tool):
    for i, (name, _) in enumerate(SHAPES):
        for asked in (name, name + ":0"):
            assert int(subprocess.check_output([tool, "find", asked])) == i
    for asked in ("fc1", "fc1/w:1", "fc1/w/RMSProp:0", ":0", ""):
        assert int(subprocess.check_output([tool, "find", asked])) == -1


def test_pack_members_writes_the_rules_members_variable_major_with_each_variables_shape_and_slice(tool, tmp_path):
    path = str(tmp_path / "w.npz")
    step = 1234567890123
    subprocess.check_call([tool, "write", path, str(step)])
    want = expected_members(synthetic())
    with np.load(path, allow_pickle=False) as z:
        assert z.files == ["step"] + list(want)              # the set, and the order: step, then variable-major
        assert z["step"].dtype == np.int64 and z["step"].shape == () and int(z["step"]) == step
        for member, value in want.items():
            got = z[member]
            assert got.dtype == np.float32 and got.shape == value.shape, member
            assert np.array_equal(got, value), member
    assert len(want) == 4 * 5 + 4 * 3


def test_unpack_members_fills_what_members_name_and_leaves_the_rest(tool, tmp_path):
    path = str(tmp_path / "r.npz")
    rng = np.random.default_rng(11)
    values = rng.normal(size=(NARENA, N)).astype(np.float32)
    np.savez(path, step=np.int64(-5), **expected_members(values))
    rc, err, step, got = read_back(tool, path, str(tmp_path / "dump"))
    assert rc == 0, err
    assert step == -5
    named = np.zeros((NARENA, N), bool)
    for name, _, off, count in layout():
        for _, w in rule(name):
            named[w, off:off + count] = True
    assert named[0].all() and not named[3].any() and not named[6].any() and not named[1].all() and not named[4].all()
    assert np.array_equal(got[named], values[named])
    assert np.all(got[~named] == SENTINEL)


def refused(tool, tmp_path, members):
    path = str(tmp_path / "bad.npz")
    np.savez(path, **members)
    rc, err, step, got = read_back(tool, path, str(tmp_path / "dump"))
    assert rc == 1 and err.strip()
    assert step == -1 and got.tobytes() == np.full((NARENA, N), SENTINEL).tobytes()
    return err


def good_file():
    return dict(step=np.int64(9), **expected_members(synthetic()))


def test_a_file_with_a_member_missing_is_refused_untouched(tool, tmp_path):
    for gone in ("fc1/w:0", "fc2/b/RMSProp_3:0", "head_p/b/RMSProp_1:0"):
        members = good_file()
        del members[gone]
        assert gone in refused(tool, tmp_path, members)


def test_a_member_of_the_right_count_and_another_shape_is_refused_untouched(tool, tmp_path):
    for member, shape in (("fc2/w:0", (3, 4)), ("fc2/w/RMSProp_2:0", (12,)), ("head_v/b:0", ()), ("head_p/b/RMSProp:0", (2, 1))):
        members = good_file()
        members[member] = members[member].reshape(shape)
        assert member in refused(tool, tmp_path, members)


def test_a_member_as_f8_is_refused_untouched(tool, tmp_path):
    members = good_file()
    members["head_p/w:0"] = members["head_p/w:0"].astype(np.float64)
    assert "head_p/w:0" in refused(tool, tmp_path, members)


def test_a_file_without_a_step_or_with_another_steps_type_is_refused_untouched(tool, tmp_path):
    members = good_file()
    del members["step"]
    assert "step" in refused(tool, tmp_path, members)
    assert "step" in refused(tool, tmp_path, dict(good_file(), step=np.int32(9)))

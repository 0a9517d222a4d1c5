"""CPU tests of the self-collision check (wbcqp_check_collisions): the readers and the numpy statement of inria_wbc_amd/collision.py against a
literal transcription of the reference's four loops, the library's surface (symbols declared, exported, bound; without a handle the entry
points refuse -- the per-field refusals of a table need a slot with a model, hence a device: tests/test_gpu_collision.py), and the facade's YAML
reader on the collision file.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from inria_wbc_amd import model as mdl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "talos_collisions.yaml")


def random_table(m, n_spheres, n_members, seed, spread=0.1, dmin=0.05, dmax=0.3):
    """A sphere table on model m: random bodies, centres and float32 diameters; member numbers sorted, every member present when there are
    spheres enough.  (tests/test_gpu_collision.py draws its tables here too.)"""
    from inria_wbc_amd import collision
    rng = np.random.default_rng(seed)
    member = np.sort(np.concatenate([np.arange(min(n_members, n_spheres)), rng.integers(0, n_members, max(0, n_spheres - n_members))])).astype(np.int32)
    return collision.SphereTable(body=rng.integers(0, m.nbody, n_spheres).astype(np.int32), member=member,
                                 centre=(spread * rng.standard_normal((n_spheres, 3))).astype(np.float32).astype(np.float64),
                                 diameter=rng.uniform(dmin, dmax, n_spheres).astype(np.float32), member_names=["m%02d" % k for k in range(n_members)])


def four_loops(m, table, q):
    """collision_check.cpp:27-87 written out: spherical_members_ as a name-sorted map of (centre, float diameter) lists, then the four loops
    with the early return.  Also what the early return hides: every colliding unordered pair and the smallest clearance."""
    R, p = m.body_placements(q)
    members = {}
    for s in range(table.n_spheres):
        b = table.body[s]
        members.setdefault(table.member_names[table.member[s]], []).append((R[b] @ table.centre[s] + p[b], np.float32(table.diameter[s]), s))
    first, pairs, clearance = None, set(), np.inf
    for a in sorted(members):
        for b in sorted(members):
            if a != b:
                for i, (ca, da, sa) in enumerate(members[a]):
                    for j, (cb, db, sb) in enumerate(members[b]):
                        dist = float(np.linalg.norm(cb - ca))
                        thr = float(np.float32(db / np.float32(2)) + np.float32(da / np.float32(2)))
                        clearance = min(clearance, dist - thr)
                        if dist < thr:
                            if first is None:
                                first = ((a, i), (b, j), sa, sb)
                            pairs.add((min(sa, sb), max(sa, sb)))
    return first, pairs, clearance


def ordering_case():
    """One fixed body, members A (two spheres), B, C: A1 hits B0 and A0 hits C0.  The reference's loops reach member B before sphere A1's turn
    matters -- (A, B, 1, 0) comes before (A, C, 0, 0) -- although (0, 3) is the smaller pair of table indices."""
    from inria_wbc_amd import collision
    m = mdl.random_tree(91, 1, False)
    t = collision.SphereTable(body=np.zeros(4, np.int32), member=np.array([0, 0, 1, 2], np.int32),
                              centre=np.array([[0.0, 0, 0], [5.0, 0, 0], [5.125, 0, 0], [0.125, 0, 0]]), diameter=np.full(4, 0.2, np.float32),
                              member_names=["A", "B", "C"])
    return m, t, m.q0[None]


def test_sphere_table_of_the_talos_file():
    from inria_wbc_amd import collision
    m = mdl.talos_like()
    members = collision.load_members(FIXTURE)
    assert len(members) == 5 and sum(len(s) for links in members.values() for s in links.values()) == 116
    t = collision.sphere_table(m, FIXTURE)
    assert t.member_names == ["arm_left", "arm_right", "leg_left", "leg_right", "torso"]
    assert sorted(t.skipped) == ["gripper_left_base_link", "gripper_right_base_link"] and t.n_spheres == 112
    assert t.diameter.dtype == np.float32 and t.body.dtype == np.int32 and t.member.dtype == np.int32 and t.centre.dtype == np.float64
    assert (np.diff(t.member) >= 0).all() and np.bincount(t.member).tolist() == [12, 12, 31, 31, 26]
    # *_link names land on the *_joint bodies; frames the model holds go to their own body
    assert t.body[0] == m.joint_names.index("arm_left_1_joint") and t.body[24] == m.joint_names.index("leg_left_1_joint")
    torso = t.body[t.member == 4]
    assert torso[0] == m.joint_names.index("head_1_joint") and torso[2] == m.joint_names.index("torso_2_joint") and torso[-1] == 0  # base_link
    # numbers are the file's, read as float32: leg_left_3_link's second sphere, file order inside a member
    k = int(np.nonzero(t.member == 2)[0][0]) + 2 + 3 + 1
    assert np.array_equal(t.centre[k], np.array([0, 0.015, -0.1], np.float32).astype(np.float64)) and t.diameter[k] == np.float32(0.17)
    assert t.local_index()[k] == 6
    assert collision.sphere_table(m, collision.load_members(FIXTURE)).body.tolist() == t.body.tolist()  # a dict serves as well as a path
    out = collision.check(m, t, m.q0)
    assert out["centres"].shape == (1, 112, 3) and out["first_pair"].shape == (1, 2)


@pytest.mark.parametrize("n_members,n_spheres,seed,scale", [(2, 9, 8, 1.0), (3, 40, 12, 0.5), (16, 70, 2, 0.3)])  # (both outcomes occur with these)
def test_numpy_statement_against_the_four_loops(n_members, n_spheres, seed, scale):
    from inria_wbc_amd import collision
    m = mdl.random_tree(60 + seed, 24, seed != 2)
    t = random_table(m, n_spheres, n_members, 600 + seed, dmin=0.05 * scale, dmax=0.3 * scale)
    rng = np.random.default_rng(seed)
    q = np.stack([m.q0] * 12)
    q[:, (7 if m.floating_base else 0):] += 0.5 * rng.standard_normal((12, m.na))
    got = collision.check(m, t, q)
    seen = set()
    for k in range(12):
        first, pairs, clearance = four_loops(m, t, q[k])
        seen.add(first is not None)
        assert got["colliding"][k] == (first is not None) and got["n_pairs"][k] == len(pairs)
        assert abs(got["clearance"][k] - clearance) <= 1e-12
        if first is None:
            assert got["first_pair"][k].tolist() == [-1, -1] and collision.pair_names(t, got["first_pair"][k]) is None
        else:
            assert got["first_pair"][k].tolist() == [first[2], first[3]]
            assert collision.pair_names(t, got["first_pair"][k]) == (first[0], first[1])
    assert seen == {True, False}, "the states must show both outcomes"


def test_one_member_never_collides():
    from inria_wbc_amd import collision
    m = mdl.random_tree(65, 24, True)
    t = random_table(m, 30, 1, 650, spread=0.01)
    got = collision.check(m, t, m.q0)
    assert got["colliding"][0] == 0 and got["n_pairs"][0] == 0 and np.isposinf(got["clearance"][0]) and got["first_pair"][0].tolist() == [-1, -1]


def test_first_pair_follows_the_reference_loops_not_the_table_indices():
    from inria_wbc_amd import collision
    m, t, q = ordering_case()
    got = collision.check(m, t, q)
    first, pairs, _ = four_loops(m, t, q[0])
    assert pairs == {(1, 2), (0, 3)} and first[:2] == (("A", 1), ("B", 0))
    assert got["n_pairs"][0] == 2 and got["first_pair"][0].tolist() == [1, 2]
    assert collision.pair_names(t, got["first_pair"][0]) == (("A", 1), ("B", 0))


def test_readers_refuse():
    from inria_wbc_amd import collision
    m = mdl.talos_like()
    with pytest.raises(ValueError):
        collision.load_members({"members": {"a": {"base_link": [[0, 0, 0]]}}})  # a sphere of three numbers
    with pytest.raises(ValueError):
        collision.sphere_table(m, {"m%02d" % k: {"base_link": [[0, 0, 0, 0.1]]} for k in range(17)})
    with pytest.raises(ValueError):
        collision.sphere_table(m, {"a": {"base_link": [[0, 0, 0, 0.1]] * 257}})
    t = collision.sphere_table(m, {"a": {"no_such_link": [[0, 0, 0, 0.1]], "base_link": [[0, 0, 0, 0.1]]}})
    assert t.skipped == ["no_such_link"] and t.n_spheres == 1


def test_symbols_declared_exported_bound(built_lib):
    from inria_wbc_amd import capi
    hdr = open(os.path.join(ROOT, "include", "wbcqp.h")).read()
    declared = set(re.findall(r"\b(wbcqp_[a-z_]+)\s*\(", hdr))
    new = {"wbcqp_set_collision_spheres", "wbcqp_check_collisions", "wbcqp_check_collisions_host"}
    assert new <= declared and new <= set(capi.EXPORTS)
    assert re.search(r"#define\s+WBCQP_MAX_SPHERES\s+256\b", hdr) and re.search(r"#define\s+WBCQP_MAX_MEMBERS\s+16\b", hdr)
    assert "wbcqp_sphere_model" in hdr and "wbcqp_collisions" in hdr
    raw = ctypes.CDLL(built_lib)
    lib = capi.load_library()
    for sym in new:
        assert hasattr(raw, sym), sym
        assert getattr(lib, sym).argtypes, sym
    assert ctypes.sizeof(capi.CSphereModel) == 40 and ctypes.sizeof(capi.CCollisions) == 40
    assert [k for k, _ in capi.CSphereModel._fields_] == ["n_spheres", "body", "member", "centre", "diameter"]
    assert [k for k, _ in capi.CCollisions._fields_] == ["colliding", "first_pair", "n_pairs", "clearance", "centres"]
    assert raw.wbcqp_version() == 151
    for name in ("set_collision_spheres", "check_collisions", "check_collisions_host"):
        assert callable(getattr(capi.Handle, name))
    # without a handle every entry point refuses before it touches a device
    sm, out = capi.CSphereModel(0, None, None, None, None), capi.CCollisions()
    assert lib.wbcqp_set_collision_spheres(None, 0, ctypes.byref(sm)) == 1
    assert lib.wbcqp_check_collisions(None, 0, 1, None, ctypes.byref(out), None) == 1
    assert lib.wbcqp_check_collisions_host(None, 0, 1, None, ctypes.byref(out)) == 1


def test_facade_yaml_reader_takes_the_multi_line_flow_sequences(tmp_path):
    """The collision file continues its flow sequences over several lines; yaml_lite joins them while brackets are open."""
    src = tmp_path / "count.cpp"
    src.write_text('#include <inria_wbc/utils/yaml_lite.hpp>\n#include <iostream>\n'
                   'int main(int, char** argv) {\n'
                   '    auto members = inria_wbc::yaml::LoadFile(argv[1])["members"];\n'
                   '    size_t n = 0, links = 0;\n'
                   '    for (const auto& m : members)\n'
                   '        for (const auto& l : m.second) { ++links; for (const auto& s : l.second.as<std::vector<std::vector<float>>>()) n += s.size() == 4; }\n'
                   '    auto quoted = inria_wbc::yaml::Load("a: \\"x[0\\"\\nb: 2\\n");  // a bracket inside quotes opens nothing\n'
                   '    std::cout << members.size() << " " << links << " " << n << " " << quoted["a"].as<std::string>() << " " << quoted["b"].as<int>() << std::endl;\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "count"
    inc = os.path.join(ROOT, "inria_wbc_amd", "csrc", "host", "include")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", inc, str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe), FIXTURE], text=True).split() == ["5", "32", "116", "x[0", "2"]

"""The C ABI of the global voxel map (include/scl_engine.h "GLOBAL MAP") without a GPU: the calls, the struct and the test hook declared,
exported and bound with the declarations' types, the ABI version moved to 16, a NULL engine refused with nothing written, the header
still C99, and the host-only plan (scl_slam_amd/csrc/global_map_plan.hpp) through tests/cpp/global_map_plan_check -- a program of its
own under ASan + UBSan, built by the test -- against tests/global_map_cases.py.  (The technique of tests/test_pgo_abi.py.)"""
import os
import re
import subprocess
from ctypes import POINTER, byref, c_double, c_float, c_int, c_uint64, c_void_p

import numpy as np

import global_map_cases as gm
from scl_slam_amd import MapStats, load_library
from scl_slam_amd.engine import MAP_RECORD, ScanContextEngine, _bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scl_map_reset", "scl_map_set_keyframes", "scl_map_remove_keyframes", "scl_map_extract", "scl_map_stats", "scl_map_last_timing",
         "scl_selftest_map_capacity")
INVALID_ARG = -1
C_TYPES = {"scl_engine *": c_void_p, "int": c_int, "float": c_float, "uint64_t": c_uint64, "const int *": POINTER(c_int), "int *": POINTER(c_int),
           "const double *": POINTER(c_double), "double []": POINTER(c_double), "void *": c_void_p, "struct scl_map_stats *": POINTER(MapStats)}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scl_engine.h")).read(), flags=re.S)


def _declaration(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), flags=re.S)
    assert m, f"{name} is not declared in scl_engine.h"
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        array = re.search(r"\[\d*\]$", a)                                # `double ms[3]` is a pointer: listed as "double []"
        out.append(re.match(r"(.*?)(\w+)$", a[:array.start()] if array else a).group(1).strip() + (" []" if array else ""))
    return out


def test_declared_exported_and_typed():
    lib = load_library(); _bind(lib)
    assert lib.scl_abi_version() >= 16
    for name in NAMES:
        fn = getattr(lib, name)
        want = [C_TYPES[t] for t in _declaration(name)]
        assert fn.restype is c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert [len(_declaration(n)) for n in NAMES] == [2, 5, 4, 5, 2, 2, 2]
    for method in ("map_reset", "map_set_keyframes", "map_remove_keyframes", "map_extract", "map_stats", "map_last_timing", "selftest_map_capacity"):
        assert callable(getattr(ScanContextEngine, method))


def test_the_struct_and_the_record_mirror_the_header():
    body = re.search(r"struct scl_map_stats\s*\{(.*?)\}", _header(), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            t, name = decl.split(" ", 1)
            fields.append((name.strip(), {"uint64_t": c_uint64}[t]))
    assert fields == list(MapStats._fields_) and [f for f, _ in fields] == ["keyframes", "points_added", "points_skipped", "occupied_voxels",
                                                                            "capacity", "growths"]
    assert MAP_RECORD.itemsize == 16 and MAP_RECORD == gm.RECORD


def test_a_null_engine_is_refused_and_nothing_is_written():
    lib = load_library(); _bind(lib)
    ids = np.zeros(2, np.int32); poses = np.tile(gm.IDENTITY, 2)
    ip = lambda a: a.ctypes.data_as(POINTER(c_int)); dp = lambda a: a.ctypes.data_as(POINTER(c_double))
    out = np.full(4, 7, np.uint32); n = c_int(7); st = MapStats(); st.keyframes = 7; ms = np.full(3, 7.0)
    assert lib.scl_map_reset(None, 0.4) == INVALID_ARG
    assert lib.scl_map_set_keyframes(None, ip(ids), ip(ids), dp(poses), 2) == INVALID_ARG
    assert lib.scl_map_remove_keyframes(None, ip(ids), ip(ids), 2) == INVALID_ARG
    assert lib.scl_map_extract(None, None, out.ctypes.data_as(c_void_p), 1, byref(n)) == INVALID_ARG
    assert lib.scl_map_stats(None, byref(st)) == INVALID_ARG
    assert lib.scl_map_last_timing(None, dp(ms)) == INVALID_ARG
    assert lib.scl_selftest_map_capacity(None, 64) == INVALID_ARG
    assert (out == 7).all() and n.value == 7 and st.keyframes == 7 and (ms == 7).all()


def test_the_header_is_still_c99(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "scl_engine.h"\nint main(void) { struct scl_map_stats s; int (*fn)(scl_engine *, struct scl_map_stats *) = scl_map_stats; s.growths = 0; return (int)s.growths + (fn != 0); }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr


def _ask(text):
    exe = os.path.join(ROOT, "tests", "cpp", "global_map_plan_check")
    # built here by the Makefile's rule (ASan + UBSan), so that a binary older than global_map_plan.hpp is never what answers
    r = subprocess.run(["make", "-C", ROOT, "tests/cpp/global_map_plan_check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout + r.stderr
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_the_capacity_rule_the_hash_and_the_key():
    ns = [0, 1, 7, 8, 9, 31, 32, 33, 1000, 2 ** 20, 2 ** 20 + 1, 2 ** 31, 2 ** 31 + 1, 3 * 2 ** 40]
    rs = np.random.RandomState(5)
    keys = [0, 1, (1 << 63) - 1, gm.make_key(0, 0, 0)] + [int(rs.randint(0, 2 ** 31)) << 32 | int(rs.randint(0, 2 ** 31)) for _ in range(40)]
    vox = [(0, 0, 0), (-gm.BIAS, -gm.BIAS, -gm.BIAS), (gm.BIAS - 1, gm.BIAS - 1, gm.BIAS - 1), (-1, 2, -3), (5, 0, 0)]
    hooks = [0, 1, 16, 17, 64, 65, 4096, 2 ** 31]
    text = "".join(f"cap {n}\n" for n in ns) + "".join(f"hash {k}\n" for k in keys) + "".join("key %d %d %d\n" % v for v in vox)
    text += "".join(f"start {h}\n" for h in hooks) + "grown 64 10\ngrown 64 200\nprobe 16\nprobe 64\nprobe 128\nprobe 1048576\nload 32 64\nload 33 64\nroom 0 64\nroom 31 64\nroom 32 64\nroom 40 64\n"
    lines = iter(_ask(text))
    for n in ns:
        c = int(next(lines))
        assert c & (c - 1) == 0 and c >= 16 and c >= 2 * n and (c == 16 or c // 2 < 2 * n), (n, c)     # a power of two, never below the load bound
        assert c == gm.capacity_for(n)
    assert gm.capacity_for(2 ** 31) == 2 ** 32                          # formed in 64 bits, not wrapped to 0
    for k in keys:
        assert int(next(lines)) == gm.hash_key(k)
    for v in vox:
        assert int(next(lines)) == gm.make_key(*v)
    assert [int(next(lines)) for _ in hooks] == [2 ** 20, 16, 16, 32, 64, 128, 4096, 2 ** 31]
    assert [int(next(lines)) for _ in range(12)] == [128, 512, 16, 64, 128, 128, 0, 1, 32, 1, 0, 0]
    assert next(lines, None) is None


def test_the_launch_groups_and_their_offsets():
    cases = [(4, 10 ** 9, [5, 0, 7, 3, 0, 0, 2, 9, 1]), (100, 10, [4, 4, 4, 11, 1, 0, 9, 1, 1]), (3, 100, []), (2, 5, [0, 0, 0]),
             (4096, 2 ** 30, [2 ** 30, 5, 2 ** 31 - 1, 7])]
    text = "".join(f"groups {len(c)} {mj} {mp} " + " ".join(map(str, c)) + "\n" for mj, mp, c in cases)
    lines = _ask(text)
    for (mj, mp, counts), line in zip(cases, lines):
        first, offsets = (list(map(int, part.split()[1:])) for part in line.split("|"))
        if not counts:
            assert first == [0] and offsets == []
            continue
        assert first[0] == 0 and first[-1] == len(counts) and first == sorted(set(first))
        for a, b in zip(first, first[1:]):
            assert b - a <= mj and (sum(counts[a:b]) <= mp or b - a == 1)                       # a group's bounds, or one larger job alone
            assert offsets[a:b] == [sum(counts[a:k]) for k in range(a, b)]                      # exclusive sums inside the group
            if b < len(counts):                                                                 # greedy: the next job did not fit
                assert b - a == mj or sum(counts[a:b + 1]) > mp
    assert len(lines) == len(cases)


def _entry_line(r, x, gen, pose):
    return f"{r} {x} {gen} " + " ".join(float(v).hex() for v in pose) + "\n"


def test_the_diff_of_a_set_call_duplicates_and_removals():
    rs = np.random.RandomState(9)
    P = [gm.random_pose(rs, (0, 0, 0), 5.0) for _ in range(6)]
    entries = [(0, 0, 1, P[0]), (0, 1, 1, P[1]), (1, 0, 3, P[2])]
    head = lambda cmd, n: f"{cmd} {len(entries)} {n}\n" + "".join(_entry_line(*e) for e in entries)
    text = head("set", 4) + _entry_line(0, 0, 1, P[0]) + _entry_line(0, 1, 1, P[3]) + _entry_line(0, 2, 1, P[4]) + _entry_line(1, 0, 3, P[2])
    text += head("set", 2) + _entry_line(0, 2, 1, P[4]) + _entry_line(0, 2, 1, P[5])                       # listed twice
    text += head("set", 1) + _entry_line(0, 1, 2, P[3])                                                   # its cloud was put again
    bad = P[4].copy(); bad[1] = np.inf
    text += head("set", 1) + _entry_line(0, 2, 1, bad)
    small = P[4].copy(); small[3:] *= 0.49 / np.linalg.norm(small[3:])
    text += head("set", 1) + _entry_line(0, 2, 1, small)
    negz = P[0].copy(); negz[3:] = -negz[3:]                                                              # the same rotation, other bits: a re-pose
    text += head("set", 1) + _entry_line(0, 0, 1, negz)
    text += head("remove", 2) + "1 0 3\n0 0 1\n" + head("remove", 1) + "0 2 1\n" + head("remove", 2) + "0 0 1\n0 0 1\n" + head("remove", 1) + "0 1 5\n"
    text += "set 0 0\nremove 0 0\n"
    lines = _ask(text)

    def jobs(line):
        part = line.split("|")[1].strip()
        return [(int(j.split()[0]), int(j.split()[1]), [float.fromhex(v) for v in j.split()[2:]]) for j in part.split(";")] if part else []
    assert lines[0].split("|")[0].split() == ["ok", "0", "2", "1", "0"]                                    # skip, re-pose, add, skip
    assert jobs(lines[0]) == [(1, -1, P[1].tolist()), (1, 1, P[3].tolist()), (2, 1, P[4].tolist())]       # the subtraction at the OLD pose, first
    assert lines[1] == "bad: a keyframe is listed twice"
    assert lines[2].startswith("bad: a listed keyframe's stored cloud was replaced")
    assert lines[3] == "bad: a pose is not finite" and lines[4] == "bad: a quaternion's squared norm is outside [0.25, 4]"
    assert lines[5].split("|")[0].split() == ["ok", "2"] and jobs(lines[5]) == [(0, -1, P[0].tolist()), (0, 1, negz.tolist())]
    assert jobs(lines[6]) == [(0, -1, P[2].tolist()), (1, -1, P[0].tolist())]
    assert lines[7] == "bad: a listed keyframe is not in the map" and lines[8] == "bad: a keyframe is listed twice"
    assert lines[9].startswith("bad: a listed keyframe's stored cloud was replaced")
    assert lines[10].split() == ["ok", "|"] and lines[11].split() == ["ok", "|"] and len(lines) == 12

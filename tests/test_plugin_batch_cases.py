"""CPU side of the batched detections: the GRSD restatement of tests/plugin_batch_cases.py against a pair-by-pair loop form, and the
C ABI of the batch calls (declared by the three headers, exported by the built library, headers still plain C99)."""
import os
import re
import subprocess

import numpy as np
import pytest

from plugin_batch_cases import BATCH_CALLS, GRSD_DIM, HEADERS, GrsdChecker, grsd_rows
from plugin_cases import same_detection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sq_dist_pair(a, b):
    """squared L2 of two rows of 21 floats, one float operation at a time in nanoflann's order"""
    s = np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        k = 0
        while k + 4 <= GRSD_DIM:
            d = [np.float32(a[k + j]) - np.float32(b[k + j]) for j in range(4)]
            s = np.float32(s + np.float32(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]))
            k += 4
        while k < GRSD_DIM:
            d = np.float32(a[k]) - np.float32(b[k])
            s = np.float32(s + d * d)
            k += 1
    return s


class _LoopGrsd:
    """scl_grsd.h's detections pair by pair: a candidate replaces the best only when its distance is smaller (a NaN never is), the
    first of equal ones stays"""

    def __init__(self, num_exclude_recent, tree_making_period, inter_mode, robot_num, this_id, dist_thres=160.0):
        self.excl, self.period, self.mode, self.robot_num, self.this_id, self.thres = (num_exclude_recent, tree_making_period, inter_mode,
                                                                                       robot_num, this_id, dist_thres)
        self.rows, self.robots, self.l2g = [], [], [[] for _ in range(robot_num)]
        self.counter, self.snap_n = 0, 0

    def save(self, v, robot, index):
        self.l2g[robot].append(len(self.rows)); self.rows.append(np.asarray(v, np.float32)); self.robots.append(robot)

    def _answer(self, q, keys, local):
        if not keys:
            return -1, np.float32(np.inf)
        best, at = None, -1
        for pos, k in enumerate(keys):
            d = _sq_dist_pair(self.rows[q], self.rows[k])
            if not np.isnan(d) and (best is None or d < best):
                best, at = d, pos
        if best is None:
            return -1, np.float32(np.nan)
        dist = np.float32(np.sqrt(best))
        return ((at if local else keys[at]) if float(dist) < self.thres else -1), dist

    def detect_intra(self, cur):
        mine = self.l2g[self.this_id]
        return self._answer(mine[cur], mine[:max(0, cur - self.excl)], True)

    def detect_inter(self, cur):
        n = len(self.rows)
        if self.mode == 0:
            if n < self.excl + 1:
                return -1, np.float32(0.0)
            if self.counter % self.period == 0:
                self.snap_n = n - self.excl
            self.counter += 1
            return self._answer(cur, list(range(self.snap_n)), False)
        if self.robots[cur] == self.this_id:
            keys = sorted(k for r in range(self.robot_num) if r != self.this_id for k in self.l2g[r])
        else:
            keys = list(self.l2g[self.this_id])
        return self._answer(cur, keys, False)


@pytest.mark.parametrize("mode", (0, 1))
def test_grsd_restatement_agrees_with_the_loop_form(mode):
    """150 drawn rows (10 % copies of row 0: ties), one NaN row and one inf row, three robots: every intra and inter detection of the
    restatement equals the pair-by-pair form, distances by bit pattern"""
    rows = grsd_rows(150, seed=5)
    rows[40, 3] = np.nan
    rows[77, 9] = np.inf
    kw = dict(num_exclude_recent=7, tree_making_period=3, inter_mode=mode, robot_num=3, this_id=1)
    a, b = GrsdChecker(**kw), _LoopGrsd(**kw)
    for k, v in enumerate(rows):
        a.save(v, k % 3, k); b.save(v, k % 3, k)
        if k in (3, 60, 149):                                   # before num_exclude_recent + 1 keyframes, midway, full
            for cur in range(0, k + 1, 5):
                assert same_detection(a.detect_inter(cur), b.detect_inter(cur), nan_ok=True), (k, cur)
    for cur in range(len(a.l2g[1])):
        assert same_detection(a.detect_intra(cur), b.detect_intra(cur), nan_ok=True), cur
    for cur in range(150):
        assert same_detection(a.detect_inter(cur), b.detect_inter(cur), nan_ok=True), cur
    lost = a.detect_inter(40)                                                     # the NaN query row: nothing is nearest
    assert lost[0] == -1 and np.isnan(lost[1])
    ties = [k for k in range(1, 150) if np.array_equal(rows[k], rows[0])]
    assert ties, "the drawn rows hold copies of row 0"


@pytest.mark.parametrize("plugin", sorted(HEADERS))
def test_headers_declare_and_the_library_exports_the_batch_calls(plugin):
    """the declarations as a C compiler sees them (the header through the preprocessor: the four calls come from
    SCL_PLUGIN_BATCH_API of scl_plugin_batch.h), and the symbols of the built library"""
    pre = subprocess.run(["gcc", "-std=c99", "-E", "-P", "-I", os.path.join(ROOT, "include"), "-x", "c",
                          os.path.join(ROOT, "include", HEADERS[plugin])], capture_output=True, text=True, check=True).stdout
    lib = os.path.join(ROOT, "scl_slam_amd", "lib", "libscl_engine.so")
    assert os.path.exists(lib), "build it with `make`"
    exported = set(re.findall(r" T (\w+)", subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout))
    for call in BATCH_CALLS:
        name = f"scl_{plugin}_{call}"
        assert re.search(r"\bint\s+%s\s*\(\s*scl_%s\s*\*" % (name, plugin), pre), f"{HEADERS[plugin]} does not declare {name}"
        assert name in exported, f"libscl_engine.so does not export {name}"


@pytest.mark.parametrize("plugin", sorted(HEADERS))
def test_headers_are_plain_c99(plugin):
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", os.path.join(ROOT, "include", HEADERS[plugin])], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

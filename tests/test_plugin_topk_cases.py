"""CPU side of the candidate lists (scl_X_detect_intra_topk / scl_X_detect_inter_topk, include/scl_plugin_batch.h): the checker
top-k of tests/plugin_topk_cases.py against a pair-by-pair loop form that keeps its list the way nanoflann's KNNResultSet does and
against the reference's own nanoflann (tests/golden/plugin_topk_golden.json), and the C ABI of the two calls (declared by the three
headers, exported by the built library)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from golden.gen_plugin_topk_golden import CASES, K, golden_keys, golden_queries
from plugin_topk_cases import HEADERS, TOPK_CALLS, TopkModel, checker_topk, plugin_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plugin_topk_golden.json")


def _sq_dist_pair(a, b, dims):
    """squared L2 of two rows over the first dims floats, one float operation at a time in nanoflann's order"""
    s = np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        k = 0
        while k + 4 <= dims:
            d = [np.float32(a[k + j]) - np.float32(b[k + j]) for j in range(4)]
            s = np.float32(s + np.float32(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]))
            k += 4
        while k < dims:
            d = np.float32(a[k]) - np.float32(b[k])
            s = np.float32(s + d * d)
            k += 1
    return s


def _loop_topk(q, cands, k, report_dims):
    """the candidates in list order into a result set of k: one enters only when its distance is below the worst kept (a NaN never
    is) or the set is not full, behind every kept one that is not farther -- equal distances stay in list order"""
    kept = []                                                                    # (sum, position), ascending
    for pos, c in enumerate(cands):
        d = _sq_dist_pair(q, c, len(q))
        if np.isnan(d) or (len(kept) == k and not d < kept[-1][0]):
            continue
        at = len(kept)
        while at > 0 and d < kept[at - 1][0]:
            at -= 1
        kept.insert(at, (d, pos))
        del kept[k:]
    with np.errstate(invalid="ignore", over="ignore"):
        rep = [np.float32(np.sqrt(_sq_dist_pair(q, cands[pos], report_dims))) for _, pos in kept]
    return [pos for _, pos in kept], [d for d, _ in kept], rep


def _bits(a):
    return [int(x) for x in np.ascontiguousarray(a, np.float32).view(np.uint32)]


@pytest.mark.parametrize("plugin, report_dims", (("m2dp", 192), ("fpfh", 21), ("fpfh", 33), ("grsd", 21)))
def test_checker_topk_agrees_with_the_loop_form(plugin, report_dims):
    """150 drawn rows with exact copies (ties), two NaN rows, a +inf and a -inf row; k = 1, 2, 10, 32 and more candidates than k,
    exactly k, fewer: positions, sums and reported distances equal, the floats by bit pattern"""
    rows = plugin_rows(plugin, 150, seed=9)
    dim = rows.shape[1]
    rows[17, dim - 1] = np.nan; rows[60, 0] = np.nan
    rows[33, 2] = np.inf; rows[34, dim - 2] = -np.inf
    for qi in (149, 5, 33):
        for n in (0, 1, 9, 10, 11, 70, 140):
            for k in (1, 2, 10, 32):
                pos, s, rep = checker_topk(rows[qi], rows[:n], k, report_dims)
                lp, ls, lr = _loop_topk(rows[qi], rows[:n], k, report_dims)
                assert [int(p) for p in pos] == lp and _bits(s) == _bits(ls) and _bits(rep) == _bits(lr), (qi, n, k)
                assert len(lp) == min(k, n - sum(1 for b in (17, 60) if b < n)) or qi == 33
    assert checker_topk(rows[17], rows[:140], 10, report_dims)[0].size == 0        # a NaN query row: nothing is listed
    pos, s, _ = checker_topk(rows[149], rows[:140], 140, report_dims)
    assert np.isposinf(s[-2:]).all() and set(pos[-2:]) == {33, 34}                 # +inf sums are candidates, the last ones
    assert any(s[j] == s[j + 1] and np.isfinite(s[j]) and pos[j] < pos[j + 1] for j in range(s.size - 1)), "the drawn rows hold ties"


def test_model_walks_the_reference_inter_state():
    """inter_mode 0 of the model: below num_exclude_recent + 1 keyframes nothing is found and the counter stays; then the snapshot is
    retaken every tree_making_period queries, inside a call too; entry 0 is the nearest of the snapshot"""
    rows = plugin_rows("grsd", 60, seed=3)
    m = TopkModel("grsd", num_exclude_recent=5, tree_making_period=3, inter_mode=0, robot_num=2, this_id=0)
    m.save_many(rows[:5], np.arange(5) % 2)
    ids, dists, found = m.topk("inter", [0, 4, 2], 4)
    assert (found == 0).all() and (ids == -1).all() and np.isposinf(dists).all() and m.counter == 0
    m.save_many(rows[5:40], np.arange(5, 40) % 2)
    m.topk("inter", [1, 2], 4)
    assert (m.counter, m.snap_n) == (2, 35)
    m.save_many(rows[40:], np.arange(40, 60) % 2)
    ids, _, found = m.topk("inter", [59, 58, 57], 32)                             # the second query retakes the snapshot
    assert (m.counter, m.snap_n) == (5, 55) and ids[0].max() < 35 and ids[1].max() >= 35 and (found == 32).all()


def test_checker_topk_agrees_with_the_reference_nanoflann():
    """the order of the list is nanoflann's: every stored query of the golden file (192, 33 and 21 dimensions, k = 10; queries with a
    tie among the first k + 1 sums are left out there) -- indices and squared distances by bit pattern"""
    gold = json.load(open(GOLDEN))
    assert gold["k"] == K and sorted(gold["cases"]) == sorted(c[0] for c in CASES)
    for name, dim, N, seed, nq in CASES:
        case = gold["cases"][name]
        keys = golden_keys(dim, N, seed)
        queries = golden_queries(keys, seed, nq)
        assert len(case["results"]) == nq and case["left_out"] <= 0.1 * nq
        for q, want in zip(queries, case["results"]):
            if want.get("tie"):
                continue
            pos, s, _ = checker_topk(q, keys, K)
            assert want["found"] == min(K, N) == pos.size, name
            assert [int(p) for p in pos] == want["idx"] and _bits(s) == want["d2_bits"], name


@pytest.mark.parametrize("plugin", sorted(HEADERS))
def test_headers_declare_and_the_library_exports_the_topk_calls(plugin):
    """the declarations as a C compiler sees them (SCL_PLUGIN_TOPK_API of scl_plugin_batch.h through the preprocessor, the header
    still plain C99), and the symbols of the built library"""
    inc = os.path.join(ROOT, "include")
    pre = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-E", "-P", "-I", inc, "-x", "c",
                          os.path.join(inc, HEADERS[plugin])], capture_output=True, text=True, check=True).stdout
    lib = os.path.join(ROOT, "scl_slam_amd", "lib", "libscl_engine.so")
    assert os.path.exists(lib), "build it with `make`"
    exported = set(re.findall(r" T (\w+)", subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout))
    for call in TOPK_CALLS:
        name = f"scl_{plugin}_{call}"
        assert re.search(r"\bint\s+%s\s*\(\s*scl_%s\s*\*\s*h\s*,\s*const\s+int\s*\*\s*curs\s*,\s*int\s+count\s*,\s*int\s+k\s*," % (name, plugin), pre), \
            f"{HEADERS[plugin]} does not declare {name}"
        assert name in exported, f"libscl_engine.so does not export {name}"
    assert "SCL_PLUGIN_TOPK_MAX 32" in open(os.path.join(inc, "scl_plugin_batch.h")).read()

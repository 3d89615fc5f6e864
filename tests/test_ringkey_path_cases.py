"""The cases of tests/ringkey_path_cases.py, pinned with the CPU checker alone (no GPU), so that tests/test_gpu_ringkey_paths.py may
rest on them:
  - the constants the cases are worked out from are the ones in the sources (kernels.hpp, topk_merge.hpp, ringkey_topk.hip,
    engine.hip), so an edit of a limit turns this file red instead of silently moving a case to the other side;
  - the case list holds at least one case on each side of each of the six rules of the dispatch;
  - every planted placement holds on oracle_binding.knn: "the nearest keys lie in the last chunk", "workgroup w's neighbours are
    split over its two chunks", "fewer than q lists have an m-th key", "40 equal distances over three workgroups", ...;
  - every id names the path the case's own arithmetic gives."""
import os
import re

import numpy as np
import pytest

import oracle_binding as ob
import ringkey_path_cases as rc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scl_slam_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert m, name
    return int(m.group(1))


def test_the_restated_constants_are_the_sources():
    kern, merge, topk, eng = _src("kernels.hpp"), _src("topk_merge.hpp"), _src("ringkey_topk.hip"), _src("engine.hip")
    assert _const(kern, "kTopkMaxBlocks") == rc.MAX_BLOCKS and _const(kern, "kTopkMaxK") == rc.MAX_K
    assert _const(kern, "kCandMergeMaxKeys") == rc.CAND_MAX_KEYS and _const(kern, "kTailTop") == rc.FULL_KS[0] == rc.FULL_KS[1] - 1
    assert _const(merge, "kTopkMergeLds") == rc.MERGE_LDS
    assert _const(topk, "kTopkThreads") == rc.THREADS and _const(topk, "kTopkPerThread") * rc.THREADS == rc.CHUNK
    assert "if (n <= kTopkThreads * kTopkMaxBlocks) {" in topk
    assert f"if (RGfull <= {rc.STRAIGHT_MAX_GROUPS} && tail == 0) {{" in topk and f"if (k <= {rc.DPP_MAX_K}) {{" in topk
    assert "if (n_lists * k <= kTopkMergeLds) {" in topk and f"__shared__ float sq[{rc.MAX_RINGS}];" in topk
    assert f"*have_dist && k <= {rc.CAND_MAX_K} && sc_cand_exact_supported" in eng and "const bool fused = n_lists * k <= kCandMergeMaxKeys;" in eng
    assert f"cfg->num_ring < 1 || cfg->num_ring > {rc.MAX_RINGS}" in eng and rc.METRIC_REFUSED_R == rc.MAX_RINGS + 1
    assert "db.RG == 5 && db.S == 60 && W == 7 && db.R == 20" in _src("sc_masked.hip")       # section 5's grid is a supported one


def test_both_sides_of_each_of_the_six_rules():
    routes = [r for r, _ in rc.all_routes()]
    have = lambda **kw: any(all(r[a] == b for a, b in kw.items()) for r in routes)       # noqa: E731
    assert have(scan="lists") and have(scan="chunked") and have(scan="chunked-stride")                        # 1
    assert have(scan="lists", metric="straight") and have(scan="lists", metric="general") and have(scan="chunked", metric="general")   # 2
    assert have(rank="dpp") and have(rank="count")                                                            # 3
    assert have(merge="threshold", cand=None, tail=None) and have(merge="rounds", cand=None, tail=None)       # 4, the bare search
    assert have(scan="chunked", merge="threshold") and have(scan="chunked", merge="rounds")
    assert have(cand="cand-fused") and have(cand="cand-merge-first", merge="threshold") and have(cand="cand-merge-first", merge="rounds")   # 5
    assert have(tail="dist-pack", merge="threshold") and have(tail="dist-pack", merge="rounds")               # 6
    # ... and the very edges: the last launch of the lists kernel and the first of the chunked one, 3 072 and 1 024 keys exactly
    edge = [(r["lists"], rid) for r, rid in rc.all_routes()]
    assert any(c.hi - c.lo == 65536 for c in rc.range_world()[1]) and any(c.hi - c.lo == 65537 for c in rc.range_world()[1])
    assert any(L * k == rc.MERGE_LDS for c in rc.merge_world()[1] for k in c.ks for L in [rc.route(c.hi - c.lo, rc.MERGE_R, k)["lists"]])
    assert any(rc.route(hi - lo, rc.GRID_R, k, "dist", True)["lists"] * k == rc.CAND_MAX_KEYS for _, lo, hi, k in rc.grid_cases())
    assert len(edge) > 300


def test_the_sizes_the_issue_sets():
    sizes = {c.hi - c.lo for c in rc.range_world()[1]}
    assert sizes == set(rc.RANGE_SIZES) == {65535, 65536, 65537, 66560, 66561, 262144, 262145, 263169}
    assert {c.lo for c in rc.range_world()[1]} == {0, 1023} and rc.RANGE_KS == (1, 3, 8, 9, 64) and rc.RANGE_N == 262144 + 1025
    assert rc.METRIC_RS == (1, 3, 4, 22, 60, 64, 68, 100, 130, 255, 256) and rc.METRIC_KS == (3, 25) and rc.METRIC_BIG == (68, 66000)
    assert rc.SHORT_SIZES == (0, 1, 2, 5, 63, 64, 65, 255, 256, 257, 513) and rc.SHORT_KS == (1, 2, 7, 8, 9, 16, 64)
    assert [(L * k <= rc.MERGE_LDS) for k, L in rc.MERGE_BOUNDS] == [True, False] * 3
    assert [rc.threshold_mq(L, k)[0] for L, k in rc.THRESHOLD_SHAPES] == [64, 32, 22, 13, 2, 1]
    assert [(L * k <= rc.CAND_MAX_KEYS) for k, L in rc.CAND_BOUNDS] == [True, False] * 3
    assert -(-rc.ROUNDS_L * 64 // (4 * rc.THREADS)) >= 4 and rc.ROUNDS_L * 64 > 4096


def test_every_id_names_its_path():
    for c in rc.range_world()[1]:
        assert c.id.startswith(rc.route(c.hi - c.lo, rc.RANGE_R, 1)["scan"] + "-n"), c.id
    for c in rc.short_world()[1]:
        ranks = {rc.route(c.hi - c.lo, rc.SHORT_R, k)["rank"] for k in c.ks}
        assert len(ranks) == 1 and (c.hi == c.lo or f"rank-{ranks.pop()}-" in c.id), c.id
    for c in rc.merge_world()[1]:
        merges = {rc.route(c.hi - c.lo, rc.MERGE_R, k)["merge"] for k in c.ks}
        assert len(merges) == 1 and merges.pop() in c.id, c.id
        assert ("chunked" in c.id) == (rc.route(c.hi - c.lo, rc.MERGE_R, 1)["scan"] == "chunked")
    for R, N in rc.metric_worlds():
        for c in rc.metric_world(R, N)[1]:
            assert f"metric-{rc.route(c.hi - c.lo, R, 3)['metric']}-R{R}-{rc.route(c.hi - c.lo, R, 3)['scan']}" in c.id
    ids = [c.id for w in (rc.range_world, rc.short_world, rc.merge_world) for c in w()[1]] + [g[0] for g in rc.grid_cases()]
    assert len(set(ids)) == len(ids)


def _tables(c):
    if c.db == "range":
        return rc.range_world()[0]
    if c.db == "merge":
        return rc.merge_world()[0]
    return rc.short_world()[0][c.db]


PLANTED = [c for w in (rc.range_world, rc.short_world, rc.merge_world) for c in w()[1] if c.prop is not None]


@pytest.mark.parametrize("c", PLANTED, ids=lambda c: c.id)
def test_the_planted_placement_holds_on_the_checker(c):
    keys = _tables(c)
    n_checked = 0
    for k in c.ks:
        for kind, val in c.queries:
            if not (c.prop_all or kind == "planted"):
                continue
            o_idx, o_d2, o_found = ob.knn(keys[c.lo:c.hi], keys[val] if kind == "slot" else val, k, exclude_eps=c.eps)
            assert c.prop(o_idx, o_found, k), (c.id, k, kind, o_idx[:o_found])
            if kind == "planted":                            # rank j sits at squared distance ((j + 1) / 64)^2, exactly
                want = (((np.arange(o_found) + 1) / 64.0) ** 2).astype(np.float32)
                planted = int(np.sum(np.all(np.abs(keys[c.lo:c.hi] - val) <= 1.0, axis=1)))
                assert np.array_equal(o_d2[:min(o_found, planted)], want[:min(o_found, planted)]), c.id
            n_checked += 1
    assert n_checked


def test_the_stride_cases_need_the_list_carried_between_the_chunks():
    """(c): a workgroup that forgot its first chunk's keys would return the second chunk's only -- both chunks hold neighbours"""
    keys, cases = rc.range_world()
    split = [c for c in cases if "split-over-its-two-chunks" in c.id]
    assert {c.hi - c.lo for c in split} == {262145, 263169}
    for c in split:
        o_idx, _, found = ob.knn(keys[c.lo:c.hi], c.queries[0][1], 8)
        chunks = [int(x) // rc.CHUNK for x in o_idx[:found]]
        assert len(set(chunks)) == 2 and max(chunks) - min(chunks) == rc.MAX_BLOCKS and chunks[0] == max(chunks)


def test_the_threshold_cases_whose_tau_is_no_key():
    """fewer than q lists hold m valid keys, so the q-th smallest of the lists' m-th entries is "no key"; and the mostly-holes ranges
    begin with empty lists"""
    keys, cases = rc.merge_world()
    sel = [c for c in cases if c.id.endswith("tau-is-no-key")]
    assert len(sel) == len(rc.THRESHOLD_SHAPES)
    for c in sel:
        k = c.ks[0]
        L = rc.route(c.hi - c.lo, rc.MERGE_R, k)["lists"]
        m, q = rc.threshold_mq(L, k)
        valid = np.isfinite(keys[c.lo:c.hi]).all(axis=1)
        per_list = [int(valid[i * rc.THREADS:(i + 1) * rc.THREADS].sum()) for i in range(L)]
        assert sum(v >= m for v in per_list) < q, (c.id, per_list)
        if "holes" in c.id:
            assert per_list[0] == per_list[1] == 0 and sum(per_list) >= k
    for c in cases:
        if c.id.endswith("m-in-each-of-the-first-q-lists") or c.id.endswith("all-in-one-list"):
            assert np.isfinite(keys[c.lo:c.hi]).all()


def test_the_blocks_of_copies_holes_and_ties():
    tables, cases = rc.short_world()
    a, b = rc.BLOCK
    assert b - a == 300 and np.all(tables["copies"][a:b] == tables["copies"][600]) and not np.isfinite(tables["holes"][a:b]).any()
    assert np.isnan(tables["holes"][a + 1]).all() and np.isposinf(tables["holes"][a]).all() and np.isneginf(tables["holes"][a + 2]).all()
    for c in cases:
        if "exclude-every-copy-n513" in c.id:               # [300, 813): the second and the third workgroup hold copies only
            assert c.lo + rc.THREADS >= a and c.hi <= b
        if "holes-first-list-empty" in c.id:
            assert a <= c.lo and c.lo + rc.THREADS <= b and c.hi > b
    ties = tables["holes"][list(rc.TIE_SLOTS)]
    assert len({t.tobytes() for t in ties}) == 40            # forty different keys ...
    q = np.full(rc.SHORT_R, rc.TIE_CENTRE, np.float32)
    _, d2, found = ob.knn(tables["holes"][0:513], q, 64)
    assert found == 64 and np.all(d2[:40].view(np.uint32) == np.float32(0.0625).view(np.uint32)) and d2[40] > 1.0    # ... one distance
    assert sorted({s // rc.THREADS for s in rc.TIE_SLOTS}) == [0, 1, 2]

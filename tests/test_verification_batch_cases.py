"""The candidate list of tests/verification_batch_cases.py pinned on the CPU checker (oracle/icp_oracle.c), one
icpo_geometric_verification per candidate on the scan's finite rows (verification_cases.CHECKER_ON_FINITE_ROWS).  Without this,
"batch == single call == checker" in tests/test_gpu_verification_batch.py could hold on a list whose candidates all answer alike.
No GPU needed; every checker call takes about 10 ms."""
import functools

import numpy as np
import pytest

import oracle_icp_binding as oi
import verification_batch_cases as bc


@functools.lru_cache(maxsize=None)
def checker(iterations, threshold=bc.THRESHOLD, ratio=bc.RATIO, seed=bc.SEED):
    """[(T, success, n_corr, n_inliers)] per candidate, computed once per setting and shared (the GPU tests import it)"""
    src = bc.finite_source()
    return [oi.geometric_verification(src, c, iterations, threshold, ratio, seed) for c in bc.clouds()]


def test_the_scan_and_the_list():
    src, rows = bc.source()
    assert src.shape == (2000, 8) and len(rows) == bc.N_NONFINITE
    assert (~np.isfinite(src[:, :3]).all(1)).sum() == bc.N_NONFINITE and len(bc.finite_source()) == 2000 - bc.N_NONFINITE
    names = bc.names()
    assert len(names) == len(set(names)) == 13
    sizes = dict(zip(names, (len(c) for c in bc.clouds())))
    assert (sizes["first_257"], sizes["first_256"], sizes["first_3"], sizes["first_1"], sizes["empty"]) == (257, 256, 3, 1, 0)
    assert sizes["other_place"] == 3000 and sizes["matching"] == sizes["permuted"] == sizes["half_moved"] == 4000
    a, b = bc.clouds()[names.index("matching")], bc.clouds()[names.index("permuted")]
    assert not np.array_equal(a, b) and np.array_equal(np.sort(a[:, 0]), np.sort(b[:, 0]))


@pytest.mark.parametrize("iterations", bc.ITERATIONS)
def test_the_list_tells_candidates_apart(iterations):
    res = dict(zip(bc.names(), checker(iterations)))
    for n, r in res.items():
        print(iterations, n, r[1:])
    assert any(r[1] for r in res.values()) and any(not r[1] for r in res.values())
    assert len({r[3] for r in res.values()}) >= 4                     # a batch that mixes up candidates cannot pass
    a, b = res["matching"], res["matching_again"]
    assert a[1:] == b[1:] and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert res["empty"][1:] == (False, 0, 0) and np.array_equal(res["empty"][0], np.eye(4, dtype=np.float32))
    for n, r in res.items():
        if n != "empty":
            assert r[2] == 2000 - bc.N_NONFINITE                      # every finite source finds a neighbour in a non-empty target
        if r[3] < 3:
            assert np.array_equal(r[0], np.eye(4, dtype=np.float32))
    assert res["matching"][1] and res["permuted"][1:] == res["matching"][1:]
    assert not res["yaw_90"][1] and not res["other_place"][1] and not res["first_3"][1]


def test_the_counts_move_with_the_iteration_count():
    """1, 9 and 300 hypotheses answer differently on the failing candidates: a batch that ignores its iteration count cannot pass"""
    counts = {it: tuple(r[3] for r in checker(it)) for it in (1, 9, 300)}
    assert len(set(counts.values())) == 3

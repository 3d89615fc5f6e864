"""The checkers of tests/plugin_cases.py that tests/test_gpu_plugins_at_scale.py holds the GPU to, checked here without one: the
vectorised 1-NN equals the loop form bit for bit, and a NaN distance never wins (nanoflann admits a point only when
dist < worst)."""
import numpy as np

import fpfh_checker as fc
import m2dp_checker as mc
from plugin_cases import FpfhChecker, M2dpChecker, first_minimum, sq_dist_rows


def _same(x, y):
    return x[0] == y[0] and (np.float32(x[1]).view(np.uint32) == np.float32(y[1]).view(np.uint32) or (np.isnan(x[1]) and np.isnan(y[1])))


def test_vectorised_distance_equals_the_loop_form_on_2000_pairs():
    """sq_dist_rows against m2dp_checker.sqdist_nanoflann (192 floats) and fpfh_checker.sq_dist (33 and 21 floats: the tail) on
    2 000 random pairs each -- rows of every magnitude, exact copies, infinities, a NaN -- by bit pattern"""
    rs = np.random.RandomState(17)
    for dim in (mc.DIM, fc.DIM):
        a = (rs.standard_normal((2000, dim)) * 10.0 ** rs.uniform(-4, 3, size=(2000, 1))).astype(np.float32)
        b = (a + rs.standard_normal((2000, dim)) * 10.0 ** rs.uniform(-6, 2, size=(2000, 1))).astype(np.float32)
        b[::50] = a[::50]
        b[7, dim - 1] = np.inf; a[9, 3] = np.nan; b[11, 20] = -np.inf; a[11, 20] = -np.inf
        for i in range(2000):
            many = sq_dist_rows(a[i], b[i:i + 3])
            with np.errstate(invalid="ignore", over="ignore"):
                one = mc.sqdist_nanoflann(a[i], b[i]) if dim == mc.DIM else fc.sq_dist(a[i], b[i:i + 1])[0]
                short = None if dim == mc.DIM else fc.sq_dist(a[i], b[i:i + 1], 21)[0]
            assert _same((0, many[0]), (0, one)), (dim, i)
            if short is not None:
                assert _same((0, sq_dist_rows(a[i], b[i:i + 1], 21)[0]), (0, short)), i


def test_vectorised_1nn_equals_the_loop_form():
    """the two forms of M2dpChecker's 1-NN on a database with ties, NaN rows and rows with an infinity; and on a database without
    them both equal m2dp_checker.CheckerDB as it stands"""
    rs = np.random.RandomState(18)
    protos = np.abs(rs.standard_normal((3, mc.DIM))).astype(np.float32) * 0.1
    for special in (True, False):
        kw = dict(robot_num=2, this_id=0, num_exclude_recent=3)
        loop, fast, plain = M2dpChecker(**kw), M2dpChecker(vectorised=True, **kw), mc.CheckerDB(**kw)
        for k in range(60):
            v = protos[rs.randint(3)] + (rs.standard_normal(mc.DIM).astype(np.float32) * 0.01 if rs.rand() < 0.5 else 0.0)
            v = np.asarray(v, np.float32)
            if special and k in (10, 31):
                v[5] = np.nan
            if special and k in (12, 33):
                v[6] = np.inf
            for c in (loop, fast, plain):
                c.save(v, k % 2, k)
        for cur in range(30):
            assert _same(loop.detect_intra(cur), fast.detect_intra(cur)), cur
            assert special or _same(loop.detect_intra(cur), plain.detect_intra(cur)), cur
        for key in range(60):
            assert _same(loop.detect_inter(key), fast.detect_inter(key)), key
            assert special or _same(loop.detect_inter(key), plain.detect_inter(key)), key


def test_a_nan_distance_never_wins():
    """a NaN row that comes first in the list must not become the nearest, and a query that is a NaN row finds nothing:
    (-1, NaN); an empty search set stays (-1, +inf); +inf wins only over NaNs, at its own first position"""
    s = lambda *v: np.array(v, np.float32)
    assert first_minimum(s(np.nan, 2.0, 1.0, 1.0, np.inf)) == 2
    assert first_minimum(s(np.nan, np.inf, np.nan, np.inf)) == 1
    assert first_minimum(s(np.nan, np.nan)) == -1 and first_minimum(s()) == -1
    for vectorised in (False, True):
        c = M2dpChecker(num_exclude_recent=0, dist_thres=10.0, vectorised=vectorised)
        rows = np.zeros((4, mc.DIM), np.float32)
        rows[0, 0] = np.nan; rows[1, 0] = 3.0; rows[2, 0] = 1.0; rows[3, 0] = 1.5
        for k in range(4):
            c.save(rows[k], 0, k)
        assert c.detect_intra(3) == (2, np.float32(0.5))
        assert c.detect_intra(2) == (1, np.float32(2.0))
        loop, d = c.detect_intra(1)                                # the only candidate is the NaN row
        assert loop == -1 and np.isnan(d)
        loop, d = c._nn(0, [1, 2, 3])                              # the NaN row as the query
        assert loop == -1 and np.isnan(d)
        assert c.detect_intra(0) == (-1, np.float32(np.inf))
    rows = np.zeros((5, fc.DIM), np.float32)
    rows[0, 32] = np.nan; rows[1, 0] = 2.0; rows[2, 32] = 1.0; rows[3, 32] = 1.0; rows[4, 25] = np.inf
    db = FpfhChecker(num_exclude_recent=0, inter_mode=1, robot_num=2, this_id=0, report_dims=21)
    for k in range(5):
        db.save(rows[k], k % 2, k)
    loop, d = db.detect_intra(2)      # robot 0 holds rows 0, 2, 4: the query is the inf row, the NaN row comes first in its history
    assert loop == 1 and d == np.float32(0.0)                      # +inf to row 2 beats the NaN; over 21 reported floats the two rows agree
    loop, d = db.detect_inter(0)                                   # the NaN row as the query
    assert loop == -1 and np.isnan(d)
    loop, d = db.detect_inter(3)                                   # robot 1's row 3 among robot 0's rows 0 (NaN), 2 (equal), 4 (inf)
    assert loop == 2 and d == np.float32(0.0)

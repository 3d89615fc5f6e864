"""Named clouds for the voxel filter's tests (numpy only) and a plain restatement of the filter.

tests/test_voxel_cases.py pins the CPU checker (oracle/icp_oracle.c, icpo_voxel_grid) on these clouds -- by answers written out by
hand and by restate() below --, tests/test_gpu_voxel.py holds csrc/voxel.hip to the checker on the same clouds, bit for bit.
A case is (cloud [n, floats per point] float32, leaf); cases() builds them all, by name, once."""
import numpy as np

F32_TINY = np.float32(2.0 ** -149)                                   # the smallest subnormal
SIZES = (1, 2, 255, 256, 257, 65535, 65536, 65537, 70000)           # past 65 536 points the bounding-box grid stops at 256 blocks
STRIDES = (12, 16, 20, 32, 48)
BOUNDARY_LEAVES = (0.25, 0.5, 0.1, 0.2, 0.4)                         # the first two are exact in fp32 (so is 1 / leaf)
NONFINITE = (np.nan, np.inf, -np.inf)


def boundary_values(leaf):
    """k * leaf for k = -40 .. 40, each with its two neighbouring floats, then -0.0 and +0.0"""
    v = np.array([np.float32(k * leaf) for k in range(-40, 41)], np.float32)
    below, above = np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))
    return np.concatenate([np.stack([v, above, below], 1).reshape(-1), np.array([-0.0, 0.0], np.float32)])


def boundaries(leaf, seed=0):
    """three lines of the boundary values, one along each axis (the other two coordinates at 0.3 leaf), then 600 points whose
    coordinates are drawn from the values: voxel k of a line holds k * leaf, its upper neighbour and (k + 1) * leaf's lower one"""
    vals = boundary_values(leaf)
    rs = np.random.RandomState(100 + seed)
    mid = np.float32(0.3 * leaf)
    c = np.zeros((3 * vals.size + 600, 8), np.float32)
    for a in range(3):
        blk = c[a * vals.size:(a + 1) * vals.size]
        blk[:, :3] = mid
        blk[:, a] = vals
    c[3 * vals.size:, :3] = vals[rs.randint(0, vals.size, (600, 3))]
    c[:, 4] = rs.uniform(0, 100, c.shape[0])
    return c[rs.permutation(c.shape[0])]


ORDER_LEAF = 1.0


def order(seed=0):
    """200 voxels (20 x 10 in y, z; leaf 1) of 3 .. 9 points whose coordinates inside the voxel are u * 2^-e, e = 0 .. 20 with a
    spread of at least 2^12 in every voxel, scattered through the cloud: a voxel's fp32 sums depend on the order of its points"""
    rs = np.random.RandomState(200 + seed)
    rows = []
    for v in range(200):
        m = rs.randint(3, 10)
        e = rs.randint(0, 21, (m, 4))
        e[0], e[1] = rs.randint(0, 5, 4), rs.randint(17, 21, 4)      # magnitudes 2^12 .. 2^21 apart
        p = (rs.uniform(0.5, 1.0, (m, 4)) * 2.0 ** -e.astype(np.float64)).astype(np.float32)
        r = np.zeros((m, 8), np.float32)
        r[:, 0], r[:, 1], r[:, 2] = p[:, 0], np.float32(v % 20) + p[:, 1], np.float32(v // 20) + p[:, 2]
        r[:, 4] = p[:, 3] * 4096 * rs.choice([-1, 1], m)              # (intensities of both signs: their sums cancel)
        rows.append(r)
    c = np.concatenate(rows)
    return c[rs.permutation(c.shape[0])]


def one_voxel(n=5000, seed=0):
    rs = np.random.RandomState(300 + seed)
    c = np.zeros((n, 8), np.float32)
    c[:, :3] = rs.uniform(12.01, 12.39, (n, 3))                      # leaf 0.4: voxel 30 of every axis
    c[:, 4] = rs.uniform(0, 255, n)
    return c


def all_distinct():
    """16^3 points, one per voxel of leaf 0.5, in DESCENDING voxel index (x fastest): the filter returns them reversed"""
    i = np.arange(4096)[::-1]
    c = np.zeros((4096, 8), np.float32)
    c[:, 0], c[:, 1], c[:, 2] = (i % 16) * 0.5 + 0.125, (i // 16 % 16) * 0.5 + 0.25, (i // 256) * 0.5 + 0.375
    c[:, 4] = i
    return c


def _random_cloud(n, seed, extent=(6.0, 6.0, 2.0), floats=8):
    rs = np.random.RandomState(seed)
    c = np.zeros((n, floats), np.float32)
    c[:, :3] = rs.uniform(-1, 1, (n, 3)) * extent
    if floats > 4:
        c[:, 4] = rs.uniform(0, 255, n)
    return c


def sized(n):
    return _random_cloud(n, 400 + n)


def nonfinite_mixed():
    """600 points; NaN, +inf and -inf each in x only, y only and z only, at row 0, the last row, rows 255 .. 257 and four more"""
    c = _random_cloud(600, 500)
    rows = [0, 599, 255, 256, 257, 1, 254, 258, 598]
    for r, (a, bad) in zip(rows, [(a, bad) for bad in NONFINITE for a in range(3)]):
        c[r, a] = bad
    return c


def nonfinite_all():
    c = _random_cloud(300, 501)
    for r in range(300):
        c[r, r % 3] = NONFINITE[r // 3 % 3]
    return c


def nonfinite_fields():
    """finite coordinates; NaNs of several payloads in the intensity and in a padding field: the points stay"""
    c = _random_cloud(400, 502)
    u = c.view(np.uint32)
    for r, bits in zip((0, 3, 128, 255, 256, 399), (0x7fc00000, 0xffc00000, 0x7fc00001, 0x7fa00000, 0xffffffff, 0x7f800001)):
        u[r, 4] = bits
    for r, bits in zip((1, 3, 200, 398), (0x7fc00000, 0xffc12345, 0x7fa00000, 0x7fc00000)):
        u[r, 6] = bits
    return c


def subnormal(max_m=1 << 14, n=300, seed=0):
    """coordinates and intensities m * 2^-149, |m| <= max_m"""
    rs = np.random.RandomState(600 + seed)
    c = np.zeros((n, 8), np.float32)
    m = rs.randint(1, max_m + 1, (n, 4)) * rs.choice([-1, 1], (n, 4))
    m[:, 3] = np.abs(m[:, 3])
    c[:, :3] = m[:, :3].astype(np.float32) * F32_TINY
    c[:, 4] = m[:, 3].astype(np.float32) * F32_TINY
    return c


def index_cloud(far, extra=True):
    """leaf 1: the corners (0, 0, 0) and `far`, and three points inside the box"""
    pts = [(0, 0, 0), far]
    if extra:
        pts += [(far[0] + 0.25, far[1] + 0.5, far[2] + 0.75), (1000.5, 500.5, 511.5), (0.5, 0.5, 0.5)]
    c = np.zeros((len(pts), 8), np.float32)
    c[:, :3] = np.array(pts, np.float32)
    c[:, 4] = np.arange(len(pts)) + 1
    return c


def strided(stride_bytes, seed=0):
    """every field filled: only x, y, z (and the intensity from 20 bytes up) survive the filter, the rest comes back zero"""
    w = stride_bytes // 4
    rs = np.random.RandomState(700 + stride_bytes + seed)
    c = rs.uniform(1, 9, (900, w)).astype(np.float32)
    c[:, :3] = rs.uniform(-1, 1, (900, 3)) * (3.0, 3.0, 1.0)
    return c


_cases = None


def cases():
    """{name: (cloud, leaf)}; the arrays are shared: do not write to them"""
    global _cases
    if _cases is not None:
        return _cases
    d = {}
    for leaf in BOUNDARY_LEAVES:
        d[f"boundaries_{leaf}"] = (boundaries(leaf), leaf)
    d["order"] = (order(), ORDER_LEAF)
    d["one_voxel"] = (one_voxel(), 0.4)
    d["all_distinct"] = (all_distinct(), 0.5)
    d["nonfinite_mixed"] = (nonfinite_mixed(), 0.4)
    d["nonfinite_all"] = (nonfinite_all(), 0.4)
    d["nonfinite_fields"] = (nonfinite_fields(), 0.4)
    d["subnormal"] = (subnormal(), 0.4)
    d["subnormal_leaf"] = (subnormal(max_m=(1 << 23) - 1, n=40, seed=1), 2.0 ** -127)   # 1 / leaf = 2^127: voxels -2 .. 1
    d["index_below_2_31"] = (index_cloud((2047, 1023, 1022)), 1.0)
    d["index_2_31"] = (index_cloud((2047, 1023, 1023)), 1.0)
    one = np.zeros((1, 8), np.float32); one[0, 0] = -2147483648.0; one[0, 4] = 7
    d["index_min_int"] = (one, 1.0)
    d["index_inf_inv"] = (_random_cloud(200, 800), 1e-39)
    for s in STRIDES:
        d[f"stride_{s}"] = (strided(s), 0.4)
    for n in SIZES:
        d[f"size_{n}"] = (sized(n), 0.4)
    for c, _ in d.values():
        c.setflags(write=False)
    _cases = d
    return d


def names(prefixes=None):
    return [k for k in cases() if prefixes is None or k.startswith(tuple(prefixes))]


# ---- the filter once more: float64 and integers around the fp32 operations that decide the bits -----------------------------------

def voxel_index(cloud, leaf):
    """(finite rows, their integer voxel coordinates before min_b is taken off) -- np.floor of the fp32 product p * (1 / leaf)"""
    c = np.ascontiguousarray(cloud, np.float32)
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / np.float32(leaf)
        fin = np.isfinite(c[:, :3]).all(1)
        return np.nonzero(fin)[0], np.floor(c[fin, :3] * inv)


def restate(cloud, leaf):
    """PCL's VoxelGrid as the checker states it: None when the voxel index leaves int32 (the input comes back unchanged)"""
    c = np.ascontiguousarray(cloud, np.float32)
    rows, f = voxel_index(c, leaf)
    if rows.size == 0:
        return c[:0].copy()
    lo, hi = f.min(0).astype(np.float64), f.max(0).astype(np.float64)
    if not (np.all(lo >= -2147483648.0) and np.all(hi <= 2147483520.0)):       # (NaN fails)
        return None
    minb = [int(x) for x in lo]
    div = [int(h) - m + 1 for h, m in zip(hi, minb)]
    if max(div) > 2 ** 31 - 1 or div[0] * div[1] > 2 ** 31 - 1 or div[0] * div[1] * div[2] > 2 ** 31 - 1:
        return None
    ijk = f.astype(np.int64) - np.array(minb, np.int64)
    srt = np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))                        # by z, then y, then x; stable: input order inside a voxel
    ijk, rows = ijk[srt], rows[srt]
    head = np.ones(rows.size, bool); head[1:] = (ijk[1:] != ijk[:-1]).any(1)
    start = np.nonzero(head)[0]
    count = np.diff(np.append(start, rows.size))
    has_i = c.shape[1] >= 5
    vals = c[rows][:, [0, 1, 2, 4]] if has_i else c[rows][:, :3]
    acc = np.zeros((start.size, vals.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for r in range(int(count.max())):                                      # sequential fp32 sums, every voxel at its r-th point
            m = count > r
            acc[m] = acc[m] + vals[start[m] + r]
        acc = acc / count.astype(np.float32)[:, None]
    out = np.zeros((start.size, c.shape[1]), np.float32)
    out[:, :3] = acc[:, :3]
    if has_i:
        out[:, 4] = acc[:, 3]
    return out


def same_bits(got, want):
    """equal shapes; equal bits wherever `want` is not NaN, NaN (of any payload) where it is"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.isnan(got[nan]).all() and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))

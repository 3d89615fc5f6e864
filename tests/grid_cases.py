"""The named grids of the grid contract and, per grid, ONE point cloud that reaches every place the descriptor kernels can go wrong on
it (tests/test_grid_cases.py checks on the CPU that it does; tests/test_gpu_grids.py runs the engine on it).

A cloud (at most 30 000 points, records of 8 floats like synth_scan's) holds
  - a synth_scan;
  - points ON every ring boundary and every sector boundary of the grid and 1, 2 float steps either side of each;
  - points 0.9, 1.1 and 2 guard widths either side of every boundary (the fast binning's guard bands: inside one a point takes the
    reference's chain, outside the cheap quotients -- csrc/device_common.hpp);
  - the special values of test_gpu_make_sc.py::test_edge_points_and_strides;
  - points in the first and last ring and the first and last sector, and just inside and outside max_radius.
Every generated point has a z of its own, so a point in the wrong cell shows in that cell's maximum."""
import numpy as np

from scl_slam_amd.synth import synth_scan

MAX_RADIUS = 80.0
# the largest num_ring scl_create takes at 224 sectors (csrc/grid_limits.hpp; tests/cpp/grid_limits_check.cpp asserts the literal):
# 4 * (R * 225 + 226) + 24 * 224 + 256 bytes of LDS <= 163840
RMAX_224 = 174

GRIDS = [
    (20, 60), (64, 120), (80, 180),      # the three baseline grids
    (7, 13), (22, 50),                   # R % 4 != 0 (ring-group padding), S % 4 != 0 (no alignment image)
    (1, 2),
    (5, 128), (5, 129),                  # two threads per column while 2 S <= 256
    (33, 192), (33, 193),                # word 6 of the sector mask: the bound E up to 192 sectors, sector bits beyond
    (16, 224),                           # the last sector bit
    (256, 40),                           # 10 240 cells: the 8 192-point slice; 64 ring groups
    (RMAX_224, 224),                     # the LDS edge of the scatter's and the ingest's launch
]
SEARCH_GRIDS = [(7, 13), (5, 129), (33, 193), (256, 40), (RMAX_224, 224)]
REFUSED_GRIDS = [(1, 1), (16, 225), (20, 1024), (256, 224), (RMAX_224 + 1, 224)]

SPECIAL_POINTS = np.array(
    [[0, 0, 1.0], [80.0, 0, 2.0], [80.00001, 0, 9.0], [10, 10, -5.0], [10, 10, -2000.0],
     [0, 5, 1.0], [-5, 0, 1.0], [0, -5, 1.0], [np.nan, 1, 1], [1, 1, np.nan], [np.inf, 0, 3],
     [1e-30, 1e-30, 0.5], [-1e-3, -1e-3, 0.25], [79.999, -0.0001, 4.0],
     [-0.0, 3.0, 1.5], [-0.0, -3.0, 1.25], [3.0, -0.0, 1.75], [-3.0, -0.0, 0.75], [-0.0, -0.0, 2.5], [0.0, -0.0, 2.25],
     [np.inf, np.inf, 1.0], [-np.inf, 2.0, 1.0], [1e-40, 1e-42, 0.6], [-1e-40, 3e-41, 0.7], [30.0, 30.0, 1.0], [30.0, 13.125, 1.1],
     [30.0, 20.625, 1.2], [30.0, 35.625, 1.3], [30.0, 73.125, 1.4], [1.0, 4e7, 1.5], [-2.0, 7e7, 1.6]], dtype=np.float32)


def guard_ring(R):
    """the ring guard of the fast binning on R rings, in float32 as the device forms it (device_common.hpp: bin_guard_ring)"""
    return np.float32(1.0e-4) * (np.float32(R) / np.float32(80.0) if R > 80 else np.float32(1.0))


def guard_sect(S):
    return np.float32(2.5e-4) * (np.float32(S) / np.float32(180.0) if S > 180 else np.float32(1.0))


def ring_quotient(cloud, R, max_radius=MAX_RADIUS):
    """range / max_radius * R of every point, in float64 from the stored float32 coordinates"""
    x, y = cloud[:, 0].astype(np.float64), cloud[:, 1].astype(np.float64)
    return np.sqrt(x * x + y * y) / max_radius * R


def sector_quotient(cloud, S):
    x, y = cloud[:, 0].astype(np.float64), cloud[:, 1].astype(np.float64)
    return np.mod(np.arctan2(y, x), 2.0 * np.pi) / (2.0 * np.pi) * S


def _polar(q_ring, q_sect, R, S, max_radius):
    r = np.asarray(q_ring, np.float64) * max_radius / R
    a = np.asarray(q_sect, np.float64) * (2.0 * np.pi / S)
    return (r * np.cos(a)).astype(np.float32), (r * np.sin(a)).astype(np.float32)


def _steps(x, y, k):
    """both coordinates k float steps away from zero (k < 0: towards it): the point moves along its ray"""
    for _ in range(abs(k)):
        x = np.nextafter(x, np.copysign(np.float32(np.inf), x) if k > 0 else np.float32(0))
        y = np.nextafter(y, np.copysign(np.float32(np.inf), y) if k > 0 else np.float32(0))
    return x, y


_CACHE = {}


def grid_cloud(R, S, max_radius=MAX_RADIUS):
    """the cloud of grid R x S (computed once; callers must not write to it)"""
    key = (R, S, max_radius)
    if key in _CACHE:
        return _CACHE[key]
    rs = np.random.RandomState(1000 * R + S)
    gr, gs = float(guard_ring(R)), float(guard_sect(S))
    xs, ys = [], []

    def add(x, y):
        xs.append(np.asarray(x, np.float32).reshape(-1)); ys.append(np.asarray(y, np.float32).reshape(-1))

    # ring boundaries 1 .. R at ka angles each (mid-sector, so the sector is not in question): on it, float steps and guard widths either side
    ka = max(4, -(-128 // R))
    b = np.repeat(np.arange(1, R + 1, dtype=np.float64), ka)
    qs = (rs.randint(0, S, size=b.size) + rs.uniform(0.2, 0.8, size=b.size))
    x0, y0 = _polar(b, qs, R, S, max_radius)
    for k in (0, 1, 2, -1, -2):
        add(*_steps(x0, y0, k))
    for w in (0.9, 1.1, 2.0):
        for side in (1.0, -1.0):
            add(*_polar(b + side * w * gr, qs, R, S, max_radius))
    # sector boundaries 0 .. S - 1 at kr ranges each (mid-ring), likewise; steps on ONE coordinate turn the point
    kr = max(4, -(-128 // S))
    c = np.repeat(np.arange(0, S, dtype=np.float64), kr)
    qr = (rs.randint(0, R, size=c.size) + rs.uniform(0.2, 0.8, size=c.size))
    x0, y0 = _polar(qr, c, R, S, max_radius)
    add(x0, y0)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    add(np.nextafter(x0, up), y0); add(np.nextafter(x0, down), y0); add(x0, np.nextafter(y0, up)); add(x0, np.nextafter(y0, down))
    add(np.nextafter(np.nextafter(x0, up), up), y0); add(x0, np.nextafter(np.nextafter(y0, down), down))
    for w in (0.9, 1.1, 2.0):
        for side in (1.0, -1.0):
            add(*_polar(qr, np.mod(c + side * w * gs, S), R, S, max_radius))
    # the first and the last ring, the first and the last sector; just inside and outside max_radius
    m = 48
    add(*_polar(rs.uniform(0.05, 0.95, m), rs.uniform(0, S, m), R, S, max_radius))
    add(*_polar(R - rs.uniform(0.05, 0.95, m), rs.uniform(0, S, m), R, S, max_radius))
    add(*_polar(rs.uniform(0.05, R - 0.05, m), rs.uniform(0.05, 0.95, m), R, S, max_radius))
    add(*_polar(rs.uniform(0.05, R - 0.05, m), S - rs.uniform(0.05, 0.95, m), R, S, max_radius))
    add(*_polar(R * (1.0 + np.array([-1e-3, -1e-5, -1e-6, -2e-7, 2e-7, 1e-6, 1e-5, 1e-3])[:, None] * np.ones(6)).reshape(-1),
                rs.uniform(0, S, 48), R, S, max_radius))
    gx, gy = np.concatenate(xs), np.concatenate(ys)
    gen = np.zeros((gx.size, 8), np.float32)
    gen[:, 0] = gx; gen[:, 1] = gy; gen[:, 2] = rs.uniform(-1.5, 10.0, gx.size).astype(np.float32)
    special = np.zeros((len(SPECIAL_POINTS), 8), np.float32); special[:, :3] = SPECIAL_POINTS
    n_scan = 30000 - gen.shape[0] - special.shape[0]
    assert n_scan >= 4000, (R, S, gen.shape[0])
    cloud = np.concatenate([synth_scan(min(n_scan, 12000), seed=R * 7 + S), gen, special])
    cloud = np.ascontiguousarray(cloud[rs.permutation(cloud.shape[0])])      # (slices of it are ragged clouds of every kind of point)
    cloud.setflags(write=False)
    _CACHE[key] = cloud
    return cloud


def rotated(cloud, sectors, S):
    """the cloud turned about z by whole sectors (a revisit: the same place seen under another heading)"""
    a = sectors * 2.0 * np.pi / S
    out = cloud.copy()
    x, y = cloud[:, 0].astype(np.float64), cloud[:, 1].astype(np.float64)
    out[:, 0] = (x * np.cos(a) - y * np.sin(a)).astype(np.float32); out[:, 1] = (x * np.sin(a) + y * np.cos(a)).astype(np.float32)
    return out

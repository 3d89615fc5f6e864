#!/usr/bin/env python
"""The global voxel map (scl_map_*) on a synthetic overlapping trajectory: one JSON line.

Per size N x P (N keyframes of P points, scans of scl_slam_amd.synth.synth_scan placed one metre apart on a circle, so that every
keyframe overlaps dozens of others): building the map from the keyframe store, re-posing 1 % and 100 % of the keyframes (every pose
moved by a few centimetres, as an optimisation does), extracting everything and extracting a box, and the occupied voxels.  Wall
times are host clocks around calls that end in a device synchronise, medians over --reps; the device times of scl_map_last_timing are
taken in further repetitions under scl_profile_enable(1).  adds_per_s = 4 integer atomic adds per point and pass over the device time of
the whole integration (reserve pass and add pass: a lower bound of the add pass's own rate).

Baselines.  Device: the route the map replaces, scl_submap_from_store -- the same stored clouds, float poses, one call holding every
point, int32 voxel index -- on the --baseline-n first keyframes, where its index still fits, and on a --overflow-radius circle, where
it does not and the call hands back its input unfiltered.  Host: the CPU checker's pcl::VoxelGrid (oracle/icp_oracle.c,
icpo_transform + icpo_voxel_grid) on the same --baseline-n keyframes.

    python scripts/bench_map.py [--sizes 1000x20000 2000x100000] [--reps 5] [--leaf 0.4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scl_slam_amd import ScanContextEngine                # noqa: E402
from scl_slam_amd.synth import synth_scan                 # noqa: E402

POOL = 8                                                  # distinct scans; keyframe k stores scan k % POOL


def trajectory(n, radius, seed=0):
    """n poses (x, y, z, qx, qy, qz, qw) one metre apart on a circle of `radius`, heading along it, a little roll / pitch noise"""
    rs = np.random.RandomState(seed)
    a = np.arange(n) / radius
    yaw = a + np.pi / 2
    tilt = rs.uniform(-0.01, 0.01, (n, 2))
    q = np.stack([tilt[:, 0], tilt[:, 1], np.sin(yaw / 2), np.cos(yaw / 2)], axis=1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([np.stack([radius * np.cos(a), radius * np.sin(a), 0.05 * rs.standard_normal(n)], axis=1), q], axis=1)


def nudged(poses, seed):
    """every pose a few centimetres and milliradians elsewhere: what an optimisation does to a trajectory"""
    rs = np.random.RandomState(seed)
    out = poses.copy()
    out[:, :3] += 0.03 * rs.standard_normal((len(poses), 3))
    out[:, 3:] += 0.002 * rs.standard_normal((len(poses), 4))
    out[:, 3:] /= np.linalg.norm(out[:, 3:], axis=1, keepdims=True)
    return out


def pose_matrix32(p):
    x, y, z, w = p[3:] / np.linalg.norm(p[3:])
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = p[:3]
    return T.astype(np.float32)


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def run_size(n, p, leaf, reps, radius):
    e = ScanContextEngine(initial_capacity=16)
    pool = [synth_scan(p, seed=100 + k, stride_floats=4) for k in range(POOL)]
    for k in range(n):
        e.keyframe_put(0, k, pool[k % POOL])
    robots = np.zeros(n, np.int32); idx = np.arange(n, dtype=np.int32)
    poses = [trajectory(n, radius), None, None]
    poses[1] = nudged(poses[0], 1); poses[2] = nudged(poses[0], 2)
    one = np.arange(0, n, 100)                                          # 1 % of the keyframes, spread over the trajectory
    row = {"keyframes": n, "points_per_keyframe": p, "points": n * p, "radius_m": radius}

    def build():
        e.map_reset(leaf)
        e.map_set_keyframes(robots, idx, poses[0])
    build()                                                             # warm-up: code objects, the table's growths, the buffers
    st = e.map_stats().as_dict()
    row.update(occupied_voxels=st["occupied_voxels"], capacity=st["capacity"], growths_from_default=st["growths"],
               points_added=st["points_added"], points_skipped=st["points_skipped"])
    row["build_ms"], row["build_min_ms"] = timed(build, reps)
    flip = [0]

    def repose_all():
        flip[0] ^= 1
        e.map_set_keyframes(robots, idx, poses[1 + flip[0]])

    def repose_one():
        flip[0] ^= 1
        e.map_set_keyframes(robots[one], idx[one], poses[1 + flip[0]][one])
    repose_all()
    row["repose_100pct_ms"], row["repose_100pct_min_ms"] = timed(repose_all, reps)
    repose_one()
    row["repose_1pct_ms"], row["repose_1pct_min_ms"] = timed(repose_one, max(reps, 9))
    row["repose_1pct_keyframes"] = int(len(one))
    # device times (scl_map_last_timing): a fresh build from the default table (its growths and repeated reserve passes included), the
    # first re-pose of everything (new voxels: the table may grow), a later one back to poses it has seen (every key has its slot), and
    # the same keyframes added back into a table that still holds their keys (no insert, no growth)
    e.profile_enable(1)
    dev = {"build_integrate": [], "build_grow": [], "first_repose_100pct": [], "repose_100pct": [], "repose_100pct_grow": [], "readd": [], "extract": [],
           "extract_box": []}
    for _ in range(reps):
        e.map_reset(leaf)
        e.map_set_keyframes(robots, idx, poses[0]); t = e.map_last_timing(); dev["build_integrate"].append(t[0]); dev["build_grow"].append(t[1])
        e.map_set_keyframes(robots, idx, poses[1]); dev["first_repose_100pct"].append(sum(e.map_last_timing()[:2]))    # may grow the table
        e.map_set_keyframes(robots, idx, poses[2])
        e.map_set_keyframes(robots, idx, poses[1]); t = e.map_last_timing(); dev["repose_100pct"].append(t[0]); dev["repose_100pct_grow"].append(t[1])
        e.map_set_keyframes(robots, idx, poses[0])
        e.map_remove_keyframes(robots, idx)
        e.map_set_keyframes(robots, idx, poses[0]); dev["readd"].append(e.map_last_timing()[0])
    box = [-radius, -radius, -5.0, 0.0, 0.0, 30.0]                      # a quarter of the site
    for _ in range(reps):
        e.map_extract(count_only=False); dev["extract"].append(e.map_last_timing()[2])
        e.map_extract(box); dev["extract_box"].append(e.map_last_timing()[2])
    e.profile_enable(0)
    row["extract_all_ms"], _ = timed(lambda: e.map_extract(), reps)
    row["extract_box_ms"], _ = timed(lambda: e.map_extract(box), reps)
    row["extract_box_voxels"] = e.map_extract(box, count_only=True)
    for k, v in dev.items():
        row[f"device_{k}_ms"] = float(np.median(v))
    pts = float(n * p)
    row["build_points_per_s"] = pts / ((row["device_build_integrate_ms"] + row["device_build_grow_ms"]) * 1e-3)
    row["readd_adds_per_s"] = 4 * pts / (row["device_readd_ms"] * 1e-3)              # reserve pass (lookups only) + add pass
    row["repose_adds_per_s"] = 8 * pts / (row["device_repose_100pct_ms"] * 1e-3)    # every point subtracted and added
    e.close()
    return row


def baselines(n, p, leaf, reps, radius, overflow_radius):
    import oracle_icp_binding as oi
    e = ScanContextEngine(initial_capacity=16)
    pool = [synth_scan(p, seed=100 + k, stride_floats=4) for k in range(POOL)]
    n |= 1                                                              # a window is 2 * search_num + 1 keyframes
    for k in range(n):
        e.keyframe_put(0, k, pool[k % POOL])
    out = {"keyframes": n, "points_per_keyframe": p, "points": n * p}
    for name, r in (("fits", radius), ("overflows", overflow_radius)):
        step = 1.0 if name == "fits" else 2 * np.pi * r / n             # the large circle is walked all the way round
        poses = trajectory(n, r / step)
        poses[:, :3] *= step
        Ts = np.stack([pose_matrix32(q) for q in poses])
        call = lambda: e.submap_from_store(0, n // 2, n // 2, Ts, leaf, n * p, floats_per_point=4)
        sub = call()
        ms, mn = timed(call, reps)
        e.map_reset(leaf)
        robots = np.zeros(n, np.int32); idx = np.arange(n, dtype=np.int32)
        build = lambda: (e.map_reset(leaf), e.map_set_keyframes(robots, idx, poses))
        build()
        mms, _ = timed(build, reps)
        xms, _ = timed(lambda: e.map_extract(), reps)
        out[name] = {"radius_m": r, "submap_from_store_ms": ms, "submap_from_store_min_ms": mn, "submap_points_out": int(len(sub)),
                     "submap_returned_its_input": bool(len(sub) == n * p), "map_build_ms": mms, "map_extract_ms": xms,
                     "map_voxels": e.map_extract(count_only=True)}
        if name == "fits":
            t = time.perf_counter()
            moved = np.concatenate([oi.transform(pool[k % POOL], Ts[k]) for k in range(n)])
            host = oi.voxel_grid(moved, leaf)
            out[name]["host_icpo_transform_and_voxel_grid_ms"] = (time.perf_counter() - t) * 1e3
            out[name]["host_points_out"] = int(len(host))
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["1000x20000", "2000x100000"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leaf", type=float, default=0.4)
    ap.add_argument("--radius", type=float, default=100.0)
    ap.add_argument("--baseline-n", type=int, default=201)
    ap.add_argument("--baseline-p", type=int, default=20000)
    ap.add_argument("--overflow-radius", type=float, default=2000.0)
    ap.add_argument("--no-baselines", action="store_true")
    a = ap.parse_args()
    e = ScanContextEngine(initial_capacity=16)
    out = {"bench": "global_map", "device": e.device_name(), "leaf": a.leaf, "reps": a.reps, "sizes": {}}
    e.close()
    for s in a.sizes:
        n, p = (int(v) for v in s.split("x"))
        out["sizes"][s] = run_size(n, p, a.leaf, a.reps, max(a.radius, n / (2 * np.pi) / 4))
    if not a.no_baselines:
        out["baselines"] = baselines(a.baseline_n, a.baseline_p, a.leaf, a.reps, a.radius, a.overflow_radius)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

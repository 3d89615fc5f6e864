"""The chain from the search to the pose-graph solve (the chain of tests/test_gpu_pcm.py restated, extended by scl_pgo_optimize): five
places, inter-robot search -> guess from the shift -> guessed ICP from the store -> scoring -> scl_loop_pose_between ->
scl_loop_covariance -> scl_pcm_select with one between-pose replaced by a wrong one -> scl_pgo_optimize over the members, with the very
arrays PCM took (z, cov, and idx_a / idx_b as f_i / f_j).

The graph.  Both robots' keyframes in one array, in robot 0's world frame: poses 0 .. 4 robot 1's (A, the loops' f_i), 5 .. 9 robot 0's
(B, the loops' f_j).  Planted truth: B_k = the pose the clouds were stored at, A_k = B_k Rz_k^-1 (robot 1 saw place k turned by its
sector shift, from the same spot), so the true loop is A_k^-1 B_k = Rz_k.  Robot 0 is the mapped robot: a prior on its first keyframe,
exact odometry of covariance 1e-8.  Robot 1 drifts: every odometry step of it -- and its first pose -- is off by the same 5 cm and
10 mrad (covariance (10 mrad)^2, (5 cm)^2), so its chained odometry is 5, 10, .. 25 cm off.  That is "the drifted odometry"; robot 0's
has no error to improve on, so the comparison is over robot 1's keyframes, the wrong loop's place -- which the members leave with no
loop of its own -- among them.  A comparison takes no tolerance."""
import numpy as np
import pytest

import icp_guess_cases as gc
import pcm_cases as pc
import pgo_cases as pg
from scl_slam_amd import PgoParams, ScanContextEngine
from scl_slam_amd.synth import rigid_transform, synth_scan

pytestmark = pytest.mark.gpu
K, SECTORS, WRONG = 5, (7, 3, 11, 0, 5), 2


def _pose7(M):
    """x, y, z, qx, qy, qz, qw of a 4 x 4 rigid motion"""
    R = np.asarray(M, np.float64)[:3, :3]
    Kq = np.array([[R[0, 0] - R[1, 1] - R[2, 2], 0, 0, 0], [R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], 0, 0],
                   [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1], 0],
                   [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(Kq, UPLO="L")
    q = v[:, np.argmax(w)]
    return np.concatenate([np.asarray(M, np.float64)[:3, 3], q if q[3] >= 0 else -q])


def _errors(X, truth):
    """(translation error in metres, rotation error in radians) per pose"""
    d = pg._rel(pg.canonical(truth), pg.canonical(X))
    return np.linalg.norm(d[:, :3], axis=1), 2 * np.arctan2(np.linalg.norm(d[:, 3:6], axis=1), np.abs(d[:, 6]))


def test_the_chain_from_search_to_the_solve():
    W = rigid_transform(0.01, -0.02, 0.7, 40.0, -25.0, 0.5)              # robot 1's world frame in robot 0's
    odom_var = [1e-6] * 3 + [1e-4] * 3
    e = ScanContextEngine(num_ring=20, num_sector=60)
    try:
        clouds = [synth_scan(20000, seed=7 + 10 * k) for k in range(K)]
        poses_pre = [np.float32([14.0 + 9 * k, -6.5 + 4 * k, 0.4 - 0.1 * k, 0.02, -0.015, 1.1 + 0.3 * k]) for k in range(K)]
        for k in range(K):                                                # robot 0: descriptors and clouds, sensor frame
            e.make_and_save(clouds[k], 0, k)
            e.keyframe_put(0, k, clouds[k])
        poses_a, poses_b, zs, covs, truth_a, truth_b = [], [], [], [], [], []
        for k in range(K):
            Rz = rigid_transform(0.0, 0.0, np.radians(6.0 * SECTORS[k]), 0, 0, 0)
            M_pre = gc.pose_matrix(poses_pre[k])
            pose_cur = np.float32(e.matrix_to_pose(np.linalg.inv(W) @ M_pre @ np.linalg.inv(Rz)))   # what robot 1 believes of its keyframe
            M_cur = gc.pose_matrix(pose_cur)
            turned = clouds[k].copy()
            turned[:, :3] = (clouds[k][:, :3].astype(np.float64) @ Rz[:3, :3].T).astype(np.float32)
            received = turned.copy()
            xyz = turned[:, :3].astype(np.float64) @ M_cur[:3, :3].T + M_cur[:3, 3]
            received[:, :3] = (xyz + gc.NOISE * np.random.RandomState(90 + k).standard_normal(xyz.shape)).astype(np.float32)
            e.make_and_save(turned, 1, k)                                 # key K + k
            ids, shifts, dists, found = e.sc_search_inter([K + k], 2, robot_pre=0)
            assert found[0] >= 1 and e.get_index(int(ids[0, 0])) == (0, k) and shifts[0, 0] == SECTORS[k]
            G = e.loop_guess_from_shift(int(shifts[0, 0]), 60, pose_cur, poses_pre[k])[None]
            args = (received, gc.E2E_LEAF, 0, [k], 0, M_pre.astype(np.float32).reshape(1, 1, 4, 4), gc.E2E_LEAF)
            icp = e.icp_align_batch_from_store_guess(*args, G)
            ev = e.registration_eval_batch_from_store(*args, icp[0], 0.5)
            assert ev.overlap[0] > 0.9
            info = ev.information(0)
            s2 = ev.moments[0, 9] / max(1, int(ev.n_inliers[0]) - 6)
            zs.append(e.loop_pose_between(icp[0][0], pose_cur, poses_pre[k])[0]); covs.append(ScanContextEngine.loop_covariance(info, s2))
            poses_a.append(_pose7(M_cur)); poses_b.append(_pose7(M_pre))
            truth_b.append(_pose7(M_pre)); truth_a.append(_pose7(M_pre @ np.linalg.inv(Rz)))
        truth = np.array(truth_a + truth_b)
        idx = np.arange(K, dtype=np.int32)
        right_z = np.array(zs)
        z = right_z.copy()
        z[WRONG] = pc.compose(z[WRONG], np.concatenate([[3.0, 0.0, 0.0], pc.rotvec_to_quat([0.0, 0.0, 0.5])]))
        cov = np.array(covs).reshape(K, 36)
        mem, seed, deg = e.pcm_select(np.array(poses_a), np.array(poses_b), idx, idx, z, cov, pc.THRESHOLD, odom_var=odom_var)
        assert mem.tolist() == [k for k in range(K) if k != WRONG]
        # what the chain measured is the planted loop A_k^-1 B_k = Rz_k, in that direction: a registration on a 0.1 m voxel grid is off
        # by less than a voxel, the inverse loop by the sine of 18 degrees and more at every place but the unturned one
        want = pg._rel(truth[:K], truth[K:])
        print("the loops' deviation from the planted ones:", pg.pose_deviation(right_z, want))
        assert pg.pose_deviation(right_z, want) <= gc.E2E_LEAF

        # the graph: robot 1's drifted odometry, robot 0's exact one, a prior on robot 0's first keyframe
        bias = np.array([0.0, 0.0, 0.01, 0.05, 0.0, 0.0])                 # 10 mrad of yaw and 5 cm ahead per step
        odo_cov_a = np.diag([1e-4] * 3 + [2.5e-3] * 3).ravel(); tight = (1e-8 * np.eye(6)).ravel()
        f_i, f_j, f_z, f_cov = [], [], [], []
        for k in range(K - 1):
            f_i += [k, K + k]; f_j += [k + 1, K + k + 1]
            f_z += [pg.perturb(pg.between(truth[k], truth[k + 1]), bias), pg.between(truth[K + k], truth[K + k + 1])]
            f_cov += [odo_cov_a, tight]
        start = [pg.perturb(truth[0], bias)]
        for k in range(K - 1):
            nxt = pc.compose(start[-1], f_z[2 * k]); nxt[3:] /= np.linalg.norm(nxt[3:])
            start.append(nxt)
        start = np.array(start + [truth[K + k] for k in range(K)])
        prm = PgoParams.defaults(relative_cost_tolerance=1e-14, step_tolerance=1e-14, cg_tolerance=1e-12, cg_max_iterations=4000)

        def solve(loops):
            g = pg.graph(start, f_i + [int(idx[m]) for m in loops], f_j + [K + int(idx[m]) for m in loops],
                         np.vstack([np.array(f_z)] + [z[m][None] for m in loops]), np.vstack([np.array(f_cov)] + [cov[m][None] for m in loops]),
                         [K], truth[K][None], tight[None])
            X, res, chi2 = e.pgo_optimize(*g, params=prm)
            assert res.final_cost < res.initial_cost and res.accepted >= 1
            return X, res, chi2
        X, res, chi2 = solve(mem)
        t0, r0 = _errors(start, truth)
        t1, r1 = _errors(X, truth)
        print("drifted odometry, robot 1: ", t0[:K], r0[:K], "\noptimised over the members:", t1[:K], r1[:K], "\nrobot 0:", t1[K:], r1[K:])
        assert (t1[:K] < t0[:K]).all() and (r1[:K] < r0[:K]).all()        # closer to the truth at every keyframe of the drifting robot
        assert t1[K:].max() < t0[:K].min() and r1[K:].max() < r0[:K].min()   # and the mapped robot moved by less than one step's drift
        # with the wrong loop among the factors: worse, and worst where it sits
        Xw, resw, _ = solve(list(range(K)))
        tw, rw = _errors(Xw, truth)
        print("with the rejected loop:    ", tw[:K], rw[:K])
        assert tw[WRONG] > t1[WRONG] and rw[WRONG] > r1[WRONG] and tw[:K].sum() > t1[:K].sum() and rw[:K].sum() > r1[:K].sum()
        assert tw[WRONG] > t0[WRONG]                                      # worse than not having optimised at all
    finally:
        e.close()

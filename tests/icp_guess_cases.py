"""Named inputs for the batched ICP with one initial guess per candidate (include/scl_engine.h "THE BATCHED ICP WITH INITIAL
GUESSES"; numpy only).

ONE source (a place seen by its sensor: every second point of a structured cloud, 1 cm of noise) against candidates that are the
same place in other frames: candidate c's cloud is the place moved by TRUE[c], so TRUE[c] is the motion source -> candidate.  Its
guess is what a caller with a Scan Context yaw and two odometry poses would pass: TRUE[c] behind a small error motion (ERR), so
that the alignment has something left to do.  The yaws are 0, about 90 and about 180 degrees, the translations tens of metres: the
candidates' moved sources have different boxes, and therefore different working orders.

  near      TRUE is a few centimetres and degrees; guess = identity (the unguessed call's case)
  yaw90     91.3 degrees, (12, -31, 0.4) m; guess 2 degrees and 0.25 m off
  yaw180    179 degrees, (-27, 18, -0.3) m; guess -1.5 degrees and 0.3 m off
  tight90   yaw90's cloud; guess 0.15 degrees and 5 cm off: the one a 0.5 m rejection distance can start from
  far       yaw90's cloud; guess 12 m too high (the cloud is 6 m tall): under a 0.5 m rejection distance no pair at the first
            search.  (12 and not 50 m: the checker's grid walk for sources far outside the target's box takes seconds per metre)

PARAMS names the parameter sets the whole list is run under.  CHECKED lists the (candidate, parameter set) pairs that are held to the
CPU checker; tests/test_icp_guess_cases.py proves with the checker alone that each is off every knife edge (the method of
tests/icp_param_cases.py), and for the YAWED ones that the alignment fails without the guess and succeeds with it.  The other
pairs (a loose guess under a 0.5 m rejection distance ends wherever its few pairs take it) are held to the single call bit for bit
only.

end_to_end() is the 20 x 60 chain's input: two robots, the received keyframe seen with the sensor turned by seven sectors."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from icp_param_cases import FIT_REL, TOL, jittered, oracle_params  # noqa: F401  (the bars of tests/test_gpu_icp_params.py)
from scl_slam_amd.synth import rigid_transform, synth_scan, synth_structured_cloud

FITNESS_MAX = 0.3                                                    # historyKeyframeFitnessScore, DM.h:192
T_TRUE_TOL = 5e-3                                                    # tests/test_gpu_icp.py, test_icp_align_matches_oracle
JITTER_TOL = 5e-6
NOISE = 0.01
NAMES = ("near", "yaw90", "yaw180", "tight90", "far")
_T90 = rigid_transform(0.01, -0.02, np.radians(91.3), 12.0, -31.0, 0.4)
_T180 = rigid_transform(-0.015, 0.01, np.radians(179.0), -27.0, 18.0, -0.3)
TRUE = {"near": rigid_transform(0.01, -0.02, 0.05, 0.3, -0.2, 0.1), "yaw90": _T90, "yaw180": _T180, "tight90": _T90, "far": _T90}
ERR = {"yaw90": rigid_transform(0.004, -0.003, np.radians(2.0), 0.25, -0.15, 0.05),
       "yaw180": rigid_transform(-0.002, 0.005, np.radians(-1.5), -0.2, 0.3, -0.04),
       "tight90": rigid_transform(0.0005, -0.0004, np.radians(0.15), 0.05, -0.03, 0.01),
       "far": rigid_transform(0.0, 0.0, 0.0, 0.0, 0.0, 12.0)}
PARAMS = {"p2p": {}, "plane": {"estimator": 1, "normal_radius": 1.5}, "mcd0.5": {"max_correspondence_dist": 0.5}}
YAWED = (("yaw90", "p2p"), ("yaw180", "p2p"), ("yaw90", "plane"), ("yaw180", "plane"), ("tight90", "mcd0.5"))
CHECKED = YAWED + (("near", "p2p"), ("near", "plane"), ("tight90", "p2p"), ("far", "mcd0.5"))


def moved(cloud, T):
    """the cloud's x, y, z moved by T in double, rounded once (how the inputs are MADE; the calls move clouds in float32)"""
    out = cloud.copy()
    out[:, :3] = (cloud[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def place():
    return synth_structured_cloud(6000, seed=21)


@functools.lru_cache(maxsize=None)
def source():
    src = place()[::2].copy()
    src[:, :3] += (NOISE * np.random.RandomState(5).standard_normal((src.shape[0], 3))).astype(np.float32)
    return src


@functools.lru_cache(maxsize=None)
def targets():
    """candidate clouds, in NAMES' order (yaw90, tight90 and far share one cloud, as three keys of a list may share a place)"""
    made = {}
    out = []
    for n in NAMES:
        key = TRUE[n].tobytes()
        if key not in made:
            made[key] = np.ascontiguousarray(moved(place(), TRUE[n]))
        out.append(made[key])
    return out


@functools.lru_cache(maxsize=None)
def guesses():
    """(5, 4, 4) float32, in NAMES' order"""
    return np.stack([(ERR[n] @ TRUE[n] if n in ERR else np.eye(4)).astype(np.float32) for n in NAMES])


def compose(T_icp, G):
    """T_icp * G with G's last row taken as (0, 0, 0, 1): ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in double, rounded once"""
    out = np.empty((4, 4), np.float32)
    for r in range(4):
        a0, a1, a2, a3 = (float(v) for v in T_icp[r])
        for c in range(4):
            b0, b1, b2, b3 = float(G[0, c]), float(G[1, c]), float(G[2, c]), (1.0 if c == 3 else 0.0)
            out[r, c] = np.float32(((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3)
    return out


# ---- checker results, each computed once ------------------------------------------------------------------------------------------
_results = {}


def _run(name, pname, guessed, jitter):
    import oracle_icp_binding as oi
    src = source() if jitter is None else jittered(source(), jitter)
    k = NAMES.index(name)
    if guessed:
        src = oi.transform(src, guesses()[k])
    return oi.icp_align(src, targets()[k], oracle_params(PARAMS[pname]))


def oracle_many(requests, workers=8):
    """requests: (candidate name, parameter set, guessed, jitter seed or None) -> the checker's (T_icp, fitness, converged,
    iterations) of icpo_icp_align(icpo_transform(source, G), target), or of the unmoved source where guessed is False"""
    todo = [r for r in dict.fromkeys(requests) if r not in _results]
    if todo:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            for r, res in zip(todo, pool.map(lambda a: _run(*a), todo)):
                _results[r] = res
    return [_results[r] for r in requests]


def oracle(name, pname, guessed=True, jitter=None):
    return oracle_many([(name, pname, guessed, jitter)])[0]


# ---- the 20 x 60 chain --------------------------------------------------------------------------------------------------------------
SECTORS_TURNED = 7
E2E_LEAF = 0.1
POSE_PRE = np.float32([14.0, -6.5, 0.4, 0.02, -0.015, 1.1])          # x, y, z, roll, pitch, yaw of robot 0's keyframe 1
POSE_CUR = np.float32([-35.0, 22.0, -0.3, -0.01, 0.025, -2.3])       # ... of the received keyframe in robot 1's world frame


def pose_matrix(pose):
    x, y, z, roll, pitch, yaw = (float(v) for v in pose)
    return rigid_transform(roll, pitch, yaw, x, y, z)


@functools.lru_cache(maxsize=None)
def end_to_end():
    """(cloud, other, turned, received, T_true): robot 0's keyframe 1 in its sensor frame, its keyframe 0 (another place), keyframe 1's
    place seen with the sensor turned by seven sectors (the received keyframe's descriptor), that scan in robot 1's world frame with
    1 cm of noise (what robot 1 sends, DM.h:1333), and the motion received cloud -> the candidate's submap in robot 0's world frame"""
    cloud = synth_scan(20000, seed=7)
    other = synth_scan(20000, seed=11)
    Rz = rigid_transform(0.0, 0.0, np.radians(SECTORS_TURNED * 6.0), 0, 0, 0)
    turned = cloud.copy()
    turned[:, :3] = (cloud[:, :3].astype(np.float64) @ Rz[:3, :3].T).astype(np.float32)
    M_pre, M_cur = pose_matrix(POSE_PRE), pose_matrix(POSE_CUR)
    received = turned.copy()
    xyz = turned[:, :3].astype(np.float64) @ M_cur[:3, :3].T + M_cur[:3, 3]
    received[:, :3] = (xyz + NOISE * np.random.RandomState(9).standard_normal(xyz.shape)).astype(np.float32)
    T_true = M_pre @ np.linalg.inv(Rz) @ np.linalg.inv(M_cur)
    return cloud, other, turned, received, T_true

"""The list of tests/verification_batch_cases.py with an initial guess per candidate, for the guessed batched verification
(include/scl_engine.h "THE BATCHED VERIFICATION WITH INITIAL GUESSES"; numpy only).

The received scan is verification_batch_cases' (2 000 rows, 5 of them non-finite).  The candidates are that list plus `moved_6dof`,
the scan's place moved by a full 6-DoF motion.  Candidate c's guess is what a caller with the right yaw (or pose) would pass:
the identity where the clouds already agree, Rz of the candidate's own turn for yaw_3 / yaw_20 / yaw_90, the 6-DoF motion for
moved_6dof -- and a deliberately wrong Rz(17 deg) for matching_again, so that two equal clouds answer differently and a batch that
reads candidate c + 1's guess (or none) cannot pass.  first_3, first_1 and empty get arbitrary finite guesses.

tests/test_verification_guess_cases.py pins the list on the CPU checker, tests/test_gpu_verification_guess.py holds the guessed
calls to the single calls on the moved scan, bit for bit, and to the checker."""
import numpy as np

import verification_batch_cases as bc
from scl_slam_amd.synth import rigid_transform

ITERATIONS = bc.ITERATIONS
THRESHOLD, RATIO, SEED = bc.THRESHOLD, bc.RATIO, bc.SEED
N_NONFINITE = bc.N_NONFINITE
MOTION_6DOF = (0.05, -0.08, 0.6, 4.0, -7.5, 1.25)                    # roll, pitch, yaw (rad), x, y, z (m)

source, finite_source = bc.source, bc.finite_source
_cache = {}


def rz(degrees):
    return rigid_transform(0.0, 0.0, np.radians(degrees), 0, 0, 0).astype(np.float32)


def _moved(cloud, T):
    out = cloud.copy()
    out[:, :3] = (cloud[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return out


def candidates():
    """[(name, cloud, guess)] in the order the batch takes them; guess = float32 4x4"""
    if "candidates" not in _cache:
        ident = np.eye(4, dtype=np.float32)
        M = rigid_transform(*MOTION_6DOF)
        guess = {"matching": ident, "permuted": ident, "yaw_3": rz(3.0), "yaw_20": rz(20.0), "yaw_90": rz(90.0),
                 "other_place": rz(-5.0), "half_moved": ident, "first_257": ident, "first_256": rz(0.5),
                 "first_3": rigid_transform(0.3, -0.2, 2.0, -3.0, 11.0, 0.5).astype(np.float32),
                 "first_1": (rigid_transform(0.0, 0.0, -1.0, 100.0, 0.0, 0.0) * 1.5).astype(np.float32),   # not even rigid
                 "empty": np.arange(16, dtype=np.float32).reshape(4, 4) - 7.0,
                 "matching_again": rz(17.0), "moved_6dof": M.astype(np.float32)}
        cs = list(bc.candidates()) + [("moved_6dof", np.ascontiguousarray(_moved(bc.target(), M)))]
        _cache["candidates"] = [(n, c, np.ascontiguousarray(guess[n])) for n, c in cs]
    return _cache["candidates"]


def names():
    return [n for n, _, _ in candidates()]


def clouds():
    return [c for _, c, _ in candidates()]


def guesses():
    """(m, 4, 4) float32"""
    return np.stack([g for _, _, g in candidates()])

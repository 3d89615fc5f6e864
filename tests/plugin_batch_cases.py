"""What the batched-detection test modules share (tests/test_plugin_batch_cases.py, tests/test_gpu_plugin_detect_many.py): GRSD rows
from the wire and a restatement of the GRSD detections (include/scl_grsd.h) -- FPFH's rules with DIM = report dims = 21 and a
threshold of 160 -- on plugin_cases.sq_dist_rows and first_minimum.  A plain module, no fixtures."""
import numpy as np

from plugin_cases import FpfhChecker, M2dpChecker, first_minimum, same_detection, sq_dist_rows, vector_rows  # noqa: F401

GRSD_DIM = 21
HEADERS = {"m2dp": "scl_m2dp.h", "fpfh": "scl_fpfh.h", "grsd": "scl_grsd.h"}
BATCH_CALLS = ("detect_intra_many", "detect_inter_many", "save_from_wire_many", "make_save_and_detect")


def grsd_rows(n, seed):
    """n rows of 21 non-negative floats shaped like transition counts (whole numbers, most mass on a few class pairs); 10 % exact
    copies of row 0 (ties)"""
    rs = np.random.RandomState(seed)
    scale = np.array([400, 60, 30, 10, 20, 300] + [25] * 15, np.float64)
    rows = np.floor(rs.gamma(2.0, 1.0, size=(n, GRSD_DIM)) * scale).astype(np.float32)
    rows[rs.rand(n) < 0.10] = rows[0]
    return np.ascontiguousarray(rows, np.float32)


def plugin_rows(plugin, n, seed):
    return grsd_rows(n, seed) if plugin == "grsd" else vector_rows(plugin, n, seed)


class GrsdChecker(FpfhChecker):
    """plugin_cases.FpfhChecker over rows of 21 floats: every rule of scl_grsd.h's detections is FPFH's with the reported distance
    over all 21 floats (sqrtf of the 1-NN's own squared distance) and dist_thres = 160"""

    def __init__(self, dist_thres=160.0, **kw):
        kw.pop("report_dims", None)
        super().__init__(dist_thres=dist_thres, report_dims=GRSD_DIM, **kw)

    def save(self, values, robot=0, index=0):
        assert np.asarray(values).size == GRSD_DIM
        super().save(values, robot, index)

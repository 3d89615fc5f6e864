"""What the candidate-list test modules share (tests/test_plugin_topk_cases.py, tests/test_gpu_plugin_topk.py): the checker top-k on
plugin_cases.sq_dist_rows and a model of a vector plugin's handle (the search sets of scl_plugin_batch.h, the state of the
reference's inter mode) that answers detect_*_topk.  A plain module, no fixtures."""
import numpy as np

from plugin_batch_cases import HEADERS, plugin_rows  # noqa: F401
from plugin_cases import sq_dist_rows

TOPK_MAX = 32
TOPK_CALLS = ("detect_intra_topk", "detect_inter_topk")
DIMS = {"m2dp": 192, "fpfh": 33, "grsd": 21}


def checker_topk(q, cands, k, report_dims=None):
    """the k nearest rows of cands to q: NaN sums dropped, a stable sort by (float bits of the sum, position), the first k.
    Returns (positions int64, sums float32, reported distances float32: sqrtf of the sum over the first report_dims floats)"""
    cands = np.asarray(cands, np.float32).reshape(-1, np.asarray(q).size)
    s = sq_dist_rows(q, cands)
    pos = np.flatnonzero(~np.isnan(s))
    pos = pos[np.argsort(s[pos].view(np.uint32), kind="stable")][:k]
    with np.errstate(invalid="ignore", over="ignore"):
        rep = np.sqrt(sq_dist_rows(q, cands[pos], report_dims)) if pos.size else np.zeros(0, np.float32)
    return pos, s[pos], rep.astype(np.float32)


class TopkModel:
    """A vector plugin's handle as scl_plugin_batch.h describes it: rows with their robots, the search sets of the detections and, for
    inter_mode 0, the call counter and the snapshot.  topk(form, curs, k) answers what scl_X_detect_<form>_topk answers"""

    def __init__(self, plugin, num_exclude_recent=30, tree_making_period=10, inter_mode=0, robot_num=1, this_id=0, report_dims=None):
        self.plugin, self.dim = plugin, DIMS[plugin]
        self.excl, self.period, self.robot_num, self.this_id = num_exclude_recent, tree_making_period, robot_num, this_id
        self.mode = 1 if plugin == "m2dp" else inter_mode
        self.rdims = (report_dims or 21) if plugin == "fpfh" else self.dim
        self.rows, self.robots, self.l2g = [], [], [[] for _ in range(robot_num)]
        self.counter, self.snap_n = 0, 0
        self._mat = None

    def save_many(self, rows, robots):
        for v, r in zip(rows, robots):
            self.l2g[int(r)].append(len(self.rows)); self.rows.append(np.asarray(v, np.float32)); self.robots.append(int(r))

    def mat(self):
        if self._mat is None or self._mat.shape[0] != len(self.rows):
            self._mat = np.stack(self.rows) if self.rows else np.zeros((0, self.dim), np.float32)
        return self._mat

    def sets(self, form, curs):
        """per query (query key, searched keys in list order, ids are positions); None for the early return of inter_mode 0.
        Walks the counter and the snapshot as the call does"""
        out = []
        n = len(self.rows)
        mine = self.l2g[self.this_id]
        for cur in curs:
            cur = int(cur)
            if form == "intra":
                out.append((mine[cur], mine[:max(0, cur - self.excl)], True))
            elif self.mode == 0:
                if n < self.excl + 1:
                    out.append(None)
                    continue
                if self.counter % self.period == 0:
                    self.snap_n = n - self.excl
                self.counter += 1
                out.append((cur, list(range(self.snap_n)), False))
            elif self.robots[cur] == self.this_id:
                out.append((cur, sorted(k for r in range(self.robot_num) if r != self.this_id for k in self.l2g[r]), False))
            else:
                out.append((cur, list(mine), False))
        return out

    def topk(self, form, curs, k):
        curs = np.asarray(curs).ravel()
        ids = np.full((curs.size, k), -1, np.int32)
        dists = np.full((curs.size, k), np.inf, np.float32)
        found = np.zeros(curs.size, np.int32)
        mat = self.mat()
        for i, st in enumerate(self.sets(form, curs)):
            if st is None or not st[1]:
                continue
            q, keys, local = st
            keys = np.asarray(keys, np.int64)
            pos, _, rep = checker_topk(mat[q], mat[keys], k, self.rdims)
            found[i] = pos.size
            ids[i, :pos.size] = pos if local else keys[pos]
            dists[i, :pos.size] = rep
        return ids, dists, found


def same_lists(got, want):
    """(ids, dists, n_found) equal: ids and n_found as integers, distances by their uint32 pattern"""
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and
            np.array_equal(np.ascontiguousarray(got[1], np.float32).view(np.uint32), np.ascontiguousarray(want[1], np.float32).view(np.uint32)))

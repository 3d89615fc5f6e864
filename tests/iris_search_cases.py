"""The CPU checker of the exhaustive ranked search of the LiDAR-Iris plugin (scl_iris.h "THE EXHAUSTIVE SEARCH"; test infrastructure
only).  A World is a hand mirror of what a handle holds: per global key the robot it came from and the templates of its image, and
the two search-set rules.  A pair is scored by oracle/iris_oracle.c's iriso_hamming_all through tests/oracle_iris_binding.py; the
ranking is a plain Python sort on (float32 bits of the score, position in the search set) with the NaN pairs left out.

Keyframes are named by a `wid`: two keyframes with one wid hold the same image (a wire vector saved twice), so a pair's score is
computed once per pair of wids however many keyframes share them.
"""
import numpy as np

import oracle_iris_binding as oi

ORACLE_FIELDS = ("rows", "cols", "nscan", "nscale", "min_wavelength", "mult", "sigma_onf")
NO_ENTRY = (-1, 0.0, np.inf)                                # id, bias, distance of an unused slot


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rank(dists, k):
    """positions of the k smallest scores of `dists` (float32, NaN = no score) by (float32 bits, position)"""
    d = np.ascontiguousarray(dists, np.float32)
    keyed = sorted((int(bits(d[p:p + 1])[0]), p) for p in range(d.size) if not np.isnan(d[p]))
    return [p for _, p in keyed[:k]]


class World:
    def __init__(self, conf, robot_num=1, this_id=0, num_exclude_recent=0):
        self.conf = dict(conf)
        self.cfg = oi.config(**{f: conf[f] for f in ORACLE_FIELDS if f in conf})
        self.robot_num, self.this_id, self.num_exclude_recent = robot_num, this_id, num_exclude_recent
        self.feats, self.wires = {}, {}                     # wid -> (T, M); wid -> the wire vector (layout of wire_decode = 1)
        self.wids, self.robots = [], []                     # per global key
        self.keys_of = [[] for _ in range(robot_num)]       # per robot: its global keys in arrival order
        self._scores = {}

    # ---- what is stored
    def add_feature(self, wid, T, M):
        tr = 2 * self.cfg.nscale * self.cfg.rows
        self.feats[wid] = (np.ascontiguousarray(T, np.uint8).reshape(tr, self.cfg.cols), np.ascontiguousarray(M, np.uint8).reshape(tr, self.cfg.cols))

    def add_wire(self, wid, wire):
        """a wire vector: rows * cols image values row-major, then the row key (makeAndSaveDescriptorAndKey's layout)"""
        rows, cols = self.cfg.rows, self.cfg.cols
        w = np.ascontiguousarray(wire, np.float32)
        assert w.size == rows * cols + rows
        self.wires[wid] = w
        self.add_feature(wid, *oi.encode(self.cfg, w[:rows * cols].astype(np.uint8).reshape(rows, cols)))

    def add_cloud(self, wid, cloud):
        img, key = oi.make_image(self.cfg, cloud)
        self.add_wire(wid, np.concatenate([img.reshape(-1).astype(np.float32), key]))

    def add_blank(self, wid):
        """the all-zero image: every template bit is masked"""
        self.add_wire(wid, np.zeros(self.cfg.rows * self.cfg.cols + self.cfg.rows, np.float32))

    def push(self, wid, robot=0):
        key = len(self.wids)
        self.wids.append(wid); self.robots.append(robot); self.keys_of[robot].append(key)
        return key

    def wire_rows(self, first=0):
        """(values, robots, indexs) of the keyframes from global key `first` on, for save_from_wire_many"""
        keys = range(first, len(self.wids))
        return (np.stack([self.wires[self.wids[k]] for k in keys]), np.array([self.robots[k] for k in keys], np.int8),
                np.array(list(keys), np.int32))

    # ---- the search sets: global keys in search order
    def intra_set(self, cur):
        mine = self.keys_of[self.this_id]
        assert 0 <= cur < len(mine)
        return mine[:max(0, cur - self.num_exclude_recent)]

    def inter_set(self, key):
        assert 0 <= key < len(self.wids)
        if self.robots[key] != self.this_id:
            return list(self.keys_of[self.this_id])
        return [k for r in range(self.robot_num) if r != self.this_id for k in self.keys_of[r]]

    def query_and_set(self, mode, cur):
        """(global key of the query, global keys of its search set, the ids the call reports for them)"""
        if mode == "intra":
            keys = self.intra_set(cur)
            return self.keys_of[self.this_id][cur], keys, list(range(len(keys)))
        keys = self.inter_set(cur)
        return cur, keys, keys

    # ---- the score of a pair
    def score(self, wq, wc):
        if (wq, wc) not in self._scores:
            (T1, M1), (T2, M2) = self.feats[wq], self.feats[wc]
            d, b = oi.hamming_all(self.cfg, T1, M1, T2, M2)
            self._scores[(wq, wc)] = (np.float32(d), int(b))
        return self._scores[(wq, wc)]

    def checker_scores(self, qkey, keys):
        s = [self.score(self.wids[qkey], self.wids[c]) for c in keys]
        return np.array([d for d, _ in s], np.float32), np.array([b for _, b in s], np.int32)

    # ---- the lists
    def expected(self, mode, curs, k, scores=None):
        """(ids (count, k) int32, biases float32, dists float32, n_found int32) as scl_iris_search_intra / _inter return them;
        scores(qkey, keys) -> (dists, biases) of the query against the keys, the checker's by default"""
        scores = scores or self.checker_scores
        count = len(curs)
        ids = np.full((count, k), NO_ENTRY[0], np.int32); biases = np.full((count, k), NO_ENTRY[1], np.float32)
        dists = np.full((count, k), NO_ENTRY[2], np.float32); found = np.zeros(count, np.int32)
        for i, cur in enumerate(curs):
            qkey, keys, out_ids = self.query_and_set(mode, int(cur))
            if not keys:
                continue
            d, b = scores(qkey, keys)
            top = rank(d, k)
            found[i] = len(top)
            for j, p in enumerate(top):
                ids[i, j], biases[i, j], dists[i, j] = out_ids[p], np.float32(b[p]), d[p]
        return ids, biases, dists, found


def assert_same_lists(got, want, what=""):
    """bit for bit: ids, shifts, scores, n_found"""
    assert np.array_equal(got[3], want[3]), (what, "n_found", got[3], want[3])
    assert np.array_equal(got[0], want[0]), (what, "ids", got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1])), (what, "biases", got[1], want[1])
    assert np.array_equal(bits(got[2]), bits(want[2])), (what, "dists", got[2], want[2])

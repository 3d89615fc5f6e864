"""ctypes binding of include/scl_iris.h: the LiDAR-Iris building blocks (image, templates, Hamming matching) on the GPU."""
import ctypes
from ctypes import POINTER, byref, c_double, c_float, c_int, c_int8, c_uint8, c_void_p

import numpy as np

from ._native import load_library
from ._plugin import PluginEngine, PluginError, bind, plugin_signatures


class IrisConfig(ctypes.Structure):
    """scl_iris_config; defaults = lidar_iris_descriptor's constructor defaults (descriptor.h:473-486)"""
    _fields_ = [("rows", c_int), ("cols", c_int), ("nscan", c_int), ("nscale", c_int), ("min_wavelength", c_int),
                ("mult", c_float), ("sigma_onf", c_float), ("device", c_int),
                ("dist_thres", c_double), ("num_exclude_recent", c_int), ("match_num", c_int), ("num_candidates", c_int),
                ("robot_num", c_int), ("this_id", c_int), ("knn_exclude_eps", c_float), ("wire_decode", c_int), ("shift_search", c_int)]


_P, _u8, _fp, _ip = c_void_p, POINTER(c_uint8), POINTER(c_float), POINTER(c_int)
_SIG = plugin_signatures("scl_iris", IrisConfig)
_SIG.update({
    "scl_iris_make_image": (c_int, [_P, _P, c_int, c_int, _u8, _fp]),
    "scl_iris_make_and_save": (c_int, [_P, _P, c_int, c_int, c_int8, c_int, _fp]),
    "scl_iris_save_image": (c_int, [_P, _u8, _fp, c_int8, c_int]),
    "scl_iris_detect_intra": (c_int, [_P, c_int, _ip, _fp, _fp]),
    "scl_iris_detect_inter": (c_int, [_P, c_int, _ip, _fp, _fp]),
    "scl_iris_get_image": (c_int, [_P, c_int, _u8, _fp]),
    "scl_iris_get_feature": (c_int, [_P, c_int, _u8, _u8]),
    "scl_iris_hamming": (c_int, [_P, c_int, c_int, c_int, _fp, _ip]),
    "scl_iris_hamming_batch": (c_int, [_P, c_int, _ip, _ip, c_int, _fp, _ip]),
    "scl_iris_hamming_all_shifts": (c_int, [_P, c_int, _ip, c_int, _fp, _ip]),
    "scl_iris_fft_match": (c_int, [_P, c_int, c_int, c_int, _fp, _ip]),
    "scl_iris_compare": (c_int, [_P, c_int, _ip, c_int, _fp, _ip]),
    # the batch forms
    "scl_iris_make_and_save_many": (c_int, [_P, POINTER(c_void_p), _ip, c_int, POINTER(c_int8), _ip, c_int, _fp]),
    "scl_iris_save_from_wire_many": (c_int, [_P, _fp, POINTER(c_int8), _ip, c_int]),
    "scl_iris_detect_intra_many": (c_int, [_P, _ip, c_int, _ip, _fp, _fp]),
    "scl_iris_detect_inter_many": (c_int, [_P, _ip, c_int, _ip, _fp, _fp]),
    "scl_iris_make_save_and_detect": (c_int, [_P, POINTER(c_void_p), _ip, c_int, POINTER(c_int8), _ip, c_int, _ip, _fp, _fp, _fp]),
    # the exhaustive ranked search
    "scl_iris_search_intra": (c_int, [_P, _ip, c_int, c_int, _ip, _fp, _fp, _ip]),
    "scl_iris_search_inter": (c_int, [_P, _ip, c_int, c_int, _ip, _fp, _fp, _ip]),
})

MAX_GROUP, DETECT_GROUP = 16, 16      # SCL_IRIS_MAX_GROUP, SCL_IRIS_DETECT_GROUP
SEARCH_MAX = 32                       # SCL_IRIS_SEARCH_MAX


def _lib():
    return bind(load_library(), _SIG)


class IrisError(PluginError):
    pass


class IrisEngine(PluginEngine):
    """Mirror of lidar_iris_descriptor (descriptor.h:462-1302): same constructor arguments and defaults, the six plugin
    calls (make_and_save, save_from_wire, detect_intra, detect_inter, get_index, get_size) and the building blocks."""
    PREFIX, CONFIG, ERROR = "scl_iris", IrisConfig, IrisError

    def __init__(self, rows=80, cols=360, nscan=64, dist_thres=0.32, num_exclude_recent=30, match_num=2, num_candidates=10,
                 nscale=4, min_wavelength=18, mult=1.6, sigma_onf=0.75, robot_num=1, this_id=0, device=0,
                 knn_exclude_eps=None, wire_decode=0, shift_search=0):
        super().__init__(_lib(), rows=rows, cols=cols, nscan=nscan, nscale=nscale, min_wavelength=min_wavelength, mult=mult,
                         sigma_onf=sigma_onf, device=device, dist_thres=dist_thres, num_exclude_recent=num_exclude_recent,
                         match_num=match_num, num_candidates=num_candidates, robot_num=robot_num, this_id=this_id,
                         knn_exclude_eps=knn_exclude_eps, wire_decode=wire_decode, shift_search=shift_search)
        self.rows, self.cols, self.trows = rows, cols, 2 * nscale * rows

    @staticmethod
    def _cloud(points):
        a = np.ascontiguousarray(points, dtype=np.float32)
        return a, a.shape[0], a.shape[1] * 4

    def make_image(self, points):
        a, n, st = self._cloud(points)
        img = np.empty((self.rows, self.cols), np.uint8); key = np.empty(self.rows, np.float32)
        self._check(self.L.scl_iris_make_image(self.h, a.ctypes.data_as(c_void_p), n, st, img.ctypes.data_as(POINTER(c_uint8)),
                                               key.ctypes.data_as(POINTER(c_float))), "scl_iris_make_image")
        return img, key

    def make_and_save(self, points, robot=0, index=0):
        a, n, st = self._cloud(points)
        out = np.empty(self.rows * self.cols + self.rows, np.float32)
        self._check(self.L.scl_iris_make_and_save(self.h, a.ctypes.data_as(c_void_p), n, st, robot, index, out.ctypes.data_as(POINTER(c_float))),
                    "scl_iris_make_and_save")
        return out

    def save_image(self, image, rowkey, robot=0, index=0):
        img = np.ascontiguousarray(image, np.uint8); key = np.ascontiguousarray(rowkey, np.float32)
        self._check(self.L.scl_iris_save_image(self.h, img.ctypes.data_as(POINTER(c_uint8)), key.ctypes.data_as(POINTER(c_float)), robot, index),
                    "scl_iris_save_image")

    def save_from_wire(self, values, robot=0, index=0):
        v = np.ascontiguousarray(values, np.float32)
        assert v.size == self.rows * self.cols + self.rows
        self._check(self.L.scl_iris_save_from_wire(self.h, v.ctypes.data_as(POINTER(c_float)), robot, index), "scl_iris_save_from_wire")

    def _detect(self, fn, name, cur):
        loop, bias, dist = c_int(), c_float(), c_float()
        self._check(fn(self.h, cur, byref(loop), byref(bias), byref(dist)), name)
        return loop.value, bias.value, dist.value

    def detect_intra(self, cur):
        """(loop local index or -1, column shift, smallest distance seen) -- detectIntraLoopClosureID, D.h:1085-1151"""
        return self._detect(self.L.scl_iris_detect_intra, "scl_iris_detect_intra", cur)

    def detect_inter(self, cur):
        """(loop global key or -1, column shift, smallest distance seen) -- detectInterLoopClosureID, D.h:1153-1253"""
        return self._detect(self.L.scl_iris_detect_inter, "scl_iris_detect_inter", cur)

    # ---- the batch forms (scl_iris.h "THE BATCH FORMS"): the argument conventions of _plugin.VectorPluginEngine
    def _clouds(self, clouds, robots, indexs, where):
        """the arguments of a batched build: (arrays kept alive, pointers, counts, stride, robots, indexs, count)"""
        arrs = [self._cloud(c) for c in clouds]
        count = len(arrs)
        if count and len({st for _, _, st in arrs}) != 1:
            raise ValueError(f"{where}: one stride for all clouds")
        st = arrs[0][2] if count else 12
        ptrs = (c_void_p * max(count, 1))(*[a.ctypes.data for a, _, _ in arrs])
        ns = np.ascontiguousarray([n for _, n, _ in arrs], np.int32)
        rb = np.ascontiguousarray(robots if robots is not None else np.zeros(count), np.int8)
        ix = np.ascontiguousarray(indexs if indexs is not None else np.arange(count), np.int32)
        if rb.size != count or ix.size != count:
            raise ValueError(f"{where}: one robot id and one index per cloud")
        return arrs, ptrs, ns, st, rb, ix, count

    @staticmethod
    def _batch_out(count, **arrays):
        for name, (a, t) in arrays.items():
            if a is not None and (a.dtype != t or a.size != count or not a.flags.c_contiguous):
                raise ValueError(f"{name}: a contiguous {np.dtype(t).name} array of {count} elements")

    def make_and_save_many(self, clouds, robots=None, indexs=None, want_values=True):
        """clouds: list of (n_i, k) float32 arrays with one record width k; returns (count, rows * cols + rows) float32, the
        vectors make_and_save returns (None if not wanted)"""
        _keep, ptrs, ns, st, rb, ix, count = self._clouds(clouds, robots, indexs, "make_and_save_many")
        out = np.empty((count, self.rows * self.cols + self.rows), np.float32) if want_values else None
        self._call("make_and_save_many", ptrs, ns.ctypes.data_as(_ip), st, rb.ctypes.data_as(POINTER(c_int8)), ix.ctypes.data_as(_ip), count,
                   out.ctypes.data_as(_fp) if out is not None else None)
        return out

    def save_from_wire_many(self, values, robots=None, indexs=None):
        """values: (count, rows * cols + rows) float32 vectors appended in order as robots[i] / indexs[i]"""
        v = np.ascontiguousarray(values, np.float32).reshape(-1, self.rows * self.cols + self.rows)
        count = v.shape[0]
        rb = np.ascontiguousarray(robots if robots is not None else np.zeros(count), np.int8)
        ix = np.ascontiguousarray(indexs if indexs is not None else np.arange(count), np.int32)
        if rb.size != count or ix.size != count:
            raise ValueError("save_from_wire_many: one robot id and one index per vector")
        self._call("save_from_wire_many", v.ctypes.data_as(_fp), rb.ctypes.data_as(POINTER(c_int8)), ix.ctypes.data_as(_ip), count)

    def _detect_many(self, name, curs, loops, biases, dists, want_dists):
        c = np.ascontiguousarray(curs, np.int32).ravel()
        loops = np.empty(c.size, np.int32) if loops is None else loops
        biases = np.empty(c.size, np.float32) if biases is None else biases
        if dists is None and want_dists:
            dists = np.empty(c.size, np.float32)
        self._batch_out(c.size, loops=(loops, np.int32), biases=(biases, np.float32), dists=(dists, np.float32))
        self._call(name, c.ctypes.data_as(_ip), c.size, loops.ctypes.data_as(_ip), biases.ctypes.data_as(_fp),
                   dists.ctypes.data_as(_fp) if dists is not None else None)
        return loops, biases, dists

    def detect_intra_many(self, curs, loops=None, biases=None, dists=None, want_dists=True):
        """detect_intra for every local index of curs, as the single calls in that order answer: (loops int32, biases float32,
        dists float32; dists None with want_dists=False).  loops / biases / dists: arrays to fill (untouched when the call fails)"""
        return self._detect_many("detect_intra_many", curs, loops, biases, dists, want_dists)

    def detect_inter_many(self, curs, loops=None, biases=None, dists=None, want_dists=True):
        """detect_inter for every global key of curs, as the single calls in that order answer: (loops, biases, dists)"""
        return self._detect_many("detect_inter_many", curs, loops, biases, dists, want_dists)

    def make_save_and_detect(self, clouds, robots=None, indexs=None, want_values=True, loops=None, biases=None, dists=None):
        """make_and_save_many, then detect_intra of every new keyframe of this robot in the same call: (loops int32, biases float32,
        dists float32, values (count, rows * cols + rows) float32 or None); entries of other robots answer (-1, 0, 10000000)"""
        _keep, ptrs, ns, st, rb, ix, count = self._clouds(clouds, robots, indexs, "make_save_and_detect")
        loops = np.empty(count, np.int32) if loops is None else loops
        biases = np.empty(count, np.float32) if biases is None else biases
        dists = np.empty(count, np.float32) if dists is None else dists
        self._batch_out(count, loops=(loops, np.int32), biases=(biases, np.float32), dists=(dists, np.float32))
        out = np.empty((count, self.rows * self.cols + self.rows), np.float32) if want_values else None
        self._call("make_save_and_detect", ptrs, ns.ctypes.data_as(_ip), st, rb.ctypes.data_as(POINTER(c_int8)), ix.ctypes.data_as(_ip), count,
                   loops.ctypes.data_as(_ip), biases.ctypes.data_as(_fp), dists.ctypes.data_as(_fp), out.ctypes.data_as(_fp) if out is not None else None)
        return loops, biases, dists, out

    # ---- the exhaustive ranked search (scl_iris.h "THE EXHAUSTIVE SEARCH")
    def _search(self, name, curs, k, ids, biases, dists, n_found):
        c = np.ascontiguousarray(curs, np.int32).ravel()
        k = int(k)
        rows = max(k, 0)
        ids = np.empty((c.size, rows), np.int32) if ids is None else ids
        biases = np.empty((c.size, rows), np.float32) if biases is None else biases
        dists = np.empty((c.size, rows), np.float32) if dists is None else dists
        n_found = np.empty(c.size, np.int32) if n_found is None else n_found
        for a, t, size in ((ids, np.int32, c.size * rows), (biases, np.float32, c.size * rows), (dists, np.float32, c.size * rows),
                           (n_found, np.int32, c.size)):
            if a.dtype != t or a.size != size or not a.flags.c_contiguous:
                raise ValueError(f"a contiguous {np.dtype(t).name} array of {size} elements")
        self._call(name, c.ctypes.data_as(_ip), c.size, k, ids.ctypes.data_as(_ip), biases.ctypes.data_as(_fp), dists.ctypes.data_as(_fp),
                   n_found.ctypes.data_as(_ip))
        return ids, biases, dists, n_found

    def search_intra(self, curs, k, ids=None, biases=None, dists=None, n_found=None):
        """the k best of this robot's keyframes [0, cur - num_exclude_recent) for every local index of curs, every column shift scored
        against the whole set, without dist_thres: (ids (count, k) int32 LOCAL, biases (count, k) float32, dists (count, k) float32,
        n_found int32); entries past n_found[i] are (-1, 0, +inf).  ids / biases / dists / n_found: arrays to fill (left untouched
        when the call fails)"""
        return self._search("search_intra", curs, k, ids, biases, dists, n_found)

    def search_inter(self, curs, k, ids=None, biases=None, dists=None, n_found=None):
        """the k best of the set detect_inter searches, for every global key of curs: (ids (count, k) int32 GLOBAL, biases, dists, n_found)"""
        return self._search("search_inter", curs, k, ids, biases, dists, n_found)

    def get_image(self, key):
        img = np.empty((self.rows, self.cols), np.uint8); k = np.empty(self.rows, np.float32)
        self._check(self.L.scl_iris_get_image(self.h, key, img.ctypes.data_as(POINTER(c_uint8)), k.ctypes.data_as(POINTER(c_float))), "scl_iris_get_image")
        return img, k

    def get_feature(self, key):
        T = np.empty((self.trows, self.cols), np.uint8); M = np.empty((self.trows, self.cols), np.uint8)
        self._check(self.L.scl_iris_get_feature(self.h, key, T.ctypes.data_as(POINTER(c_uint8)), M.ctypes.data_as(POINTER(c_uint8))), "scl_iris_get_feature")
        return T, M

    def hamming(self, key1, key2, scale):
        d, b = c_float(), c_int()
        self._check(self.L.scl_iris_hamming(self.h, key1, key2, scale, byref(d), byref(b)), "scl_iris_hamming")
        return d.value, b.value

    def hamming_batch(self, key1, cand, scales):
        c = np.ascontiguousarray(cand, np.int32); s = np.ascontiguousarray(scales, np.int32)
        d = np.empty(c.size, np.float32); b = np.empty(c.size, np.int32)
        self._check(self.L.scl_iris_hamming_batch(self.h, key1, c.ctypes.data_as(POINTER(c_int)), s.ctypes.data_as(POINTER(c_int)), c.size,
                                                  d.ctypes.data_as(POINTER(c_float)), b.ctypes.data_as(POINTER(c_int))), "scl_iris_hamming_batch")
        return d, b

    def hamming_all_shifts(self, key1, cand):
        c = np.ascontiguousarray(cand, np.int32)
        d = np.empty(c.size, np.float32); b = np.empty(c.size, np.int32)
        self._check(self.L.scl_iris_hamming_all_shifts(self.h, key1, c.ctypes.data_as(POINTER(c_int)), c.size,
                                                       d.ctypes.data_as(POINTER(c_float)), b.ctypes.data_as(POINTER(c_int))), "scl_iris_hamming_all_shifts")
        return d, b

    def fft_match(self, key0, roll0, key1):
        """fftMatch(image of key0 turned by roll0 columns, image of key1), descriptor.h:793-932: (centre x as float32, compatible)"""
        cx, ok = c_float(), c_int()
        self._check(self.L.scl_iris_fft_match(self.h, key0, roll0, key1, byref(cx), byref(ok)), "scl_iris_fft_match")
        return np.float32(cx.value), bool(ok.value)

    def compare(self, key1, cand):
        """compare(key1, cand[i]) of descriptor.h:964-1024 (match_num as configured): distances and shifts"""
        c = np.ascontiguousarray(cand, np.int32)
        d = np.empty(c.size, np.float32); b = np.empty(c.size, np.int32)
        self._check(self.L.scl_iris_compare(self.h, key1, c.ctypes.data_as(POINTER(c_int)), c.size,
                                            d.ctypes.data_as(POINTER(c_float)), b.ctypes.data_as(POINTER(c_int))), "scl_iris_compare")
        return d, b

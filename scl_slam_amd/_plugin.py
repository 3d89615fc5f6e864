"""The ctypes layer the descriptor plugin mirrors share (iris.py, m2dp.py, fpfh.py, grsd.py): signature binding, the error class, the
handle life-cycle and the keyframe-registry calls; for the vector plugins (M2DP, FPFH, GRSD) also the database, build and 1-NN calls."""
from ctypes import POINTER, byref, c_char_p, c_float, c_int, c_int8, c_void_p

import numpy as np

_bound = set()


def bind(lib, table):
    """Set restype / argtypes of every function of `table` ({name: (restype, argtypes)}) on `lib`, once per table; returns lib."""
    if id(table) not in _bound:
        for name, (res, args) in table.items():
            fn = getattr(lib, name); fn.restype = res; fn.argtypes = args
        _bound.add(id(table))
    return lib


def plugin_signatures(prefix, config):
    """The calls every plugin header declares: life-cycle, save_from_wire and the keyframe registry."""
    P, ip = c_void_p, POINTER(c_int)
    return {
        f"{prefix}_default_config": (c_int, [POINTER(config)]),
        f"{prefix}_create": (c_int, [POINTER(config), POINTER(P)]),
        f"{prefix}_destroy": (c_int, [P]),
        f"{prefix}_last_error": (c_char_p, [P]),
        f"{prefix}_save_from_wire": (c_int, [P, POINTER(c_float), c_int8, c_int]),
        f"{prefix}_get_size": (c_int, [P]),
        f"{prefix}_get_size_of": (c_int, [P, c_int]),
        f"{prefix}_get_index": (c_int, [P, c_int, POINTER(c_int8), ip]),
        f"{prefix}_local_to_global": (c_int, [P, c_int, c_int, ip]),
    }


def vector_signatures(prefix, config):
    """plugin_signatures plus the float-descriptor calls of M2DP, FPFH and GRSD."""
    P, fp, ip = c_void_p, POINTER(c_float), POINTER(c_int)
    sig = plugin_signatures(prefix, config)
    sig.update({
        f"{prefix}_make": (c_int, [P, P, c_int, c_int, fp]),
        f"{prefix}_make_and_save": (c_int, [P, P, c_int, c_int, c_int8, c_int, fp]),
        f"{prefix}_make_and_save_many": (c_int, [P, POINTER(c_void_p), ip, c_int, POINTER(c_int8), ip, c_int, fp]),
        f"{prefix}_get_signature": (c_int, [P, c_int, fp]),
        f"{prefix}_detect_intra": (c_int, [P, c_int, ip, fp]),
        f"{prefix}_detect_inter": (c_int, [P, c_int, ip, fp]),
        f"{prefix}_detect_intra_many": (c_int, [P, ip, c_int, ip, fp]),
        f"{prefix}_detect_inter_many": (c_int, [P, ip, c_int, ip, fp]),
        f"{prefix}_save_from_wire_many": (c_int, [P, fp, POINTER(c_int8), ip, c_int]),
        f"{prefix}_make_save_and_detect": (c_int, [P, POINTER(c_void_p), ip, c_int, POINTER(c_int8), ip, c_int, ip, fp, fp]),
        f"{prefix}_detect_intra_topk": (c_int, [P, ip, c_int, c_int, ip, fp, ip]),
        f"{prefix}_detect_inter_topk": (c_int, [P, ip, c_int, c_int, ip, fp, ip]),
    })
    return sig


class PluginError(RuntimeError):
    def __init__(self, where, status, message=""):
        super().__init__(f"{where}: status {status} ({message})")
        self.status = status


class PluginEngine:
    """One plugin handle.  Subclasses set PREFIX (the C prefix, e.g. "scl_m2dp"), CONFIG (the ctypes config struct) and ERROR
    (their PluginError subclass), and pass the bound library and the config fields to __init__ (None keeps the default)."""
    PREFIX = None
    CONFIG = None
    ERROR = PluginError

    def __init__(self, lib, **fields):
        self.L = lib
        cfg = self.CONFIG()
        getattr(lib, f"{self.PREFIX}_default_config")(byref(cfg))
        for name, value in fields.items():
            if value is not None:
                setattr(cfg, name, value)
        self.cfg = cfg
        self.h = c_void_p()
        rc = getattr(lib, f"{self.PREFIX}_create")(byref(cfg), byref(self.h))
        if rc != 0:
            self.h = c_void_p()
            raise self.ERROR(f"{self.PREFIX}_create", rc)

    def _check(self, rc, where):
        if rc != 0:
            raise self.ERROR(where, rc, getattr(self.L, f"{self.PREFIX}_last_error")(self.h).decode())

    def _call(self, name, *args):
        """PREFIX_name(handle, *args), status checked"""
        fn = f"{self.PREFIX}_{name}"
        self._check(getattr(self.L, fn)(self.h, *args), fn)

    def close(self):
        if self.h and self.h.value:
            getattr(self.L, f"{self.PREFIX}_destroy")(self.h); self.h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_size(self, robot=-1):
        n = getattr(self.L, f"{self.PREFIX}_get_size_of")(self.h, robot)
        if n < 0:
            self._check(n, f"{self.PREFIX}_get_size_of")
        return n

    def get_index(self, key):
        r, i = c_int8(), c_int()
        self._call("get_index", key, byref(r), byref(i))
        return r.value, i.value

    def local_to_global(self, robot, local):
        k = c_int()
        self._call("local_to_global", robot, local, byref(k))
        return k.value


class VectorPluginEngine(PluginEngine):
    """A plugin whose descriptor is DIM floats (M2DP, FPFH, GRSD): make, make_and_save(_many), save_from_wire, get_signature and the
    1-NN detections, each with its batch form (numpy arrays in and out), and the candidate lists (detect_*_topk)."""
    DIM = None

    @staticmethod
    def _cloud(points):
        a = np.ascontiguousarray(points, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError("points: (n, >= 3) float32 records")
        return a, a.shape[0], a.shape[1] * 4

    def make(self, points):
        a, n, st = self._cloud(points)
        out = np.empty(self.DIM, np.float32)
        self._call("make", a.ctypes.data_as(c_void_p), n, st, out.ctypes.data_as(POINTER(c_float)))
        return out

    def make_and_save(self, points, robot=0, index=0):
        a, n, st = self._cloud(points)
        out = np.empty(self.DIM, np.float32)
        self._call("make_and_save", a.ctypes.data_as(c_void_p), n, st, robot, index, out.ctypes.data_as(POINTER(c_float)))
        return out

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

    def make_and_save_many(self, clouds, robots=None, indexs=None, want_values=True):
        """clouds: list of (n_i, k) float32 arrays with one record width k; returns (count, DIM) float32 (None if not wanted)"""
        _keep, ptrs, ns, st, rb, ix, count = self._clouds(clouds, robots, indexs, "make_and_save_many")
        out = np.empty((count, self.DIM), np.float32) if want_values else None
        self._call("make_and_save_many", ptrs, ns.ctypes.data_as(POINTER(c_int)), st, rb.ctypes.data_as(POINTER(c_int8)),
                   ix.ctypes.data_as(POINTER(c_int)), count, out.ctypes.data_as(POINTER(c_float)) if out is not None else None)
        return out

    def make_save_and_detect(self, clouds, robots=None, indexs=None, want_values=True, loops=None, dists=None):
        """make_and_save_many, then detect_intra of every new keyframe of this robot in the same call: (loops int32, dists float32,
        values (count, DIM) float32 or None).  loops / dists: arrays to fill (left untouched when the call fails)"""
        _keep, ptrs, ns, st, rb, ix, count = self._clouds(clouds, robots, indexs, "make_save_and_detect")
        loops = np.empty(count, np.int32) if loops is None else loops
        dists = np.empty(count, np.float32) if dists is None else dists
        self._batch_out(loops, dists, count)
        out = np.empty((count, self.DIM), np.float32) if want_values else None
        self._call("make_save_and_detect", ptrs, ns.ctypes.data_as(POINTER(c_int)), st, rb.ctypes.data_as(POINTER(c_int8)),
                   ix.ctypes.data_as(POINTER(c_int)), count, loops.ctypes.data_as(POINTER(c_int)), dists.ctypes.data_as(POINTER(c_float)),
                   out.ctypes.data_as(POINTER(c_float)) if out is not None else None)
        return loops, dists, out

    def save_from_wire_many(self, values, robots=None, indexs=None):
        """values: (count, DIM) float32 rows appended in order as robots[i] / indexs[i]"""
        v = np.ascontiguousarray(values, np.float32).reshape(-1, self.DIM)
        count = v.shape[0]
        rb = np.ascontiguousarray(robots if robots is not None else np.zeros(count), np.int8)
        ix = np.ascontiguousarray(indexs if indexs is not None else np.arange(count), np.int32)
        if rb.size != count or ix.size != count:
            raise ValueError("save_from_wire_many: one robot id and one index per row")
        self._call("save_from_wire_many", v.ctypes.data_as(POINTER(c_float)), rb.ctypes.data_as(POINTER(c_int8)),
                   ix.ctypes.data_as(POINTER(c_int)), count)

    def save_from_wire(self, values, robot=0, index=0):
        v = np.ascontiguousarray(values, np.float32)
        assert v.size == self.DIM
        self._call("save_from_wire", v.ctypes.data_as(POINTER(c_float)), robot, index)

    def get_signature(self, key):
        out = np.empty(self.DIM, np.float32)
        self._call("get_signature", key, out.ctypes.data_as(POINTER(c_float)))
        return out

    def detect_intra(self, cur):
        """(loop local index or -1, float32 distance to the nearest)"""
        loop, d = c_int(), c_float()
        self._call("detect_intra", cur, byref(loop), byref(d))
        return loop.value, np.float32(d.value)

    def detect_inter(self, cur):
        """(loop global key or -1, float32 distance to the nearest)"""
        loop, d = c_int(), c_float()
        self._call("detect_inter", cur, byref(loop), byref(d))
        return loop.value, np.float32(d.value)

    @staticmethod
    def _batch_out(loops, dists, count):
        for a, t in ((loops, np.int32), (dists, np.float32)):
            if a is not None and (a.dtype != t or a.size != count or not a.flags.c_contiguous):
                raise ValueError(f"a contiguous {np.dtype(t).name} array of {count} elements")

    def _detect_many(self, name, curs, loops, dists, want_dists):
        c = np.ascontiguousarray(curs, np.int32).ravel()
        loops = np.empty(c.size, np.int32) if loops is None else loops
        if dists is None and want_dists:
            dists = np.empty(c.size, np.float32)
        self._batch_out(loops, dists, c.size)
        self._call(name, c.ctypes.data_as(POINTER(c_int)), c.size, loops.ctypes.data_as(POINTER(c_int)),
                   dists.ctypes.data_as(POINTER(c_float)) if dists is not None else None)
        return loops, dists

    def detect_intra_many(self, curs, loops=None, dists=None, want_dists=True):
        """detect_intra for every local index of curs, as the single calls in that order answer: (loops int32, dists float32; dists
        None with want_dists=False).  loops / dists: arrays to fill (left untouched when the call fails)"""
        return self._detect_many("detect_intra_many", curs, loops, dists, want_dists)

    def detect_inter_many(self, curs, loops=None, dists=None, want_dists=True):
        """detect_inter for every global key of curs, as the single calls in that order answer: (loops int32, dists float32)"""
        return self._detect_many("detect_inter_many", curs, loops, dists, want_dists)

    def _detect_topk(self, name, curs, k, ids, dists, n_found):
        c = np.ascontiguousarray(curs, np.int32).ravel()
        k = int(k)
        rows = max(k, 0)
        ids = np.empty((c.size, rows), np.int32) if ids is None else ids
        dists = np.empty((c.size, rows), np.float32) if dists is None else dists
        n_found = np.empty(c.size, np.int32) if n_found is None else n_found
        for a, t, size in ((ids, np.int32, c.size * rows), (dists, np.float32, c.size * rows), (n_found, np.int32, c.size)):
            if a.dtype != t or a.size != size or not a.flags.c_contiguous:
                raise ValueError(f"a contiguous {np.dtype(t).name} array of {size} elements")
        self._call(name, c.ctypes.data_as(POINTER(c_int)), c.size, k, ids.ctypes.data_as(POINTER(c_int)),
                   dists.ctypes.data_as(POINTER(c_float)), n_found.ctypes.data_as(POINTER(c_int)))
        return ids, dists, n_found

    def detect_intra_topk(self, curs, k, ids=None, dists=None, n_found=None):
        """the k nearest of the set detect_intra searches, for every local index of curs, without dist_thres: (ids (count, k) int32
        LOCAL, dists (count, k) float32, n_found int32); entries past n_found[i] are (-1, +inf).  ids / dists / n_found: arrays to
        fill (left untouched when the call fails)"""
        return self._detect_topk("detect_intra_topk", curs, k, ids, dists, n_found)

    def detect_inter_topk(self, curs, k, ids=None, dists=None, n_found=None):
        """the k nearest of the set detect_inter searches, for every global key of curs: (ids (count, k) int32 GLOBAL, dists, n_found)"""
        return self._detect_topk("detect_inter_topk", curs, k, ids, dists, n_found)

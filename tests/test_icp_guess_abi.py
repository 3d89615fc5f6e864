"""The C ABI of the batched ICP with initial guesses (include/scl_engine.h "THE BATCHED ICP WITH INITIAL GUESSES") without a GPU:
the three calls declared and exported, the binding's argument types those of the declarations, the ABI version moved to 9, a NULL
engine refused with nothing written, the Python methods the unguessed ones with `guesses` behind the candidates.  (The technique
of tests/test_verification_guess_abi.py.)"""
import ctypes
import inspect
from ctypes import POINTER, c_float, c_int

from scl_slam_amd import load_library
from scl_slam_amd.engine import IcpParams, ScanContextEngine, _bind
from test_verification_guess_abi import C_TYPES, INVALID_ARG, _declaration

NAMES = ("scl_icp_align_batch_guess", "scl_loop_icp_batch_from_store_guess", "scl_icp_align_batch_from_store_guess")
TYPES = dict(C_TYPES, **{"const scl_icp_params *": POINTER(IcpParams)})


def test_declared_exported_and_typed():
    lib = load_library(); _bind(lib)
    assert lib.scl_abi_version() >= 9
    for name in NAMES:
        fn = getattr(lib, name)
        want = [TYPES[t] for t in _declaration(name)]
        assert fn.restype is c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert [len(_declaration(n)) for n in NAMES] == [14, 20, 22]
    # the unguessed declarations with `guesses` in front of the parameters and T_icp behind T
    for guessed, plain in ((NAMES[0], "scl_icp_align_batch"), (NAMES[1], "scl_loop_icp_batch_from_store")):
        g, p = _declaration(guessed), _declaration(plain)
        at = p.index("const scl_icp_params *")
        rest = p[at:]
        t = rest.index("float *")
        assert g == p[:at] + ["const float *"] + rest[:t + 1] + ["float *"] + rest[t + 1:], (guessed, g, p)


def test_a_null_engine_is_refused_and_nothing_is_written():
    lib = load_library(); _bind(lib)
    T = (c_float * 16)(*([7.0] * 16)); Ti = (c_float * 16)(*([7.0] * 16))
    fit = c_float(7.0); cv = c_int(7); it = c_int(7); ns = c_int(7); nt = c_int(7)
    cloud = (c_float * 8)(); ptrs = (ctypes.c_void_p * 1)(ctypes.addressof(cloud)); counts = (c_int * 1)(1); keys = (c_int * 1)(0)
    poses = (c_float * 16)(); G = (c_float * 16)(*[1.0 if k % 5 == 0 else 0.0 for k in range(16)])
    p = IcpParams(); lib.scl_icp_default_params(ctypes.byref(p))
    out = (T, Ti, ctypes.byref(fit), ctypes.byref(cv), ctypes.byref(it))
    assert lib.scl_icp_align_batch_guess(None, ctypes.addressof(cloud), 1, ptrs, counts, 1, 32, G, ctypes.byref(p), *out) == INVALID_ARG
    assert lib.scl_loop_icp_batch_from_store_guess(None, 0, 0, poses, 1, keys, 0, poses, 0.3, G, ctypes.byref(p), 300, 1000, *out,
                                                   ctypes.byref(ns), ctypes.byref(nt)) == INVALID_ARG
    assert lib.scl_icp_align_batch_from_store_guess(None, ctypes.addressof(cloud), 1, 32, 0.2, 0, 1, keys, 0, poses, 0.3, G, ctypes.byref(p),
                                                    300, 1000, *out, ctypes.byref(ns), ctypes.byref(nt)) == INVALID_ARG
    assert list(T) == [7.0] * 16 and list(Ti) == [7.0] * 16
    assert (fit.value, cv.value, it.value, ns.value, nt.value) == (7.0, 7, 7, 7, 7)


def test_the_binding_follows_the_unguessed_forms():
    """the Python methods: the unguessed methods' parameters and defaults with `guesses` behind the candidates"""
    def spec(f):
        p = inspect.signature(f).parameters
        return [(n, v.default) for n, v in p.items() if n != "self"]
    E = ScanContextEngine
    plain, guessed = spec(E.icp_align_batch), spec(E.icp_align_batch_guess)
    assert guessed == plain[:2] + [("guesses", inspect.Parameter.empty)] + plain[2:]
    plain, guessed = spec(E.loop_icp_batch_from_store), spec(E.loop_icp_batch_from_store_guess)
    assert guessed == plain[:7] + [("guesses", inspect.Parameter.empty)] + plain[7:]
    # the received form: the guessed verification's cloud arguments, then the ICP's parameters and gates
    verify, guessed = spec(E.geometric_verification_batch_from_store_guess), spec(E.icp_align_batch_from_store_guess)
    assert guessed[:8] == verify[:8] and guessed[8:] == spec(E.loop_icp_batch_from_store)[7:]

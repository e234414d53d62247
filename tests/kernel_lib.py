"""TEST INFRASTRUCTURE: ctypes binding of tests/kernels/libwn_kernel_harness.so (tests/kernels/build_harness.py), the product's training-time
and inference kernels launched one at a time through their own launchers.  The argument structs are filled in C (wn_kernel_harness.hip): this side
passes scalars, device pointers and row maps as (pointer, batch_stride, row_stride, t0).  The product package never loads it."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
_P, _I, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_MAP = [_P, _LL, _LL, _LL]
NOMAP = (None, 0, 0, 0)

_SIGS = {
    "kh_nn": [_P, _I] + _MAP + _MAP + [_I, _I, _P, _P, _I, _P] + _MAP + _MAP + [_LL, _I, _I, _I, _P, _P, _P] + _MAP +
             [_I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I],
    "kh_layer": [_P] + _MAP + _MAP + [_I, _I, _P, _P] + _MAP + [_LL, _I, _P] + _MAP + [_I, _I, _I, _P, _P] + _MAP + _MAP + [_P],
    "kh_bwd_layer": [_P] + _MAP + _MAP + [_I, _I, _P, _P, _I] + _MAP + _MAP + [_LL, _I, _I, _I, _I, _I, _I, _P, _P] + _MAP + [_I] + _MAP,
    "kh_tn": [_P, _I, _I] + _MAP + [_P] + _MAP + [_I, _I, _P, _I, _LL, _I, _I] + _MAP + [_I, _I, _I, _I, _I],
    "kh_colsum": [_P, _I] + _MAP + [_LL, _I, _I, _P, _I],
    "kh_tn_reduce": [_P, _P, _I, _I, _I, _P, _I, _I],
    "kh_gate_bwd": [_P, _I, _P, _P, _P, _P, _LL, _I, _P, _I, _I, _I],
    "kh_xent": [_P, _P, _P, _LL, _P, _P, _P],
    "kh_taps": [_P, _I] + _MAP + [_LL, _LL, _I, _P, _I, _P] + _MAP + [_LL, _I] + _MAP + [_I, _P, _P, _I],
    "kh_score_head": [_P, _I, _P, _LL, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "kh_score_rows": [_P, _P, _I, _P, _LL, _P, _P, _P],
    "kh_score_reduce": [_P, _P, _LL, _P],
    "kh_fill_ring": [_P, _P, _LL, _P, _I, _I, _I, _I, _LL, _I],
    "kh_fwd_start": [_P, _P, _P, _P, _P, _LL, _I, _P],
    "kh_cvt_bf16": [_P, _P, _P, _LL],
    "kh_cvt_bf16_transposed": [_P, _P, _LL, _P, _I, _I, _I],
    "kh_transpose_batched": [_P, _P, _LL, _P, _I, _I, _I],
    "kh_tn_grid": [_LL, _I, _I, _I, _I, ctypes.POINTER(_LL)],
}


class Harness:
    def __init__(self, path):
        self.dll = ctypes.CDLL(path)
        for name, args in _SIGS.items():
            fn = getattr(self.dll, name)
            fn.argtypes = args
            fn.restype = None if name == "kh_tn_grid" else _I
        self.dll.kh_release.restype = None
        assert self.dll.kh_version() == 2, "stale kernel harness (tests/kernels/build_harness.py --force)"

    def call(self, name, *args):
        rc = getattr(self.dll, name)(*args)
        if rc:
            raise RuntimeError("%s: HIP error %d" % (name, rc))
        return rc

    def tn_grid(self, M, Ka, Nb, tile_nb, want):
        out = (_LL * 2)()
        self.dll.kh_tn_grid(M, Ka, Nb, tile_nb, want, out)
        return int(out[0]), int(out[1])

    def close(self):
        self.dll.kh_release()


def build_and_load(force=False):
    """WN_KERNEL_HARNESS=<path>: load a harness built elsewhere (a mutated copy of the kernels, for a mutation check) instead of building this one"""
    other = os.environ.get("WN_KERNEL_HARNESS")
    if other:
        return Harness(other)
    sys.path.insert(0, os.path.join(HERE, "kernels"))
    import build_harness
    return Harness(build_harness.build_harness(force=force))

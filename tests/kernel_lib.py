"""TEST INFRASTRUCTURE: what the kernel-level GPU tests (tests/test_gpu_*kernels.py) share.

  * the ctypes binding of tests/kernels/libwn_kernel_harness.so (tests/kernels/build_harness.py), the product's kernels launched one at a time through
    their own launchers.  The argument structs are filled in C (wn_kernel_harness.hip): this side passes scalars, device pointers and row maps as
    (pointer, batch_stride, row_stride, t0).  Built at most once and loaded once per process (build_and_load); the session fixture `kh` hands it out
    and releases it at the end of the session.  A test module imports `kh` into its own namespace, where pytest finds it.
  * the helpers of the tests' method: sentinels, guarded row matrices, bf16 rounding on the host, bit comparison, the bounded families' record
  * the launch of one sampler on one part of a case family (tests/test_gpu_sampler_kernels.py, tests/test_gpu_sampler_filter_kernels.py), and of its
    log-probability / forced form on a list of parts (tests/test_gpu_logp_kernels.py)
The product package never loads any of it."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_P, _I, _LL, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
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
    "kf_sample_1w": [_P, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P],
    "kf_sample_generic": [_P, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P],
    "kf_logp_1w": [_P, _I, _I, _F, _I, _P, _P, _P, _P, _P, _P, _P, _P],
    "kf_logp_generic": [_P, _I, _I, _I, _F, _I, _P, _LL, _P, _P, _P, _P, _P, _P, _P, _P],
    "kf_smp_floats": [_I],
    "kf_run_bytes": [],
    "kst_gather": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _LL, _P, _LL, _I, _P],
    "kst_scatter": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _LL, _P, _LL, _I, _I, _P],
    "kst_vec": [_I, _I, _P],
    "kt_bwd_taps": [_P, _I] + _MAP + [_LL, _LL, _LL, _I, _P, _LL, _I] + _MAP + [_I] + _MAP + [_LL, _I],
    "kt_layer_dx": [_P, _I, _I, _I, _P, _LL, _LL, _LL, _P, _LL, _P, _P, _LL, _LL],
    "kb_taps_bf16": [_P, _I] + _MAP + [_LL, _LL, _I, _P, _I, _P] + _MAP + [_LL, _I] + _MAP + [_I],
    "kp_nn_ragged": [_P, _I] + _MAP + _MAP + [_I, _I, _P, _I, _P] + _MAP + _MAP + [_LL, _P, _I, _I],
    "kp_taps_ragged": [_P, _I] + _MAP + [_LL, _LL, _I, _P, _I, _P] + _MAP + [_LL, _P, _I, _I],
    "kp_fwd_start_ragged": [_P, _P, _LL, _P, _P, _P, _LL, _P, _I, _I, _LL, _I],
    "kp_fill_ring_at": [_P, _P, _LL, _P, _I, _I, _I, _I, _LL, _I, _LL],
    "kp_gather_history": [_P, _P, _I, _I, _I, _P, _LL, _LL, _LL, _LL, _P],
}


class Harness:
    def __init__(self, path):
        self.dll = ctypes.CDLL(path)
        for name, args in _SIGS.items():
            fn = getattr(self.dll, name)
            fn.argtypes = args
            fn.restype = None if name == "kh_tn_grid" else _I
        self.dll.kh_release.restype = None
        # the product's own exports (the harness includes the runtime unit whole): the fused Adam step, called with a wn_adam_args the test fills
        self.dll.wn_adam_step.argtypes = [_P]
        self.dll.wn_adam_step.restype = _I
        self.dll.wn_last_error.argtypes = []
        self.dll.wn_last_error.restype = ctypes.c_char_p
        assert self.dll.kh_version() == 5, "stale kernel harness (tests/kernels/build_harness.py --force)"

    def call(self, name, *args):
        rc = self.rc(name, *args)
        if rc:
            raise RuntimeError("%s: HIP error %d" % (name, rc))
        return rc

    def rc(self, name, *args):
        """the call's return code, whatever it is (the tests of the argument checks inspect it)"""
        return getattr(self.dll, name)(*args)

    def last_error(self):
        return (self.dll.wn_last_error() or b"").decode("utf-8", "replace")

    def tn_grid(self, M, Ka, Nb, tile_nb, want):
        out = (_LL * 2)()
        self.dll.kh_tn_grid(M, Ka, Nb, tile_nb, want, out)
        return int(out[0]), int(out[1])

    def close(self):
        self.dll.kh_release()


_LOADED = []


def build_and_load(force=False):
    """The one harness of the process: built if stale and loaded by the first call, handed out by every later one.
    WN_KERNEL_HARNESS=<path>: load a harness built elsewhere (a mutated copy of the kernels, for a mutation check) instead of building this one"""
    if not _LOADED:
        other = os.environ.get("WN_KERNEL_HARNESS")
        if not other:
            sys.path.insert(0, os.path.join(HERE, "kernels"))
            import build_harness
            other = build_harness.build_harness(force=force)
        _LOADED.append(Harness(other))
    return _LOADED[0]


# ---------------------------------------------------------------- the session's harness and the record of the bounded families
SENT32 = np.uint32(0x7FC0DEAD)    # sentinel of fp32 outputs (a NaN no kernel produces)
SENT16 = np.uint16(0x7FDE)        # ... of bf16 outputs
WORST = {}
WALL = {}    # module -> its own wall time in seconds (modules that share the harness and its closing line)
_T0 = time.time()


def _worst(family, err):
    WORST[family] = max(WORST.get(family, 0.0), float(err))


_KH = []   # the loaded harness: every kernel test module imports this fixture, and all share one harness and one closing line


@pytest.fixture(scope="session")
def kh(request):
    if _KH:
        return _KH[0]
    t0 = time.time()
    h = build_and_load()
    build_s = time.time() - t0

    def report():
        capman = request.config.pluginmanager.getplugin("capturemanager")
        with capman.global_and_fixture_disabled():
            print("\ntest_gpu_kernels%s: %.1f s wall (harness build / load %.1f s); worst errors of the bounded families: %s"
                  % ("".join(" (+ %s: %.1f s wall of its own)" % kv for kv in sorted(WALL.items())), time.time() - _T0, build_s, ", ".join("%s %.3g" % kv for kv in sorted(WORST.items()))))
        h.close()
    request.addfinalizer(report)
    _KH.append(h)
    return h


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- numerics
def rne16(x):
    """fp32 -> the fp32 value of its bf16 round-to-nearest-even (finite inputs)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return (b & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def bits16(x):
    """fp32 values that are bf16 numbers -> their bf16 bit patterns"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def from16(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda()
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    return torch.from_numpy(a).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


class Rows:
    """A (batch, time) row matrix as the kernels address it: entry q of M // rpb (+1), rows t0 .. t0 + rpb - 1 of `T`, `cols` used columns of
    `ld`.  Everything around the rows in use -- rows before t0, the gap behind each entry, the columns past `cols` -- is a guard."""

    def __init__(self, M, rpb, cols, bf16=False, t0=3, gap=5, pad=8, fill=None):
        self.M, self.rpb, self.cols, self.bf16, self.t0 = M, rpb, cols, bf16, t0
        self.nb = (M + rpb - 1) // rpb
        self.T, self.ld = t0 + rpb + gap, cols + pad
        if fill is None:
            self.h = np.full((self.nb, self.T, self.ld), SENT16 if bf16 else SENT32, dtype=np.uint16 if bf16 else np.uint32)
        else:
            self.h = fill
        self.d = None

    def rows(self):
        m = np.arange(self.M)
        return m // self.rpb, self.t0 + m % self.rpb

    def put(self, vals):
        """vals: [M][cols] float32 (bf16 numbers when bf16) written into the rows in use"""
        q, t = self.rows()
        v = np.asarray(vals, dtype=np.float32)
        self.h[q, t, :self.cols] = bits16(v) if self.bf16 else v.view(np.uint32)
        return self

    def upload(self):
        self.d = dev(self.h)
        return self

    def map(self, t0_shift=0):
        return (self.d.data_ptr(), self.T * self.ld, self.ld, self.t0 + t0_shift)

    def got(self):
        return host(self.d, np.uint16 if self.bf16 else np.uint32)

    def expect(self, vals, rows=None):
        """the whole buffer as it must come back: the sentinel, `vals` [M][cols] on the rows in use (or on the rows where `rows` is True)"""
        e = self.h.copy()
        q, t = self.rows()
        v = np.asarray(vals, dtype=np.float32)
        b = bits16(v) if self.bf16 else v.view(np.uint32)
        if rows is None:
            e[q, t, :self.cols] = b
        else:
            e[q[rows], t[rows], :self.cols] = b[rows]
        return e


def nan_rows(M, rpb, cols, vals, bf16=False, lo=0, hi=0, t0=3):
    """an input row matrix: `vals` on its rows, NaN everywhere else -- also on the rows a window hides (rem < lo, rem >= rpb - hi)"""
    r = Rows(M, rpb, cols, bf16=bf16, t0=t0)
    r.h[...] = 0x7FC0 if bf16 else 0x7FC00000
    v = np.array(vals, dtype=np.float32)
    rem = np.arange(M) % rpb
    hide = (rem < lo) | (rem >= rpb - hi)
    v[hide] = np.nan
    r.put(v)   # (bits16 of a NaN is a bf16 NaN)
    return r.upload()


def assert_bits(got, exp, what):
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError("%s: %d element(s) differ, first at %s: got %s, want %s" % (what, len(bad), tuple(bad[0]), hex(int(got[tuple(bad[0])])), hex(int(exp[tuple(bad[0])]))))


# The bound of the gate epilogue: wn_exp is accurate to ~1e-7 absolute on the exponent's range, the reciprocals to 1 ulp, tanh = 2 sigmoid(2f) - 1
# loses up to 2 ulp of 1 in the subtraction: |tanh - tanh64| <= 4e-7, |sigmoid - sigmoid64| <= 2e-7 (relative where tiny), |z - z64| <= 6e-7.
GATE_ABS = 1e-6


def _bounded(family, got, ref, rel16):
    """|got - ref| <= GATE_ABS + rel16 * |ref| (rel16 = 2^-8: a bf16 output adds half an ulp of its own)"""
    err = np.abs(got.astype(np.float64) - ref)
    ok = err <= GATE_ABS + rel16 * np.abs(ref)
    ok |= np.isnan(ref) & np.isnan(got)
    _worst(family, np.nanmax(np.where(np.isnan(ref), 0, err)) if err.size else 0)
    assert ok.all(), "%s: %d element(s) beyond the bound, worst %.3g" % (family, (~ok).sum(), np.nanmax(err))


def _check_gate_out(c, z, tag, is16):
    got = c.got()
    q, t = c.rows()
    vals = got[q, t, :c.cols]
    gz = from16(vals) if is16 else vals.view(np.float32)
    _bounded("gate z (bf16)" if is16 else "gate z", gz, z, 2.0 ** -8 if is16 else 0)
    e = c.h.copy()
    e[q, t, :c.cols] = vals
    assert_bits(got, e, tag + " guards")


def _gate64(v, N):
    F = np.concatenate([v[:, 64 * j:64 * j + 32] for j in range(N // 64)], axis=1)
    G = np.concatenate([v[:, 64 * j + 32:64 * j + 64] for j in range(N // 64)], axis=1)
    th, sg = np.tanh(F), 1 / (1 + np.exp(-G))
    return th * sg, th, sg


def _rounding_points(shape, rs):
    """fp32 values below, on (even and odd last bit) and above bf16 rounding points: b + f with b an 8-bit integer, scaled by 2^-7"""
    b = rs.randint(128, 256, shape).astype(np.float64)
    f = rs.choice([0.5 - 2.0 ** -16, 0.5, 0.5 + 2.0 ** -16, 0.25, 0.75, 0.0], shape)
    sgn = rs.choice([-1.0, 1.0], shape)
    return (sgn * (b + f) / 128).astype(np.float32)


def _pairwise(sizes, seed):
    """a covering selection: every pair of values of every two factors occurs in some case (greedy over seeded random candidates)"""
    rs = np.random.RandomState(seed)
    nf = len(sizes)
    need = {(a, i, b, j) for a in range(nf) for b in range(a + 1, nf) for i in range(sizes[a]) for j in range(sizes[b])}
    out = []
    while need:
        best, gain = None, -1
        for _ in range(64):
            cand = tuple(int(rs.randint(s)) for s in sizes)
            g = sum((a, cand[a], b, cand[b]) in need for a in range(nf) for b in range(a + 1, nf))
            if g > gain:
                best, gain = cand, g
        if gain <= 0:
            continue
        out.append(best)
        need -= {(a, best[a], b, best[b]) for a in range(nf) for b in range(a + 1, nf)}
    return out


# ---------------------------------------------------------------- one sampler on one part of a family (sampler_cases.py, sampler_filter_cases.py)
SMP_GUARD = 64
SMP_TAIL = 64                          # KF_TAIL of the harness
SMP_OTHER = np.uint32(0x7FC0BEEF)      # what the tail buffer holds before the launch (not the sentinel the kernel copies into it)
_SMP_DONE = {}


def sampler_launch(dll, kernel, part, filter_form=1, filt=None):
    """-> the indices of the part's rows, after the checks that need no expectation: guards, uniform lanes, the scratch's tail.  filt: (top_k, top_p)
    in place of the part's own; filter_form 0 with (0, 0.0): wn_sample_1w<false>, the product form (a part of sampler_cases carries no filter)"""
    GUARD, TAIL = SMP_GUARD, SMP_TAIL
    n, C = part.n, part.C
    per = 64 if kernel == "one_wave" else 1
    logits, u, greedy, temp = dev(part.logits), dev(part.u), dev(part.greedy), dev(part.temp)
    reg = dev(part.reg) if part.reg is not None else None
    top_k, top_p = filt if filt is not None else (part.top_k, part.top_p)
    out0 = np.full(GUARD + n * per + GUARD, SENT32, np.uint32)
    out = dev(out0)
    o_ptr = out.data_ptr() + 4 * GUARD
    if kernel == "one_wave":
        assert C == 256
        rc = dll.kf_sample_1w(_stream(), filter_form, n, top_k, top_p, logits.data_ptr(), reg.data_ptr() if reg is not None else None, u.data_ptr(), greedy.data_ptr(),
                              temp.data_ptr(), o_ptr)
    else:
        tail0 = np.full(GUARD + n * TAIL + GUARD, SMP_OTHER, np.uint32)
        tail = dev(tail0)
        rc = dll.kf_sample_generic(_stream(), n, C, top_k, top_p, logits.data_ptr(), reg.data_ptr() if reg is not None else None, u.data_ptr(), greedy.data_ptr(),
                                   temp.data_ptr(), o_ptr, tail.data_ptr() + 4 * GUARD)
    assert rc == 0, "HIP error %d" % rc
    torch.cuda.synchronize()
    got = host(out, np.uint32)
    assert_bits(got[:GUARD], out0[:GUARD], "%s: guard in front of the indices" % kernel)
    assert_bits(got[-GUARD:], out0[-GUARD:], "%s: guard behind the indices" % kernel)
    idx = got[GUARD:-GUARD].view(np.int32).reshape(n, per)
    if kernel == "one_wave":
        assert_bits(idx, np.repeat(idx[:, :1], 64, axis=1), "one_wave: the lanes of a row disagree")
    else:
        t = host(tail, np.uint32)
        want = tail0.copy()
        want[GUARD:-GUARD] = SENT32
        assert_bits(t, want, "generic C=%d: the %d floats behind the sampler scratch of %d floats" % (C, TAIL, dll.kf_smp_floats(C)))
    return idx[:, 0].copy()


LOGP_AT = 37      # the generic wrapper writes row r's value to out[r + at0]: at0 starts here, so that a wrong index lands in a guard band


def logp_launch(dll, kernel, parts, logp_mode, null_out=False):
    """The log-probability / forced wrappers (kf_logp_1w, kf_logp_generic) on a list of parts of one class count: ONE upload of the parts' rows, one launch
    per part (the run carries one regulariser and one filter), one synchronisation.  A part has C, reg, top_k, top_p, n, logits, temp, u, greedy and, where
    it forces classes, forced (int32 per row; absent: every position free).  logp_mode: r.logp's two low bits, 0 .. 2.
    -> [(indices, the uint32 words of the log-probabilities)] per part, after the checks that need no expectation: guards, uniform lanes, the scratch's
    tail, and that nothing but the rows' own floats changed -- nothing at all with logp_mode 0 or (generic, null_out) a NULL pointer in the status block."""
    GUARD, TAIL = SMP_GUARD, SMP_TAIL
    C = parts[0].C
    assert all(p.C == C for p in parts)
    per = 64 if kernel == "one_wave" else 1
    off = np.concatenate([[0], np.cumsum([p.n for p in parts])]).astype(np.int64)
    n = int(off[-1])
    logits = dev(np.concatenate([p.logits for p in parts]))
    u, greedy, temp = dev(np.concatenate([p.u for p in parts])), dev(np.concatenate([p.greedy for p in parts])), dev(np.concatenate([p.temp for p in parts]))
    forced = dev(np.concatenate([getattr(p, "forced", None) if getattr(p, "forced", None) is not None else np.full(p.n, -1, np.int32) for p in parts]))
    regs = {}
    for p in parts:
        if p.reg is not None and id(p.reg) not in regs:
            regs[id(p.reg)] = dev(p.reg)
    out0 = np.full(GUARD + n * per + GUARD, SENT32, np.uint32)
    out = dev(out0)
    stream = _stream()
    if kernel == "one_wave":
        assert C == 256
        lp0 = out0
        lp = dev(lp0)
    else:
        lp0 = np.full(GUARD + LOGP_AT + n + GUARD, SENT32, np.uint32)
        lp = dev(lp0)
        tail0 = np.full(GUARD + n * TAIL + GUARD, SMP_OTHER, np.uint32)
        tail = dev(tail0)
        status = dev(np.array([0, 0, 0, 0, 0, 0] + ([0, 0] if null_out else [(lp.data_ptr() + 4 * GUARD) & 0xFFFFFFFF, (lp.data_ptr() + 4 * GUARD) >> 32]), np.uint32))
    for p, o in zip(parts, off[:-1].tolist()):
        reg = regs[id(p.reg)].data_ptr() if p.reg is not None else None
        rows = (logits.data_ptr() + 4 * o * C, reg, u.data_ptr() + 8 * o, greedy.data_ptr() + 4 * o, temp.data_ptr() + 4 * o, forced.data_ptr() + 4 * o)
        if kernel == "one_wave":
            rc = dll.kf_logp_1w(stream, p.n, p.top_k, p.top_p, logp_mode, *rows, out.data_ptr() + 4 * (GUARD + 64 * o), lp.data_ptr() + 4 * (GUARD + 64 * o))
        else:
            rc = dll.kf_logp_generic(stream, p.n, C, p.top_k, p.top_p, logp_mode, status.data_ptr(), LOGP_AT + o, *rows, out.data_ptr() + 4 * (GUARD + o),
                                     tail.data_ptr() + 4 * (GUARD + TAIL * o))
        assert rc == 0, "HIP error %d" % rc
    torch.cuda.synchronize()
    what = "%s C=%d logp_mode %d" % (kernel, C, logp_mode)
    got, gl = host(out, np.uint32), host(lp, np.uint32)
    assert_bits(got[:GUARD], out0[:GUARD], what + ": guard in front of the indices")
    assert_bits(got[-GUARD:], out0[-GUARD:], what + ": guard behind the indices")
    idx = got[GUARD:-GUARD].view(np.int32).reshape(n, per)
    if kernel == "one_wave":
        assert_bits(gl[:GUARD], lp0[:GUARD], what + ": guard in front of the log-probabilities")
        assert_bits(gl[-GUARD:], lp0[-GUARD:], what + ": guard behind the log-probabilities")
        bits = gl[GUARD:-GUARD].reshape(n, 64)
        assert_bits(idx, np.repeat(idx[:, :1], 64, axis=1), what + ": the lanes of a row disagree on the index")
        assert_bits(bits, np.repeat(bits[:, :1], 64, axis=1), what + ": the lanes of a row disagree on the log-probability")
        bits = bits[:, 0].copy()
    else:
        lo = GUARD + LOGP_AT
        assert_bits(gl[:lo], lp0[:lo], what + ": the floats in front of out[at]")
        assert_bits(gl[lo + n:], lp0[lo + n:], what + ": the floats behind out[at]")
        bits = gl[lo:lo + n].copy()
        t = host(tail, np.uint32)
        want = tail0.copy()
        want[GUARD:-GUARD] = SENT32
        assert_bits(t, want, what + ": the %d floats behind the sampler scratch of %d floats" % (TAIL, dll.kf_smp_floats(C)))
    if logp_mode == 0 or (null_out and kernel != "one_wave"):
        assert_bits(bits, np.full(n, SENT32, np.uint32), what + ": a log-probability was written")
    idx = idx[:, 0].copy()
    return [(idx[a:b], bits[a:b]) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]


def sampler_run(dll, kernel, fam, filter_form=1, filt=None):
    """every part of a family through one sampler, once per process (both case tables have a family e: the form and the filter in the key tell them apart)"""
    key = (kernel, fam.kernel, fam.name, fam.C, filter_form, filt)
    if key not in _SMP_DONE:
        _SMP_DONE[key] = [sampler_launch(dll, kernel, part, filter_form, filt) for part in fam.parts]
    return _SMP_DONE[key]

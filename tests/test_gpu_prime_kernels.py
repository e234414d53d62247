"""The batched-priming kernels one at a time, through the product's own launchers and the grid expressions of wn_prime_pass (tests/kernels/
wn_kernel_harness.hip: kp_*), against the float64 / bit references of tests/prime_kernel_cases.py: the ragged products, the ragged start gather, the ring
fill at a queue time and the history gather.  The method is that of tests/test_gpu_kernels.py and tests/test_gpu_infer_kernels.py (exact / bounded; every
output inside sentinel guards that must come back untouched; NaN in every input row a kernel must not read); the helpers and the session fixture `kh`
are tests/kernel_lib.py's.  What the case data can tell -- sensitivity, the mutants of the row map and of the slot arithmetic -- is checked on the CPU
(tests/test_prime_kernel_cases_host.py), never by running an altered kernel.

Branch table: each hipLaunchKernelGGL line reached -> the cases (test ids) that take it.
  wn_launch_nn     wn_fwd_gemm_ragged<GATE>                 test_product[gate-*], test_same_bits_as_rectangle[gate2]
    (rg != NULL)   wn_fwd_gemm_ragged<PLAIN>                test_product[plain-*], test_same_bits_as_rectangle[plain]
  wn_launch_taps   wn_fwd_gemm_taps_ragged<3>               test_product[k3-*], test_same_bits_as_rectangle[taps3]
    (rg != NULL)   wn_fwd_gemm_taps_ragged<4>               test_product[k4-*]
  wn_prime_pass    wn_fwd_start_ragged                      test_fwd_start_ragged
                   wn_prime_gather_history                  test_gather_history, test_gather_then_fill_keeps_the_ring, test_rings_equal_as_maps_from_time
                   wn_fill_ring_at                          test_fill_ring_at, test_fill_ring_at_is_fill_ring_at_time_0, and behind both compositions
                   wn_fill_ring, wn_fwd_start               tests/test_gpu_infer_kernels.py (test_fill_ring_at_is_fill_ring_at_time_0 launches the first as its yardstick)
  (wn_launch_nn / wn_launch_taps with rg == NULL -- the rectangle's kernels, the yardsticks of test_same_bits_as_rectangle: tests/test_gpu_kernels.py,
   tests/test_gpu_infer_kernels.py.)
"""
import time

import numpy as np
import pytest
import torch

import prime_kernel_cases as pk
from kernel_lib import NOMAP, SENT32, WALL, Rows, _check_gate_out, _pairwise, _stream, assert_bits, dev, host
from kernel_lib import kh  # noqa: F401  (the session fixture)

pytestmark = pytest.mark.gpu

NAN32 = pk.NAN32
PRODUCTS = pk.product_cases(_pairwise)
TABLE_GUARD = np.int32(0x40000000)   # around a row table: a start the search must never load


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    """the module's wall time, for the harness's closing line (which also carries the worst errors of this module's bounded families)"""
    t0 = time.time()
    yield
    WALL["test_gpu_prime_kernels"] = time.time() - t0


def _ptr(t):
    return None if t is None else t.data_ptr()


def _table(start):
    """a row table on the device between two guards -> (tensor, pointer to start[0])"""
    h = np.concatenate([np.full(4, TABLE_GUARD, np.int32), np.asarray(start, np.int32), np.full(4, TABLE_GUARD, np.int32)])
    d = dev(h)
    return d, d.data_ptr() + 16


class _Out:
    """an output addressed by (stream, time) inside its sentinels, with what _check_gate_out asks of a row matrix"""

    def __init__(self, lay, s, t):
        self.lay, self.cols, self.s, self.t = lay, lay.cols, s, t
        self.h = lay.full(SENT32)
        self.d = dev(self.h)

    def map(self):
        return self.lay.map(self.d.data_ptr())

    def rows(self):
        return self.s, self.t + self.lay.pre

    def got(self):
        return host(self.d, np.uint32)


def _launch_product(kh, p, c):
    """one ragged product of a case into `c` -> the device tensors it reads (kept alive by the caller until the synchronize)"""
    xd = dev(p.x)
    bt = dev(np.ascontiguousarray(p.W.T))
    b_d = dev(p.bvec) if p.bvec is not None else None
    tab_d, tab_p = _table(p.tab.start)
    base, bs, rs, _ = p.xl.map(xd.data_ptr())
    keep = [xd, bt, b_d, tab_d]
    rg = (tab_p, p.tab.ns, p.tab.n)
    if p.kind == "gate2":
        kh.call("kp_nn_ragged", _stream(), pk.GATE, base, bs, rs, -p.d, base, bs, rs, 0, p.K1, p.K, bt.data_ptr(), p.N, _ptr(b_d), *NOMAP, *c.map(), p.tab.M, *rg)
    elif p.kind == "taps":
        kh.call("kp_taps_ragged", _stream(), p.taps, base, bs, rs, 0, p.d, p.t_min, p.K1, bt.data_ptr(), p.N, _ptr(b_d), *c.map(), p.tab.M, *rg)
    else:
        cin = dev(p.cin)
        keep.append(cin)
        kh.call("kp_nn_ragged", _stream(), pk.PLAIN, base, bs, rs, 0, base, bs, rs, 0, p.K, p.K, bt.data_ptr(), p.N, _ptr(b_d), *p.cl.map(cin.data_ptr()), *c.map(),
                p.tab.M, *rg)
    return keep


# ================================================================ a. the ragged products
@pytest.mark.parametrize("cid,kind,kw", PRODUCTS, ids=[c[0] for c in PRODUCTS])
def test_product(kh, cid, kind, kw):
    """PLAIN (bias, cin = x(t)): bit for bit; GATE: within GATE_ABS of float64; the sentinel everywhere but the table's own (stream, time) rows"""
    p = pk.product(cid, kw)
    p.check_sensitive()   # (on the CPU, before the launch: data that could not tell a wrong row map would make the comparison below worthless)
    c = _Out(p.ol, p.s, p.t)
    keep = _launch_product(kh, p, c)
    torch.cuda.synchronize()
    del keep
    if p.epi == pk.PLAIN:
        assert_bits(c.got(), p.expect_plain(), p.tag + " x'")
    else:
        _check_gate_out(c, p.ref, p.tag + " z", False)


RECT = {"gate2": dict(kind="gate2", K1=128, N=192, d=7, taps=2), "plain": dict(kind="plain", K1=128, N=160), "taps3": dict(kind="taps", K1=96, N=192, d=7, taps=3)}


@pytest.mark.parametrize("form", list(RECT))
def test_same_bits_as_rectangle(kh, form):
    """standard_normal data: the ragged product's row for (s, t) is, bit for bit, the row the rectangle's kernel (kh_nn / kh_taps) computes for the same
    inputs over that stream alone, where the row stands at another place of another tile"""
    tab = pk.TABLES["b"]
    p = pk.Product(tab=tab, bias=True, seed=5, data="normal", **RECT[form])
    c = _Out(p.ol, p.s, p.t)
    keep = _launch_product(kh, p, c)
    xd, bt, b_d = keep[0], keep[1], keep[2]
    torch.cuda.synchronize()
    got = c.got()
    e = c.h.copy()
    e[c.rows() + (slice(0, c.cols),)] = got[c.rows() + (slice(0, c.cols),)]
    assert_bits(got, e, p.tag + " guards")
    for s in range(tab.ns):
        rows, f = tab.rows[s], tab.first_time(s)
        if rows == 0:
            continue
        r = Rows(rows, rows, p.ncols, t0=2, gap=3).upload()
        base, bs, rs, _ = p.xl.map(xd.data_ptr())
        base += 4 * s * bs
        if p.kind == "gate2":
            kh.call("kh_nn", _stream(), pk.GATE, base, bs, rs, f - p.d, base, bs, rs, f, p.K1, p.K, bt.data_ptr(), None, p.N, _ptr(b_d), *NOMAP, *r.map(), rows, rows,
                    0, 0, None, None, None, *NOMAP, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, None, None, 0)
        elif p.kind == "taps":
            kh.call("kh_taps", _stream(), p.taps, base, bs, rs, f, p.d, p.t_min, p.K1, bt.data_ptr(), p.N, _ptr(b_d), *r.map(), rows, rows, *NOMAP, 0, None, None, 0)
        else:
            cb, cbs, crs, _ = p.cl.map(keep[4].data_ptr())
            kh.call("kh_nn", _stream(), pk.PLAIN, base, bs, rs, f, base, bs, rs, f, p.K, p.K, bt.data_ptr(), None, p.N, _ptr(b_d), cb + 4 * s * cbs, cbs, crs, f, *r.map(),
                    rows, rows, 0, 0, None, None, None, *NOMAP, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, None, None, 0)
        torch.cuda.synchronize()
        rect = r.got()
        want = got[s, p.ol.pre + f:p.ol.pre + tab.n, :p.ncols]
        assert not (want == SENT32).any() and not (want.view(np.float32) != want.view(np.float32)).any(), p.tag + ": a row of stream %d is missing or NaN" % s
        assert_bits(rect, r.expect(want.view(np.float32)), "%s: stream %d alone (%d rows)" % (p.tag, s, rows))
    del keep


# ================================================================ b. the copy kernels (bit exact)
@pytest.mark.parametrize("cid,kw", pk.start_cases(), ids=[c[0] for c in pk.start_cases()])
def test_fwd_start_ragged(kh, cid, kw):
    """x(s, n - n_s + j) = start_conv column idx[s][j] (+ bias); the pad behind a stream's length is a class whose column is NaN"""
    c = pk.StartCase(**kw)
    want, esc = c.image()
    assert esc == 0
    x = dev(c.xl.full(SENT32))
    i_d, s_d, b_d = dev(c.idx), dev(c.start_t), dev(c.bvec) if c.bvec is not None else None
    tab_d, tab_p = _table(c.tab.start)
    base, bs, _, _ = c.xl.map(x.data_ptr())
    kh.call("kp_fwd_start_ragged", _stream(), i_d.data_ptr(), c.idx_stride, s_d.data_ptr(), _ptr(b_d), base, bs, tab_p, c.tab.ns, c.tab.n, c.tab.M, c.R)
    torch.cuda.synchronize()
    assert_bits(host(x, np.uint32), want, c.tag)


def _ring(P, ns, ML, R, init=None, guard=64):
    """a ring [P][ns][ML][R] between two guards -> (tensor, pointer to the ring, the host image)"""
    h = np.full(P * ns * ML * R + 2 * guard, SENT32, np.uint32)
    if init is not None:
        h[guard:-guard] = init.ravel()
    d = dev(h)
    return d, d.data_ptr() + 4 * guard, h


def _fill_at(kh, c, ring_p, count=None, t_base=None):
    xd = dev(c.x)
    base, bs, _, _ = c.xl.map(xd.data_ptr())
    kh.call("kp_fill_ring_at", _stream(), base, 0 if c.shared else bs, ring_p, c.R, c.ML, c.ns, c.P, c.n_time, c.ML if count is None else count,
            c.t_base if t_base is None else t_base)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shared", [False, True], ids=["own", "shared"])
@pytest.mark.parametrize("P,ns,R", pk.FILL_SHAPES)
@pytest.mark.parametrize("ML", pk.FILL_ML)
def test_fill_ring_at(kh, ML, P, ns, R, shared):
    """count = ML: the pass times [n_time - ML, n_time), negative ones included, to slot (t_base + t) mod ML of all P copies, at queue times up to
    2^62 - n_time - 1; the reference slot is Python's integer arithmetic"""
    for c in pk.fill_cases(ML, P, ns, R, shared):
        want, esc = c.image()
        assert esc == 0
        ring = _ring(P, ns, ML, R)
        _fill_at(kh, c, ring[1])
        e = ring[2].copy()
        e[64:-64] = want.ravel()
        assert_bits(host(ring[0], np.uint32), e, c.tag)


@pytest.mark.parametrize("P,ns,R", pk.FILL_SHAPES)
@pytest.mark.parametrize("ML", pk.FILL_ML)
def test_fill_ring_at_is_fill_ring_at_time_0(kh, ML, P, ns, R):
    """t_base = 0 and count = min(ML, n_time): wn_fill_ring's bytes"""
    for n_time in pk.fill_times(ML):
        c = pk.FillCase(ML, n_time, 0, P, ns, R, False, seed=n_time)
        count = min(ML, n_time)
        a, b = _ring(P, ns, ML, R), _ring(P, ns, ML, R)
        _fill_at(kh, c, a[1], count=count)
        xd = dev(c.x)
        base, bs, _, _ = c.xl.map(xd.data_ptr())
        kh.call("kh_fill_ring", _stream(), base, bs, b[1], R, ML, ns, P, n_time, count)
        torch.cuda.synchronize()
        e = a[2].copy()
        w = e[64:-64].reshape(P, ns, ML, R)
        for t in range(n_time - count, n_time):
            w[:, :, t % ML] = c.X[:, c.xl.pre + t].view(np.uint32)[None]
        assert_bits(host(a[0], np.uint32), e, c.tag + " count %d" % count)
        assert_bits(host(b[0], np.uint32), e, "wn_fill_ring, " + c.tag)


def _gather(kh, c, ring_d, x_d, start=None):
    tab = _table(start if start is not None else c.start) if (start is not None or c.start is not None) else (None, None)
    base, bs, _, _ = c.xl.map(x_d.data_ptr())
    kh.call("kp_gather_history", _stream(), ring_d.data_ptr(), c.R, c.ML, c.ns, base, bs, c.Lp, c.n, c.t_base, tab[1])
    torch.cuda.synchronize()


@pytest.mark.parametrize("R", [32, 96])
@pytest.mark.parametrize("ML", pk.GATHER_ML)
def test_gather_history(kh, ML, R):
    """history row j = 1 .. ML, ring slot (t_base - j) mod ML of copy 0, to the pass time (n - n_append[s]) - j; the row below -Lp dropped, the guard in
    front of row -Lp untouched; a NULL table and tables with n_append = 0 and = n; t_base - j negative at the small queue times"""
    for c in pk.gather_cases(ML, R):
        want, esc, _ = c.image()
        assert esc == 0
        x = dev(c.xl.full(SENT32))
        _gather(kh, c, dev(c.ring), x)
        assert_bits(host(x, np.uint32), want, c.tag)


@pytest.mark.parametrize("n", ["0", "2ML"])
@pytest.mark.parametrize("ML", [3, 17])
def test_gather_then_fill_keeps_the_ring(kh, ML, n):
    """on the largest queue time: a gather with n_append = 0 everywhere, then wn_fill_ring_at with count = ML, leaves the ring's bytes as they were (the
    pass adds a multiple of ML to every row's time)"""
    n = {"0": 0, "2ML": 2 * ML}[n]
    ns, R, P = 3, 32, 2
    t_base = pk.T62 - n - 1
    c = pk.GatherCase(ML, ML + 3, n, t_base, [0] * ns, ns, R, seed=ML)
    vals = np.repeat(c.V.view(np.uint32)[None], P, axis=0)   # both copies hold the queues, as a handle's do
    ring = _ring(P, ns, ML, R, init=vals)
    x = dev(c.xl.full(NAN32))
    tab_d, tab_p = _table(c.start)
    base, bs, _, _ = c.xl.map(x.data_ptr())
    kh.call("kp_gather_history", _stream(), ring[1], R, ML, ns, base, bs, c.Lp, n, t_base, tab_p)
    kh.call("kp_fill_ring_at", _stream(), base, bs, ring[1], R, ML, ns, P, n, ML, t_base)
    torch.cuda.synchronize()
    assert_bits(host(ring[0], np.uint32), ring[2], "gather + fill at t_base 2^62 - %d - 1, ML %d" % (n, ML))
    xs = host(x, np.uint32)
    assert (xs != NAN32).any(axis=2).sum() == ns * ML, "the gather wrote other rows than the ML of every stream"


@pytest.mark.parametrize("ML", [3, 17])
def test_rings_equal_as_maps_from_time(kh, ML):
    """one logical history and one set of appended rows at the queue times 5 and 2^40 + 5: after gather + fill the two rings are the same map from
    time to row -- row i below the new queue time is the appended row, or the history row, that stands there"""
    ns, R, P, n = 3, 32, 2, 5
    n_append = [0, n, 2]
    rs = np.random.RandomState(ML)
    H = rs.standard_normal((ns, ML + 1, R)).astype(np.float32)   # H[s][i]: the i-th newest row of the history, i = 1 .. ML
    A = rs.standard_normal((ns, n, R)).astype(np.float32)        # A[s][t]: the appended row at pass time t (t >= n - n_append[s])
    maps = []
    for t_base in (5, 2 ** 40 + 5):
        c = pk.GatherCase(ML, ML + 3, n, t_base, n_append, ns, R)
        r0 = np.empty((P, ns, ML, R), np.float32)
        for i in range(1, ML + 1):
            r0[:, :, pk.ring_slot(t_base - i, ML)] = H[None, :, i]
        ring = _ring(P, ns, ML, R, init=r0.view(np.uint32))
        xh = c.xl.full(NAN32)
        for s, a in enumerate(n_append):
            xh[s, c.xl.pre + n - a:c.xl.pre + n, :R] = A[s, n - a:].view(np.uint32)
        x = dev(xh)
        tab_d, tab_p = _table(c.start)
        base, bs, _, _ = c.xl.map(x.data_ptr())
        kh.call("kp_gather_history", _stream(), ring[1], R, ML, ns, base, bs, c.Lp, n, t_base, tab_p)
        kh.call("kp_fill_ring_at", _stream(), base, bs, ring[1], R, ML, ns, P, n, ML, t_base)
        torch.cuda.synchronize()
        g = host(ring[0], np.uint32)
        assert (g[:64] == SENT32).all() and (g[-64:] == SENT32).all(), "ring guards"
        g = g[64:-64].reshape(P, ns, ML, R)
        maps.append(np.stack([g[:, :, pk.ring_slot(t_base + n - i, ML)] for i in range(1, ML + 1)], axis=2))   # [P][ns][i - 1][R]
    want = np.empty((P, ns, ML, R), np.uint32)
    for s, a in enumerate(n_append):
        for i in range(1, ML + 1):
            want[:, s, i - 1] = (A[s, n - i] if i <= a else H[s, i - a]).view(np.uint32)[None]
    assert_bits(maps[0], want, "ring at t_base 5 as a map from time, ML %d" % ML)
    assert_bits(maps[1], maps[0], "ring at t_base 2^40 + 5 against the ring at 5, ML %d" % ML)

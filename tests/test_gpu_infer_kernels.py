"""The inference kernels one at a time, through the product's own launchers and launch geometry (tests/kernels/wn_kernel_harness.hip includes
csrc/wn_runtime.hip), against float64 references: the tap product of kernel_size 3 / 4, the score kernels, the ring fill and the small layout
kernels.  The method is that of tests/test_gpu_kernels.py, the helpers and the session fixture `kh` are tests/kernel_lib.py's (exact / rounding /
bounded; every output inside sentinel guards that must come back untouched; NaN in every input row a kernel must not read).

Branch table: each hipLaunchKernelGGL line reached -> the cases (test ids) that take it.
  wn_launch_taps   wn_fwd_gemm_taps<3>                      test_taps[k3-*], test_taps_gates[k3-*], test_taps_t_min[k3-*]
                   wn_fwd_gemm_taps<4>                      test_taps[k4-*], test_taps_gates[k4-*], test_taps_t_min[k4-*]
  wn_forward_run   wn_score_head                            test_score_head[f32-*], test_score_head_null_outputs[f32], test_score_rows[C256-*] (its yardstick)
                   wn_score_head_bf16                       test_score_head[bf16-*], test_score_head_null_outputs[bf16], test_score_head_bf16_rounding
                   wn_score_rows                            test_score_rows
                   wn_score_reduce                          test_score_reduce, and behind every score case above
                   wn_fwd_start                             test_fwd_start
  wn_prime         wn_fill_ring                             test_fill_ring
  wn_train.inl     wn_cvt_bf16                              test_cvt_bf16
                   wn_cvt_bf16_transposed                   test_transposes[cvt-*]
                   wn_transpose_batched                     test_transposes[f32-*]
(The batched-priming kernels -- the ragged products, wn_fwd_start_ragged, wn_fill_ring_at, wn_prime_gather_history: tests/test_gpu_prime_kernels.py, with a table of its own.)

What the score kernels can show of their logits: the first argmax (every row), logits[target] and the logsumexp through row_nll, and the counts.  The
exact cases therefore use integer logits (ties are frequent and planted) and hold row_pred and the counts exactly and row_nll to NLL bound below.
"""
import math
import time

import numpy as np
import pytest
import torch

from kernel_lib import (GATE_ABS, NOMAP, SENT16, SENT32, WALL, Rows, _bounded, _check_gate_out, _gate64, _pairwise, _rounding_points, _stream, _worst, assert_bits, bits16,
                        dev, from16, host, rne16)
from kernel_lib import kh  # noqa: F401  (the session fixture)
from parity_common import LOGIT_RTOL
from prime_kernel_cases import start_values as _start_values   # (shared with wn_fwd_start_ragged's cases)

pytestmark = pytest.mark.gpu

NAN32 = np.uint32(0x7FC00000)
SENT64 = np.uint64(0x7FF8DEADDEADDEAD)   # sentinel of fp64 outputs
SENTI = np.int32(0x7FC0DEAD)             # ... of int32 outputs


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    """the module's wall time, for the harness's closing line (which also carries the worst errors of this module's bounded families)"""
    t0 = time.time()
    yield
    WALL["test_gpu_infer_kernels"] = time.time() - t0


def _ptr(t):
    return None if t is None else t.data_ptr()


def _guarded(n, sentinel, dtype, guard=16):
    """a device vector of n elements between two guards of `guard` sentinels: (tensor, pointer to element 0, the host image)"""
    hst = np.full(n + 2 * guard, sentinel, dtype)
    d = dev(hst.view(np.int64) if hst.dtype == np.uint64 else hst)
    return d, d.data_ptr() + guard * hst.itemsize, hst


# ================================================================ a. the tap product (wn_launch_taps: wn_fwd_gemm_taps<3>, <4>)
TAP_SHAPES = [(1, 1), (127, 50), (128, 100), (129, 129), (383, 97)]   # (M, rows_per_batch): tiles that span batch entries, ragged last tiles
TAP_R = [32, 64, 96, 128]        # 2 .. 8 K chunks of WN_GEMM_KC = 16 per view: the view switch falls on both LDS buffers
TAP_N = [64, 128, 192, 256]      # a partial only tile, one full tile, a partial second tile, two full tiles
TAP_D = [1, 2, 7, "big"]         # tap distance; big = rows_per_batch + 3
TAP_C2 = ["first", "mid", "last"]


def _taps_case(kh, taps, M, rpb, R, N, d, bias, c2_first, gates=None, t0=None, t_min=0, zero_prefix=0, seed=0):
    """z = gate([x(t - (taps-1) d) | ... | x(t)] . Wfg^T + b) on M rows in entries of rpb; x(t) reads as zero for t < t_min.  Row times count from the
    first row of an entry that the forward would own (0); `zero_prefix` rows before it hold real zeros (wn_prime's form), every other row that no tap
    of this case may read holds NaN: the slack below the oldest tap, the gap behind an entry, the rows before t_min."""
    rs = np.random.RandomState(seed)
    k1 = taps - 1
    reach = k1 * d
    if t0 is None:
        t0 = reach + 2   # (slack: two rows below the oldest tap of the first row)
    K = taps * R
    assert K * 256 < 2 ** 24   # integers / 64: every product and partial sum is an exact multiple of 2^-12 below 2^12
    nb = (M + rpb - 1) // rpb
    pre = max(0, reach - t0, zero_prefix) + 2          # physical rows before time 0
    T, ld = pre + t0 + rpb + 3, R + 8
    tau = np.arange(T) - pre
    Xf = rs.randint(-16, 17, (nb, T, R)).astype(np.float32) / 64
    if zero_prefix:
        Xf[:, tau < 0] = 0
    W = rs.randint(-16, 17, (N, K)).astype(np.float32) / 64
    bvec = rs.randint(-8, 9, N).astype(np.float64) / 64 if bias else np.zeros(N)
    m = np.arange(M)
    q, rem = m // rpb, m % rpb
    first_read = max(t_min, t0 - reach)
    xh = np.full((nb, T, ld), NAN32, np.uint32)
    for e in range(nb):
        n_e = min(rpb, M - e * rpb)
        ok = (tau >= first_read) & (tau < t0 + n_e)
        xh[e, ok, :R] = Xf[e, ok].view(np.uint32)
    X64 = Xf.astype(np.float64)

    def view(j, shift=0):   # view j (0 = the oldest tap) of every row; `shift` moves the rows it reads, not the rows that exist
        tj = t0 + rem - (k1 - j) * d
        v = X64[q, pre + tj + shift]
        return np.where((tj >= t_min)[:, None], v, 0.0)

    W64 = W.astype(np.float64)

    def z_of(views):
        acc = sum(views[j] @ W64[:, j * R:(j + 1) * R].T for j in range(taps))
        return _gate64(acc + bvec, N)

    views = [view(j) for j in range(taps)]
    z, th, sg = z_of(views)
    # sensitivity of the data (a condition on the inputs): each wrong product moves z by >= 1000 GATE_ABS somewhere in every 128-row tile
    wrong = {"views reversed": views[::-1]}
    for j in range(taps):
        wrong["view %d zeroed" % j] = views[:j] + [np.zeros_like(views[j])] + views[j + 1:]
        for s in (-1, 1):
            wrong["view %d shifted %+d" % (j, s)] = views[:j] + [view(j, s)] + views[j + 1:]
    for name, vs in wrong.items():
        dz = np.abs(z_of(vs)[0] - z).max(axis=1)
        for r0 in range(0, M, 128):
            assert dz[r0:r0 + 128].max() >= 1000 * GATE_ABS, "the data cannot tell '%s' in the tile at row %d (seed %d)" % (name, r0, seed)

    xd = dev(xh)
    xmap = (xd.data_ptr() + 4 * pre * ld, T * ld, ld, t0)
    bt = dev(np.ascontiguousarray(W.T))
    b_d = dev(bvec.astype(np.float32)) if bias else None
    c = Rows(M, rpb, N // 2, t0=5, gap=7).upload()
    c2r = None
    if c2_first is not None:
        nrow2 = rpb - c2_first
        c2r = Rows(nb * nrow2, nrow2, N // 2, t0=2, gap=3).upload()
    gt = gg = None
    if gates:
        gt = dev(np.full((M + 1, N // 2), SENT32, np.uint32))
        gg = dev(np.full((M + 1, N // 2), SENT32, np.uint32)) if gates == "f32" else None
    tag = "taps %d M %d rpb %d R %d N %d d %d t0 %d t_min %d" % (taps, M, rpb, R, N, d, t0, t_min)
    kh.call("kh_taps", _stream(), taps, *xmap, d, t_min, R, bt.data_ptr(), N, _ptr(b_d), *c.map(), M, rpb, *(c2r.map() if c2r else NOMAP),
            c2_first or 0, _ptr(gt), _ptr(gg), int(gates == "packed"))
    torch.cuda.synchronize()
    _check_gate_out(c, z, tag + " z", False)
    if c2r is not None:
        on = rem >= c2_first
        got = c2r.got()
        ev = c2r.h.copy()
        qq, tt = q[on], c2r.t0 + rem[on] - c2_first
        ref = c.got()[q[on], c.t0 + rem[on], :N // 2]
        assert np.array_equal(got[qq, tt, :N // 2], ref), tag + ": c2 is not the copy of z on the skip rows"
        ev[qq, tt, :N // 2] = ref
        assert_bits(got, ev, tag + " c2 guards")
    if gates:
        g = host(gt, np.uint32)
        assert (g[M] == SENT32).all(), tag + ": the gates run past row M"
        if gates == "packed":
            _bounded("gate tanh (bf16)", from16(g[:M] & 0xFFFF), th, 2.0 ** -8)
            _bounded("gate sigmoid (bf16)", from16(g[:M] >> 16), sg, 2.0 ** -8)
        else:
            g2 = host(gg, np.uint32)
            assert (g2[M] == SENT32).all(), tag + ": the gates run past row M"
            _bounded("gate tanh", g[:M].view(np.float32), th, 0)
            _bounded("gate sigmoid", g2[:M].view(np.float32), sg, 0)


def _tap_cases(taps):
    cases = []
    for si, ri, ni, di, bi, ci in _pairwise([len(TAP_SHAPES), len(TAP_R), len(TAP_N), len(TAP_D), 2, len(TAP_C2)], seed=taps):
        M, rpb = TAP_SHAPES[si]
        d = rpb + 3 if TAP_D[di] == "big" else TAP_D[di]
        c2 = {"first": 0, "mid": rpb // 2, "last": rpb - 1}[TAP_C2[ci]]
        cid = "k%d-M%d-R%d-N%d-d%s-b%d-c2%s" % (taps, M, TAP_R[ri], TAP_N[ni], TAP_D[di], bi, TAP_C2[ci])
        cases.append(pytest.param(taps, M, rpb, TAP_R[ri], TAP_N[ni], d, bool(bi), c2, id=cid))
    return cases


@pytest.mark.parametrize("taps,M,rpb,R,N,d,bias,c2_first", _tap_cases(3) + _tap_cases(4))
def test_taps(kh, taps, M, rpb, R, N, d, bias, c2_first):
    """gate_t == NULL, t_min = 0 below every tap (as wn_forward runs it)"""
    _taps_case(kh, taps, M, rpb, R, N, d, bias, c2_first, seed=1000 * taps + M + R + N + d)


@pytest.mark.parametrize("gates", ["f32", "packed"])
@pytest.mark.parametrize("taps", [3, 4], ids=["k3", "k4"])
def test_taps_gates(kh, taps, gates):
    """the saved gates written too (two fp32 matrices / one packed bf16 pair per element), M not a multiple of the tile"""
    _taps_case(kh, taps, 129, 43, 64, 192, 2, True, 11, gates=gates, seed=7 * taps)


TMIN = {   # id -> (t0, t_min, zero prefix) as functions of (d, taps - 1); t0 < the oldest tap's reach except in the prime form
    "t0": lambda d, k1: (3, 3, 0),                                   # nothing before the first row exists
    "t0-d": lambda d, k1: (3, 3 - d, 0),                             # one tap distance of history exists
    "reach+1": lambda d, k1: (3, 3 - k1 * d + 1, 0),                 # only the oldest tap of an entry's first row is missing
    "prime": lambda d, k1: (0, -(k1 * d + 5), k1 * d + 5),           # wn_prime: t_min = -Lp, a real zero prefix of Lp >= reach rows
}


@pytest.mark.parametrize("shape", [(127, 50, 32, 64, 7), (383, 97, 96, 192, 4)], ids=["M127", "M383"])
@pytest.mark.parametrize("form", list(TMIN))
@pytest.mark.parametrize("taps", [3, 4], ids=["k3", "k4"])
def test_taps_t_min(kh, taps, form, shape):
    """the predicate that turns a row before the first existing row of a batch entry into zeros: those rows hold NaN in memory"""
    M, rpb, R, N, d = shape
    t0, t_min, prefix = TMIN[form](d, taps - 1)
    _taps_case(kh, taps, M, rpb, R, N, d, True, rpb // 2, t0=t0, t_min=t_min, zero_prefix=prefix, seed=31 * taps + M)


# ================================================================ b. the score kernels
# NLL bound, from the arithmetic of wn_score_strip / wn_score_rows on exact logits x (|x| <= L): mx and x - mx are exact;
#   sum = fp32 sum of <= 256 terms expf(x - mx) in (0, 1], each within 2 ulp, over <= 13 additions deep (8 in the lane, 5 or 6 across lanes; all terms
#         positive): relative error <= (2 + 13) 2^-24, which is also its share of log(sum);
#   logf(sum) within 2 ulp of a value <= log 256 < 8: <= 2 * 2^-21 = 16 * 2^-24;
#   lse = mx + logf(sum), rounded once: <= 2^-24 (L + 5.6);  nll = lse - x[target], rounded once: <= 2^-24 (2 L + 5.6).
# Together 2^-24 (15 + 16 + 11.2 + 3 L) <= 2^-24 (43 + 3 L): 8.3e-6 at L = 32.  The end-to-end bar of tests/test_gpu_score.py is 2 LOGIT_RTOL max(1, L).
def _nll_bound(L):
    b = 2.0 ** -24 * (43 + 3 * L)
    assert b <= 2 * LOGIT_RTOL * max(1.0, L), "the derived bound exceeds the end-to-end bar"
    return b


def _nll64(lg, tgt, C):
    """(nll of the valid rows in float64 -- NaN on the others --, validity, first argmax)"""
    lg = np.asarray(lg, np.float64)
    valid = (tgt >= 0) & (tgt < C)
    mx = lg.max(axis=1)
    with np.errstate(divide="ignore"):
        lse = mx + np.log(np.exp(lg - mx[:, None]).sum(axis=1))
    nll = np.full(lg.shape[0], np.nan)
    nll[valid] = lse[valid] - lg[valid, tgt[valid]]
    return nll, valid, lg.argmax(axis=1)


CTRL = [0, 31, 32, 70, 71, 102, 255]   # classes with a skip channel of their own (channel i -> end channel i -> class CTRL[i]): planted ties
HEAD_TIES = {3: (70, 71), 4: (70, 102), 5: (31, 32), 6: (0, 255)}   # row kind (m % 8) -> two lanes of a tile, two tiles of a lane, lane 31 | 32, first | last


def _head_data(S, E, M, seed):
    """Integer operands with exact integer h and logits, |logits| <= 32: skip in -3 .. 3 (the staged ReLU matters), W1 four +-1 per end channel, b1 in
    -2 .. 2 (the ReLU of h matters), W2 one +1 and one -1 per class, b2 = -relu(b1) . W2 so that a row with no positive skip has 256 equal logits."""
    rs = np.random.RandomState(seed)
    nc = len(CTRL)
    skip = rs.randint(-3, 4, (M, S)).astype(np.float64)
    skip[:, :nc] = rs.randint(-3, 1, (M, nc))
    W1 = np.zeros((S, E))
    W2 = np.zeros((E, 256))
    b1 = rs.randint(-2, 3, E).astype(np.float64)
    b1[:nc] = 0
    srows = np.concatenate([rs.permutation(np.arange(nc, S)) for _ in range(4 * E // (S - nc) + 2)])   # every skip channel used, about equally often
    for e in range(nc, E):
        for s in srows[4 * (e - nc):4 * (e - nc) + 4]:
            W1[s, e] += rs.choice([-1.0, 1.0])
    erows = np.concatenate([rs.permutation(np.arange(nc, E)) for _ in range(2 * 256 // (E - nc) + 2)])   # every end channel used
    for c in range(256):
        W2[erows[2 * c], c] += 1
        W2[erows[2 * c + 1], c] -= 1
    for i, c in enumerate(CTRL):
        W1[i, i] = 1
        W2[i, c] += 1
    b2 = -(np.maximum(b1, 0) @ W2)
    kind = np.arange(M) % 8
    skip[kind == 7] = -np.abs(skip[kind == 7])   # all-equal rows

    def logits_of(sk, h_map=lambda h: h):
        h = np.maximum(np.maximum(sk, 0) @ W1 + b1, 0)
        return h, h_map(h) @ W2 + b2

    _, base = logits_of(skip)
    for k, (a, b) in HEAD_TIES.items():
        rows = np.nonzero(kind == k)[0]
        top = base[rows].max(axis=1)
        skip[rows, CTRL.index(a)] = top + 1 - base[rows, a]
        skip[rows, CTRL.index(b)] = top + 1 - base[rows, b]
    h, lg = logits_of(skip)
    assert np.array_equal(h, np.rint(h)) and np.array_equal(lg, np.rint(lg)) and h.max() < 256 and np.abs(lg).max() <= 32, "case leaves the exact range"
    if M >= 8:
        for k, (a, b) in HEAD_TIES.items():
            r = np.nonzero(kind == k)[0][0]
            assert lg[r, a] == lg[r, b] == lg[r].max() and (lg[r] == lg[r].max()).sum() == 2
        assert (lg[kind == 7] == 0).all()
    return dict(skip=skip.astype(np.float32), W1=W1.astype(np.float32), W2=W2.astype(np.float32), b1=b1.astype(np.float32), b2=b2.astype(np.float32),
                logits=lg, h=h, kind=kind, logits_of=logits_of)


def _targets(lg, rs, C):
    """targets: a third hit the first argmax, tied rows aim at the LATER maximum, three invalid ones (-1, C, 2^40) where the rows allow"""
    M = lg.shape[0]
    pred = lg.argmax(axis=1)
    tgt = rs.randint(0, C, M).astype(np.int64)
    hit = rs.rand(M) < 0.33
    tgt[hit] = pred[hit]
    last = C - 1 - lg[:, ::-1].argmax(axis=1)
    later = (last != pred) & (rs.rand(M) < 0.5)
    tgt[later] = last[later]
    for r, bad in zip((1, M // 2, M - 1) if M >= 8 else (), (-1, C, 2 ** 40)):
        tgt[r] = bad
    return tgt


class _ScoreOut:
    """row_nll / row_pred / part of one scoring launch inside their guards, and the sums of wn_score_reduce over `part`"""

    def __init__(self, M, n_part, nll=True, pred=True):
        self.M, self.n_part = M, n_part
        self.nll = _guarded(M, SENT32, np.uint32) if nll else None
        self.pred = _guarded(M, SENTI, np.int32) if pred else None
        self.part = _guarded(3 * n_part, SENT64, np.uint64, guard=6)
        self.sums = _guarded(3, SENT64, np.uint64, guard=3)

    def ptrs(self):
        return (self.nll[1] if self.nll else None, self.pred[1] if self.pred else None, self.part[1])

    def reduce(self, kh):
        kh.call("kh_score_reduce", _stream(), self.part[1], self.n_part, self.sums[1])
        torch.cuda.synchronize()

    def raw(self):
        return [host(t[0], t[2].dtype) for t in (self.nll, self.pred, self.part, self.sums) if t is not None]


def _check_score(out, lg, tgt, C, rows_per_part, tag, family):
    """everything a scoring launch + wn_score_reduce returns, against float64 of the exact logits `lg`"""
    M = lg.shape[0]
    nll64, valid, pred64 = _nll64(lg, tgt, C)
    hits = valid & (pred64 == tgt)
    g_pred = host(out.pred[0], np.int32)
    e_pred = out.pred[2].copy(); e_pred[16:16 + M] = pred64
    assert np.array_equal(g_pred, e_pred), "%s: row_pred differs from the first argmax on rows %s (or a guard is hit)" % (tag, np.nonzero(g_pred != e_pred)[0][:8] - 16)
    g_nll = host(out.nll[0], np.uint32)
    assert (g_nll[:16] == SENT32).all() and (g_nll[16 + M:] == SENT32).all(), tag + ": row_nll guards"
    rows = g_nll[16:16 + M]
    assert (rows[~valid] == NAN32).all(), tag + ": an invalid target's row_nll is not the quiet NaN 0x7fc00000"
    nll = rows.view(np.float32).astype(np.float64)
    finite = np.isfinite(lg).all(axis=1)
    L = float(np.abs(lg[finite]).max()) if finite.any() else 1.0
    bound = _nll_bound(L)
    err = np.abs(nll[valid] - nll64[valid])
    if err.size:
        _worst(family, err.max())
        print("%s: worst |row_nll - float64| %.3g, bound %.3g" % (tag, err.max(), bound))
        assert err.max() <= bound, "%s: row_nll off by %.3g (bound %.3g)" % (tag, err.max(), bound)
    g_part = host(out.part[0], np.uint64)
    assert (g_part[:6] == SENT64).all() and (g_part[6 + 3 * out.n_part:] == SENT64).all(), tag + ": `part` does not hold exactly n_part triples"
    part = g_part[6:6 + 3 * out.n_part].view(np.float64).reshape(-1, 3)
    for w in range(out.n_part):
        sl = slice(w * rows_per_part, min(M, (w + 1) * rows_per_part))
        v = nll[sl][valid[sl]]
        assert part[w, 1] == hits[sl].sum() and part[w, 2] == valid[sl].sum(), "%s: counts of partial %d" % (tag, w)
        assert abs(part[w, 0] - math.fsum(v)) <= len(v) * 2.0 ** -53 * np.abs(v).sum(), "%s: nll sum of partial %d" % (tag, w)
    g_sums = host(out.sums[0], np.uint64)
    assert (g_sums[:3] == SENT64).all() and (g_sums[6:] == SENT64).all(), tag + ": sums guards"
    sums = g_sums[3:6].view(np.float64)
    assert sums[1] == hits.sum() and sums[2] == valid.sum(), "%s: sums[1:] %s, want %d hits of %d valid rows" % (tag, sums[1:], hits.sum(), valid.sum())
    v = nll[valid]
    assert abs(sums[0] - math.fsum(v)) <= max(len(v), 1) * 2.0 ** -53 * np.abs(v).sum(), "%s: sums[0] %r, the returned rows add up to %r" % (tag, sums[0], math.fsum(v))
    return g_pred[16:16 + M], sums


def _head_launch(kh, bf16, dat, S, E, M, tgt_d, out):
    skip = np.full((M + 3, S), NAN32, np.uint32)   # (rows past M: never read)
    skip[:M] = dat["skip"].view(np.uint32)
    keep = [dev(skip), dev(dat["b1"]), dev(dat["b2"])]
    if bf16:
        w1, w2 = dev(bits16(np.ascontiguousarray(dat["W1"].T))), dev(bits16(np.ascontiguousarray(dat["W2"].T)))   # [E][S], [256][E]
        wargs = (None, None, w1.data_ptr(), w2.data_ptr())
    else:
        w1, w2 = dev(dat["W1"]), dev(dat["W2"])   # B^T: [S][E], [E][256]
        wargs = (w1.data_ptr(), w2.data_ptr(), None, None)
    kh.call("kh_score_head", _stream(), int(bf16), keep[0].data_ptr(), M, S, E, *wargs, keep[1].data_ptr(), keep[2].data_ptr(), tgt_d.data_ptr(), *out.ptrs())
    out.reduce(kh)
    del keep, w1, w2


@pytest.mark.parametrize("M", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("S,E", [(32, 64), (96, 192), (32, 192), (96, 64)], ids=["S32-E64", "S96-E192", "S32-E192", "S96-E64"])
@pytest.mark.parametrize("form", ["f32", "bf16"])
def test_score_head(kh, form, S, E, M):
    """fp32: 2 / 6 K pieces of 16, one / three chunks of 64 end channels; bf16 (operands all bf16 numbers): a single K piece of 32 / an odd count"""
    dat = _head_data(S, E, M, seed=S + E + M)
    tgt = _targets(dat["logits"], np.random.RandomState(M), 256)
    tgt_d = dev(tgt)
    n_part = (M + 127) // 128
    tag = "score_head %s S %d E %d M %d" % (form, S, E, M)
    outs = []
    for _ in range(2):
        out = _ScoreOut(M, n_part)
        _head_launch(kh, form == "bf16", dat, S, E, M, tgt_d, out)
        outs.append(out.raw())
    _check_score(out, dat["logits"], tgt, 256, 128, tag, "score row_nll")
    for a, b in zip(*outs):
        assert np.array_equal(a, b), tag + ": a second launch gives other bits"


@pytest.mark.parametrize("form", ["f32", "bf16"])
def test_score_head_null_outputs(kh, form):
    """row_nll == NULL / row_pred == NULL: the other outputs and the partials keep their bits"""
    S, E, M = 96, 192, 129
    dat = _head_data(S, E, M, seed=3)
    tgt = _targets(dat["logits"], np.random.RandomState(4), 256)
    tgt_d = dev(tgt)
    full = _ScoreOut(M, 2)
    _head_launch(kh, form == "bf16", dat, S, E, M, tgt_d, full)
    _check_score(full, dat["logits"], tgt, 256, 128, "score_head %s (both outputs)" % form, "score row_nll")
    f_nll, f_pred, f_part, f_sums = full.raw()
    no_nll = _ScoreOut(M, 2, nll=False)
    _head_launch(kh, form == "bf16", dat, S, E, M, tgt_d, no_nll)
    g_pred, g_part, g_sums = no_nll.raw()
    assert np.array_equal(g_pred, f_pred) and np.array_equal(g_part, f_part) and np.array_equal(g_sums, f_sums), "row_nll == NULL changes the other outputs"
    no_pred = _ScoreOut(M, 2, pred=False)
    _head_launch(kh, form == "bf16", dat, S, E, M, tgt_d, no_pred)
    g_nll, g_part, g_sums = no_pred.raw()
    assert np.array_equal(g_nll, f_nll) and np.array_equal(g_part, f_part) and np.array_equal(g_sums, f_sums), "row_pred == NULL changes the other outputs"


def test_score_head_bf16_rounding(kh):
    """h is rounded to bf16, to nearest even, where it becomes the second product's operand: integer h in 256 .. 1023 on ties (even and odd last bit), just
    below and just above them; logits = rne16(h) . W2 + b2 with W2 = +-1/64 (exact).  What shows of the logits: the argmax of every row, logits[target] and the
    logsumexp through row_nll -- the data must tell RNE from truncation and from no rounding by 1000 x the bound on some row (asserted first)."""
    rs = np.random.RandomState(17)
    S, E, M = 96, 64, 300
    skip = rs.randint(-255, 256, (M, S)).astype(np.float64)
    W1 = np.zeros((S, E))
    for e in range(E):
        W1[rs.choice(S, 3, replace=False), e] = (1, 1, 2)
    b1 = rs.randint(-2, 3, E).astype(np.float64)
    W2 = np.zeros((E, 256))
    for c in range(256):
        a, b = rs.choice(E, 2, replace=False)
        W2[a, c], W2[b, c] = 1 / 64, -1 / 64
    b2 = rs.randint(-64, 65, 256) / 64
    h = np.maximum(np.maximum(skip, 0) @ W1 + b1, 0)
    assert h.max() < 1024 and np.array_equal(h, np.rint(h))
    hi = h[(h >= 512)].astype(np.int64)
    lo = h[(h >= 256) & (h < 512)].astype(np.int64)
    for r8 in range(8):   # ulp 4: residues 1, 2 (tie), 3 after an even and after an odd bf16 number
        assert (hi % 8 == r8).any()
    assert (lo % 4 == 1).any() and (lo % 4 == 3).any()   # ulp 2: ties to the even and to the odd side
    h32 = h.astype(np.float32)
    forms = {"rne": rne16(h32).astype(np.float64), "trunc": (h32.view(np.uint32) & 0xFFFF0000).view(np.float32).astype(np.float64), "none": h}
    lg = {k: v @ W2 + b2 for k, v in forms.items()}
    assert np.array_equal(lg["rne"].astype(np.float32).astype(np.float64), lg["rne"]) and np.abs(lg["rne"]).max() <= 32, "case leaves the exact range"
    tgt = _targets(lg["rne"], rs, 256)
    want = _nll64(lg["rne"], tgt, 256)
    for other in ("trunc", "none"):
        o = _nll64(lg[other], tgt, 256)
        v = want[1]
        assert np.abs(o[0][v] - want[0][v]).max() >= 1000 * _nll_bound(32) and (o[2] != want[2]).any(), "the case does not tell RNE from '%s'" % other
    dat = dict(skip=skip.astype(np.float32), W1=W1.astype(np.float32), W2=W2.astype(np.float32), b1=b1.astype(np.float32), b2=b2.astype(np.float32))
    out = _ScoreOut(M, 3)
    _head_launch(kh, True, dat, S, E, M, dev(tgt), out)
    _check_score(out, lg["rne"], tgt, 256, 128, "score_head bf16 rounding of h", "score row_nll")


def _rows_logits(M, C, rs):
    """integer logits in -32 .. 32 with planted ties by row kind (lanes of wn_score_rows: class c is lane c % 64) and one row with -inf classes"""
    lg = rs.randint(-32, 29, (M, C)).astype(np.float64)
    pairs = {3: (10, 11), 4: (5, 69), 5: (63, 64), 6: (0, C - 1)}   # two lanes, two classes of a lane, lane 63 | 0, first | last
    for m in range(M):
        k = m % 8
        if k in pairs and pairs[k][1] < C:
            lg[m, list(pairs[k])] = lg[m].max() + 1
        elif k == 7:
            lg[m] = lg[m, 0]
    if M >= 8:
        r = 2
        lg[r, [0, 1, 3, C - 1]] = -np.inf       # the first classes, the last one ...
        lg[r, 7::64] = -np.inf                  # ... and every class of lane 7
    return lg


@pytest.mark.parametrize("M", [1, 31, 32, 33, 300])
@pytest.mark.parametrize("C", [256, 128, 100, 40], ids=["C256", "C128", "C100", "C40"])
def test_score_rows(kh, C, M):
    """any class count: lanes with a ragged class count (C = 100) and with no class at all (C = 40); C = 256: the head kernel on operands with the
    same logits must return the same row_pred and counts"""
    rs = np.random.RandomState(C + M)
    dat = _head_data(32, 64, M, seed=C + M) if C == 256 else None
    lg = dat["logits"].copy() if dat else _rows_logits(M, C, rs)
    if dat and M >= 8:
        lg2 = _rows_logits(M, C, rs)   # (the head's logits cannot hold -inf: a second launch on the planted rows)
    n_part = (M + 31) // 32
    tag = "score_rows C %d M %d" % (C, M)

    def targets(lgx):
        tg = _targets(lgx, rs, C)
        if np.isinf(lgx).any():
            tg[2] = 2   # (the row with -inf classes aims at a finite one: a finite row_nll is expected)
        return tg

    tgt = targets(lg)

    def run(lgx, tg):
        buf = np.full((M + 2, C), NAN32, np.uint32)   # (rows past M: never read)
        buf[:M] = lgx.astype(np.float32).view(np.uint32)
        ld, td = dev(buf), dev(tg)
        outs = []
        for _ in range(2):
            out = _ScoreOut(M, n_part)
            kh.call("kh_score_rows", _stream(), ld.data_ptr(), C, td.data_ptr(), M, *out.ptrs())
            out.reduce(kh)
            outs.append(out.raw())
        for a, b in zip(*outs):
            assert np.array_equal(a, b), tag + ": a second launch gives other bits"
        return _check_score(out, lgx, tg, C, 32, tag, "score row_nll")

    pred, sums = run(lg, tgt)
    if dat:
        out = _ScoreOut(M, (M + 127) // 128)
        _head_launch(kh, False, dat, 32, 64, M, dev(tgt), out)
        h_pred, h_sums = _check_score(out, lg, tgt, 256, 128, tag + " (wn_score_head)", "score row_nll")
        assert np.array_equal(pred, h_pred) and np.array_equal(sums[1:], h_sums[1:]), tag + ": wn_score_rows and wn_score_head disagree on the same logits"
        if M >= 8:
            run(lg2, targets(lg2))


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3000])
def test_score_reduce(kh, n):
    """partials whose sum is exact in fp64 in any order (multiples of 2^-10 below 2^30): bit equality with the float64 sum"""
    rs = np.random.RandomState(n)
    part = rs.randint(-2 ** 40, 2 ** 40, (n, 3)).astype(np.float64) / 1024
    exact = np.array([math.fsum(part[:, k]) for k in range(3)])
    assert np.abs(part).sum(axis=0).max() < 2 ** 43   # (in units of 2^-10: every partial sum of a column is an integer below 2^53)
    buf = np.full(3 * n + 12, np.nan)   # (behind the n triples: never read)
    buf[:3 * n] = part.ravel()
    pd = dev(buf)
    sums = _guarded(3, SENT64, np.uint64, guard=3)
    kh.call("kh_score_reduce", _stream(), pd.data_ptr(), n, sums[1])
    torch.cuda.synchronize()
    want = sums[2].copy(); want[3:6] = exact.view(np.uint64)
    assert_bits(host(sums[0], np.uint64), want, "score_reduce n %d" % n)


# ================================================================ c. the small kernels (bit exact)
@pytest.mark.parametrize("P,ns,R", [(1, 1, 32), (2, 3, 96), (1, 3, 96), (2, 1, 32)])
@pytest.mark.parametrize("n_kind", ["below", "equal", "above"])
@pytest.mark.parametrize("ML", [3, 5, 25])
def test_fill_ring(kh, ML, n_kind, P, ns, R):
    """the newest count = min(ML, n_time) rows of every stream go to slot t mod ML of all P copies; the other slots keep the sentinel"""
    n_time = {"below": ML - 1, "equal": ML, "above": 2 * ML + 2}[n_kind]
    count = min(ML, n_time)
    rs = np.random.RandomState(ML + n_time + R)
    T = n_time + 3
    X = rs.standard_normal((ns, T, R)).astype(np.float32)
    xh = np.full((ns, T, R), NAN32, np.uint32)
    xh[:, n_time - count:n_time] = X[:, n_time - count:n_time].view(np.uint32)   # (older rows and the rows behind n_time: never read)
    xd = dev(xh)
    ring = _guarded(P * ns * ML * R, SENT32, np.uint32, guard=64)
    kh.call("kh_fill_ring", _stream(), xd.data_ptr(), T * R, ring[1], R, ML, ns, P, n_time, count)
    torch.cuda.synchronize()
    want = ring[2].copy()
    w = want[64:-64].reshape(P, ns, ML, R)
    for t in range(n_time - count, n_time):
        w[:, :, t % ML] = X[:, t].view(np.uint32)[None]
    assert_bits(host(ring[0], np.uint32), want, "fill_ring ML %d n_time %d P %d streams %d R %d" % (ML, n_time, P, ns, R))


@pytest.mark.parametrize("shadow", [False, True], ids=["x", "x+xh"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("R", [32, 96])
@pytest.mark.parametrize("rows", [1, 63, 65])
def test_fwd_start(kh, rows, R, bias, shadow):
    """x[row] = start_conv column idx[row] (+ bias); the bf16 shadow is the RNE of that sum"""
    rs = np.random.RandomState(rows + R)
    bj = rs.randint(0, 8, R).astype(np.float64) if bias else np.zeros(R)
    start, final = _start_values((256, R), bj, rs)
    bvec = (bj / 128).astype(np.float32)
    assert np.array_equal(start + bvec, final)
    idx = rs.randint(0, 256, rows).astype(np.int32)
    idx[0] = 255
    idx[-1] = 0 if rows > 1 else 255
    ih = np.full(rows + 8, 7, np.int32)   # (behind the rows: a valid class, never read)
    ih[:rows] = idx
    i_d, s_d, b_d = dev(ih), dev(start), dev(bvec)
    x = _guarded(rows * R, SENT32, np.uint32, guard=64)
    xh = _guarded(rows * R, SENT16, np.uint16, guard=64) if shadow else None
    kh.call("kh_fwd_start", _stream(), i_d.data_ptr(), s_d.data_ptr(), b_d.data_ptr() if bias else None, x[1], rows, R, xh[1] if shadow else None)
    torch.cuda.synchronize()
    v = final[idx]
    want = x[2].copy(); want[64:-64] = v.view(np.uint32).ravel()
    assert_bits(host(x[0], np.uint32), want, "fwd_start x")
    if shadow:
        assert not np.array_equal(bits16(rne16(v)), bits16((v.view(np.uint32) & 0xFFFF0000).view(np.float32))), "the case does not tell rounding from truncation"
        want = xh[2].copy(); want[64:-64] = bits16(rne16(v)).ravel()
        assert_bits(host(xh[0], np.uint16), want, "fwd_start bf16 shadow")


@pytest.mark.parametrize("n", [1, 2, 511, 512, 513])
def test_cvt_bf16(kh, n):
    """two elements per thread, the odd tail alone, (n / 2 + 256) / 256 workgroups"""
    v = _rounding_points((n,), np.random.RandomState(n))
    ih = np.full(n + 5, NAN32, np.uint32)
    ih[:n] = v.view(np.uint32)
    i_d = dev(ih)
    out = _guarded(n, SENT16, np.uint16, guard=16)
    kh.call("kh_cvt_bf16", _stream(), i_d.data_ptr(), out[1], n)
    torch.cuda.synchronize()
    want = out[2].copy(); want[16:16 + n] = bits16(rne16(v))
    assert_bits(host(out[0], np.uint16), want, "cvt_bf16 n %d" % n)


@pytest.mark.parametrize("rows,cols", [(32, 32), (33, 31), (96, 40), (1, 70)])
@pytest.mark.parametrize("form", ["cvt", "f32"])
def test_transposes(kh, form, rows, cols):
    """out[b][c][r] = in[b][r][c] (cvt: rounded to bf16), two batches in_batch_stride > rows x cols apart with NaN between them"""
    rs = np.random.RandomState(rows + cols)
    nb, stride = 2, rows * cols + 24
    v = _rounding_points((nb, rows, cols), rs) if form == "cvt" else rs.standard_normal((nb, rows, cols)).astype(np.float32)
    ih = np.full(nb * stride, NAN32, np.uint32)
    for b in range(nb):
        ih[b * stride:b * stride + rows * cols] = v[b].view(np.uint32).ravel()
    i_d = dev(ih)
    vt = np.ascontiguousarray(v.transpose(0, 2, 1))
    if form == "cvt":
        out = _guarded(nb * rows * cols, SENT16, np.uint16, guard=64)
        kh.call("kh_cvt_bf16_transposed", _stream(), i_d.data_ptr(), stride, out[1], rows, cols, nb)
        want = out[2].copy(); want[64:-64] = bits16(rne16(vt)).ravel()
        dt = np.uint16
    else:
        out = _guarded(nb * rows * cols, SENT32, np.uint32, guard=64)
        kh.call("kh_transpose_batched", _stream(), i_d.data_ptr(), stride, out[1], rows, cols, nb)
        want = out[2].copy(); want[64:-64] = vt.view(np.uint32).ravel()
        dt = np.uint32
    torch.cuda.synchronize()
    assert_bits(host(out[0], dt), want, "%s transpose %d x %d" % (form, rows, cols))

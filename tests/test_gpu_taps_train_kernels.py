"""-m gpu: the input-gradient product of the kernel_size 3 / 4 training step, one launch at a time through its own launcher
(tests/kernels/wn_kernel_harness.hip includes csrc/wn_runtime.hip: wn_launch_taps_bwd -> wn_bwd_gemm_taps<3>, <4>):

    dx(i) = cin(i) [i >= cin_skip_lo]  +  sum_j a(i - sh + (k-1-j) d) . B_j      for the output rows i of every batch entry,

`a` = [dF|dG], rows_dfg rows of 2D floats per entry (a row outside [0, rows_dfg) reads as zero and must not be loaded), B_j = the transposed tap block
[2D][N], tap 0 the oldest.  Method of tests/test_gpu_kernels.py: EXACT operands -- integers / 64 in [-16, 16] / 64, so that every product is a multiple
of 2^-12 and every partial sum of the at most 4 * 192 = 768 terms (and the addend) stays below 2^6: representable whatever the order -- and BIT EQUALITY
with a float64 evaluation; the output between sentinel NaN guards that must come back untouched; NaN in every operand row a mask hides: the rows in front
of and behind every entry's [dF|dG] (as far as the farthest view reaches, so that a wrong mask shows as a NaN result, never as a stray read), the rows of
the addend before cin_skip_lo, the gaps between the tap blocks of B.  The data of every case can tell a dropped, a reversed or a row-shifted view.

Cases: for k = 3 and 4 a pairwise cover of M in {127, 129, 383} x rows_per_batch in {43, 50, 97} (clip boundaries inside a tile) x d in {1, 2, 7, rows + 3}
(the last leaves only the shift-0 view alive) x N = R in {32, 96, 160} (narrower than, and across, the 128-column tile) x 2D in {64, 192} x the addend
(absent, cin_skip_lo = 0, cin_skip_lo = (k-1) d); single-row clips; and the product as the training step's own helper describes it (wn_layer_dx_taps).
sh = (k-1) d, the training step's value, where that leaves an entry rows of [dF|dG] -- both ends of the window are then in play --, else 0."""
import numpy as np
import pytest
import torch

from kernel_lib import NOMAP, SENT32, Rows, _pairwise, _stream, assert_bits, dev, nan_rows
from kernel_lib import kh  # noqa: F401  (the session fixture)

pytestmark = pytest.mark.gpu
NAN32 = np.uint32(0x7FC00000)


@pytest.fixture(scope="module")
def kt(kh):
    return kh.dll


def _operands(rs, shape):
    return rs.randint(-16, 17, shape).astype(np.float32) / 64


def _dx64(A64, W64, cin64, taps, M, rpb, sh, d, rows_dfg, cin_lo, shift=None, drop=None, order=None):
    """float64 value of the product; shift / drop / order: the wrong products the data must be able to tell (view j read `shift` rows off / zeroed / the
    tap blocks in another order)"""
    m = np.arange(M)
    q, rem = m // rpb, m % rpb
    out = np.zeros((M, W64.shape[2]))
    alive = []
    for j in range(taps):
        tj = rem - sh + (taps - 1 - j) * d
        ok = (tj >= 0) & (tj < rows_dfg)
        alive.append(bool(ok.any()))
        if drop == j:
            continue
        src = tj + (shift[1] if shift is not None and shift[0] == j else 0)
        v = np.where(ok[:, None], A64[q, np.clip(src, 0, rows_dfg - 1)], 0.0)
        out += v @ W64[order[j] if order else j]
    if cin64 is not None:
        out += np.where((rem >= cin_lo)[:, None], cin64, 0.0)
    return out, alive


def _case(kt, taps, M, rpb, d, N, two_d, cin, seed):
    rs = np.random.RandomState(seed)
    k1 = taps - 1
    sh = k1 * d if k1 * d < rpb else 0
    rows_dfg = rpb - sh
    cin_lo = {"none": 0, "lo0": 0, "lokd": k1 * d}[cin]
    nb = (M + rpb - 1) // rpb
    # [dF|dG]: `pre` NaN rows in front of every entry's rows, `post` behind them: wherever a view could reach if its mask were wrong
    pre, post, ld = sh + 2, k1 * d + 2, two_d + 8
    T = pre + rows_dfg + post
    A = _operands(rs, (nb, rows_dfg, two_d))
    ah = np.full((nb, T, ld), NAN32, np.uint32)
    ah[:, pre:pre + rows_dfg, :two_d] = A.view(np.uint32)
    W = _operands(rs, (taps, two_d, N))                      # B_j = W[j]: [2D][N]
    stride = two_d * N + 64                                  # a NaN gap between the tap blocks
    bh = np.full(taps * stride, NAN32, np.uint32)
    for j in range(taps):
        bh[j * stride:j * stride + two_d * N] = W[j].reshape(-1).view(np.uint32)
    C = _operands(rs, (M, N)) if cin != "none" else None
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    C64 = None if C is None else C.astype(np.float64)
    ref, alive = _dx64(A64, W64, C64, taps, M, rpb, sh, d, rows_dfg, cin_lo)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), "the case is not exact in fp32"
    # the data can tell the wrong products (views that are alive somewhere)
    live = [j for j in range(taps) if alive[j]]
    for j in live:
        assert not np.array_equal(_dx64(A64, W64, C64, taps, M, rpb, sh, d, rows_dfg, cin_lo, drop=j)[0], ref), "view %d dropped goes unseen" % j
        if rows_dfg > 1:
            for s in (-1, 1):
                assert not np.array_equal(_dx64(A64, W64, C64, taps, M, rpb, sh, d, rows_dfg, cin_lo, shift=(j, s))[0], ref), "view %d shifted goes unseen" % j
    if len(live) > 1:
        assert not np.array_equal(_dx64(A64, W64, C64, taps, M, rpb, sh, d, rows_dfg, cin_lo, order=list(range(taps))[::-1])[0], ref)
    ad, bd = dev(ah), dev(bh)
    amap = (ad.data_ptr() + 4 * pre * ld, T * ld, ld, -sh)
    cin_r = nan_rows(M, rpb, N, C, lo=min(cin_lo, rpb)) if C is not None else None
    c = Rows(M, rpb, N, t0=5, gap=7).upload()
    tag = "taps %d M %d rpb %d d %d N %d 2D %d cin %s sh %d" % (taps, M, rpb, d, N, two_d, cin, sh)
    rc = kt.kt_bwd_taps(_stream(), taps, *amap, d, 0, rows_dfg, two_d, bd.data_ptr(), stride, N, *(cin_r.map() if cin_r else NOMAP), cin_lo, *c.map(), M, rpb)
    torch.cuda.synchronize()
    assert rc == 0, tag
    assert_bits(c.got(), c.expect(ref.astype(np.float32)), tag)


SHAPE_M = [127, 129, 383]
SHAPE_RPB = [43, 50, 97]
DIST = [1, 2, 7, "big"]
WIDTH = [32, 96, 160]
TWO_D = [64, 192]
CIN = ["none", "lo0", "lokd"]


def _cases(taps):
    out = []
    for mi, ri, di, ni, ki, ci in _pairwise([len(SHAPE_M), len(SHAPE_RPB), len(DIST), len(WIDTH), len(TWO_D), len(CIN)], seed=10 + taps):
        rpb = SHAPE_RPB[ri]
        d = rpb + 3 if DIST[di] == "big" else DIST[di]
        cid = "k%d-M%d-rpb%d-d%s-N%d-K%d-%s" % (taps, SHAPE_M[mi], rpb, DIST[di], WIDTH[ni], TWO_D[ki], CIN[ci])
        out.append(pytest.param(taps, SHAPE_M[mi], rpb, d, WIDTH[ni], TWO_D[ki], CIN[ci], id=cid))
    return out


@pytest.mark.parametrize("taps,M,rpb,d,N,two_d,cin", _cases(3) + _cases(4))
def test_bwd_taps(kt, taps, M, rpb, d, N, two_d, cin):
    _case(kt, taps, M, rpb, d, N, two_d, cin, seed=1000 * taps + M + rpb + d + N + two_d)


@pytest.mark.parametrize("cin", ["none", "lo0"])
@pytest.mark.parametrize("taps", [3, 4], ids=["k3", "k4"])
def test_bwd_taps_single_row_clips(kt, taps, cin):
    """rows_per_batch = 1: every row is a clip of its own, only the shift-0 view exists, 129 entries in two row tiles"""
    _case(kt, taps, 129, 1, 2, 96, 64, cin, seed=77 + taps)


@pytest.mark.parametrize("taps,with_dxin", [(3, True), (4, True), (4, False)], ids=["k3", "k4", "k4-last-layer"])
def test_layer_dx_as_the_training_step_describes_it(kt, taps, with_dxin):
    """wn_layer_dx_taps: dense [dF|dG] on the rows_dfg trailing rows of clips of L rows, dx and dx' on the rows_out = rows_dfg + (k-1) d trailing rows
    of x-shaped matrices [n][L][R]; the rows of dx in front of them stay untouched, the rows of dx' in front of [dF|dG]'s hold NaN."""
    rs = np.random.RandomState(5 + taps)
    R, D, n, L, d, rows_dfg = 96, 32, 3, 61, 5, 37
    rows_out = rows_dfg + (taps - 1) * d
    A, W = _operands(rs, (n, rows_dfg, 2 * D)), _operands(rs, (taps, 2 * D, R))
    C = _operands(rs, (n * rows_out, R))
    ref, _ = _dx64(A.astype(np.float64), W.astype(np.float64), C.astype(np.float64) if with_dxin else None, taps, n * rows_out, rows_out,
                   rows_out - rows_dfg, d, rows_dfg, rows_out - rows_dfg)
    cin = np.full((n, L, R), NAN32, np.uint32)
    cv = C.reshape(n, rows_out, R).copy()
    cv[:, :rows_out - rows_dfg] = np.nan
    cin[:, L - rows_out:] = cv.view(np.uint32)
    out = np.full((n + 2, L, R), SENT32, np.uint32)   # (a guard clip on either side)
    ad, bd, cd, od = dev(A), dev(W), dev(cin), dev(out)
    rc = kt.kt_layer_dx(_stream(), taps, R, D, ad.data_ptr(), rows_dfg, rows_out, d, bd.data_ptr(), 2 * D * R, cd.data_ptr() if with_dxin else None,
                        od.data_ptr() + 4 * L * R, L, n)
    torch.cuda.synchronize()
    assert rc == 0
    exp = out.copy()
    exp[1:-1, L - rows_out:] = ref.astype(np.float32).reshape(n, rows_out, R).view(np.uint32)
    assert_bits(od.cpu().numpy().view(np.uint32), exp, "wn_layer_dx_taps k=%d" % taps)

"""-m gpu: the bf16 filter/gate product of kernel_size 3 / 4, one launch at a time through its own launcher (tests/kernels/wn_kernel_harness.hip
includes csrc/wn_runtime.hip: wn_launch_taps_bf16 -> wn_fwd_gemm_taps_bf16<3 | 4, 4 | 8>):

    z = gate([x(t - (k-1) d) | ... | x(t - d) | x(t)] . B^T + b),   x fp32 rounded to bf16 (RNE) while staged, B bf16 [N][k*R], fp32 accumulation,

in the manner of the taps cases of tests/test_gpu_infer_kernels.py: a float64 reference, z and its copy c2 between sentinel NaN guards that must come
back untouched, NaN in every row of x that a mask hides or that no tap of the case may read (a wrong mask shows as a NaN result), and that module's bar
GATE_ABS.  For k = 3 and 4 a pairwise cover of R in {64, 128} (2 and 4 chunks of 32 per view) x N = 2D in {128, 256 -- the 128 x 256 tile --, 384} x
M in {1, 127, 129, 259} rows in entries of 37 (ragged row tiles, tiles that span entries) x d in {1, 2, 37, 40 -- beyond the entry} x t0 - (k-1) d
(equal to t_min; above it; below it, so that the oldest views of an entry's first rows read as zero) x bias; c2 on the last rows of an entry only.

Two operand sets per case:
  exact     x = integers / 64 in [-16, 16] / 64, weights +-2^-e (e = 2 .. 5) or 0: bf16 numbers whose products and partial sums (< 2^3, multiples of
            2^-11) are exact in fp32 in any order, so the pre-activations are exact and z sits within GATE_ABS of float64.
  rounding  x = fp32 values that are NOT bf16 numbers -- below, on (exact ties such as 1 + 2^-8 and 1 + 3 * 2^-8, scaled by 2^-3: even and odd last
            bit) and above the rounding points --, against float64 on the RNE-rounded operands.  Bar: GATE_ABS + K * 2^-23 * max Sum|a b| (fp32
            accumulation of K terms in whatever grouping the matrix core uses: each partial sum is within 2^-24 of its value relative to Sum|a b|, at
            most K roundings, doubled for slack; the gate's slope is at most 1).  The data must move z by more than 1000 GATE_ABS under truncation.
In both sets the data must tell a reversed, a row-shifted and a zeroed view by more than 1000 GATE_ABS in every 128-row tile where that view is read."""
import numpy as np
import pytest
import torch

from kernel_lib import GATE_ABS, Rows, _gate64, _pairwise, _stream, assert_bits, bits16, dev, rne16
from kernel_lib import kh  # noqa: F401  (the session fixture)

pytestmark = pytest.mark.gpu
NAN32 = np.uint32(0x7FC00000)
RPB = 37

KB_R = [64, 128]
KB_N = [128, 256, 384]
KB_M = [1, 127, 129, 259]
KB_D = [1, 2, 37, 40]
KB_TMIN = ["eq", "above", "below"]   # t0 - (k-1) d, the oldest tap of an entry's first row, against t_min


@pytest.fixture(scope="module")
def kb(kh):
    return kh.dll


def _case_data(taps, M, R, N, d, tmin, bias, mode, seed):
    """Host side of a case (no GPU): the operands, the image of x with its NaN rows, the float64 reference and the assertions on the data."""
    rs = np.random.RandomState(seed)
    rpb, k1 = RPB, taps - 1
    reach = k1 * d
    t0 = reach + 2                      # two rows of slack below the oldest tap of an entry's first row
    # above: t_min lies below the oldest tap of an entry's first row (nothing is masked; the rows in between hold NaN and are not read).  below: the first
    # d + 1 rows of that history do not exist -- view 0 reads as zero on the rows rem <= d (all of them where d is beyond the entry), view 1 on row 0
    t_min = {"eq": t0 - reach, "above": t0 - reach - 2, "below": t0 - reach + d + 1}[tmin]
    K = taps * R
    nb = (M + rpb - 1) // rpb
    pre = 2
    T, ld = pre + t0 + rpb + 3, R + 8
    tau = np.arange(T) - pre
    if mode == "exact":
        Xf = rs.randint(-16, 17, (nb, T, R)).astype(np.float32) / 64
    else:
        b = rs.randint(128, 256, (nb, T, R)).astype(np.float64)
        f = rs.choice([0.5 - 2.0 ** -16, 0.5, 0.5 + 2.0 ** -16, 0.25, 0.75], (nb, T, R))
        Xf = (rs.choice([-1.0, 1.0], (nb, T, R)) * (b + f) / 1024).astype(np.float32)
        Xf[:, :, 0] = (1 + 2.0 ** -8) / 8      # exact ties: the even neighbour is below ...
        Xf[:, :, 1] = (1 + 3 * 2.0 ** -8) / 8  # ... and above
        assert not np.array_equal(rne16(Xf), Xf) and (rne16(Xf[:, :, 0]) == 0.125).all() and (rne16(Xf[:, :, 1]) == (1 + 2.0 ** -6) / 8).all()
    W = (rs.choice([-1.0, 1.0], (N, K)) * 2.0 ** -rs.randint(2, 6, (N, K)) * (rs.rand(N, K) < 0.9)).astype(np.float32)
    assert np.array_equal(rne16(W), W)
    bvec = rs.randint(-8, 9, N).astype(np.float64) / 64 if bias else np.zeros(N)
    m = np.arange(M)
    q, rem = m // rpb, m % rpb
    first_read = max(t_min, t0 - reach)
    xh = np.full((nb, T, ld), NAN32, np.uint32)
    for e in range(nb):
        n_e = min(rpb, M - e * rpb)
        ok = (tau >= first_read) & (tau < t0 + n_e)
        xh[e, ok, :R] = Xf[e, ok].view(np.uint32)
    X64 = rne16(Xf).astype(np.float64)          # (exact: the values themselves)
    Xt64 = (Xf.view(np.uint32) & 0xFFFF0000).view(np.float32).astype(np.float64)
    W64 = W.astype(np.float64)

    def view(j, shift=0, src=X64):   # view j (0 = the oldest tap) of every row; `shift` moves the rows it reads, not the rows that exist
        tj = t0 + rem - (k1 - j) * d
        v = src[q, np.clip(pre + tj + shift, 0, T - 1)]
        return np.where((tj >= t_min)[:, None], v, 0.0)

    alive = [t0 + rem - (k1 - j) * d >= t_min for j in range(taps)]

    def z_of(views):
        acc = sum(views[j] @ W64[:, j * R:(j + 1) * R].T for j in range(taps))
        return _gate64(acc + bvec, N)[0]

    views = [view(j) for j in range(taps)]
    z = z_of(views)
    # sensitivity of the data (a condition on the inputs): a wrong product moves z by >= 1000 GATE_ABS in every 128-row tile where it can differ at all
    wrong = {}
    for j in range(taps):
        wrong["view %d zeroed" % j] = (views[:j] + [np.zeros_like(views[j])] + views[j + 1:], alive[j])
        for s in (-1, 1):
            wrong["view %d shifted %+d" % (j, s)] = (views[:j] + [view(j, s)] + views[j + 1:], alive[j])
    wrong["views reversed"] = (views[::-1], np.any([alive[j] | alive[k1 - j] for j in range(taps // 2)], axis=0))
    if mode == "rounding":
        wrong["operands truncated"] = ([view(j, src=Xt64) for j in range(taps)], np.any(alive, axis=0))
    for name, (vs, can) in wrong.items():
        dz = np.abs(z_of(vs) - z).max(axis=1)
        for r0 in range(0, M, 128):
            if can[r0:r0 + 128].any():
                assert dz[r0:r0 + 128].max() >= 1000 * GATE_ABS, "the data cannot tell '%s' in the tile at row %d (seed %d)" % (name, r0, seed)
    A = np.concatenate(views, axis=1)
    sum_abs = (np.abs(A) @ np.abs(W64).T).max()
    bar = GATE_ABS + (K * 2.0 ** -23 * sum_abs if mode == "rounding" else 0.0)
    return dict(xh=xh, pre=pre, T=T, ld=ld, t0=t0, t_min=t_min, W=W, bvec=bvec, z=z, bar=bar, q=q, rem=rem, nb=nb, K=K)


def _seed(taps, M, R, N, d, tmin, mode):
    return 100000 * taps + 1000 * KB_TMIN.index(tmin) + 7 * M + R + N + 13 * d + (50000 if mode == "rounding" else 0)


def _cases():
    out = []
    for taps in (3, 4):
        for ri, ni, mi, di, ti, bi in _pairwise([len(KB_R), len(KB_N), len(KB_M), len(KB_D), len(KB_TMIN), 2], seed=40 + taps):
            cid = "k%d-R%d-N%d-M%d-d%d-%s-b%d" % (taps, KB_R[ri], KB_N[ni], KB_M[mi], KB_D[di], KB_TMIN[ti], bi)
            out.append(pytest.param(taps, KB_M[mi], KB_R[ri], KB_N[ni], KB_D[di], KB_TMIN[ti], bool(bi), id=cid))
    return out


@pytest.mark.parametrize("mode", ["exact", "rounding"])
@pytest.mark.parametrize("taps,M,R,N,d,tmin,bias", _cases())
def test_taps_bf16(kb, taps, M, R, N, d, tmin, bias, mode):
    rpb = RPB
    c2_first = rpb - 3   # (the skip rows: the last rows of an entry only)
    D = _case_data(taps, M, R, N, d, tmin, bias, mode, _seed(taps, M, R, N, d, tmin, mode))
    q, rem, z = D["q"], D["rem"], D["z"]
    xd = dev(D["xh"])
    xmap = (xd.data_ptr() + 4 * D["pre"] * D["ld"], D["T"] * D["ld"], D["ld"], D["t0"])
    guard = 64
    bnh = np.full(N * D["K"] + 2 * guard, 0x7FC0, np.uint16)   # (NaN around the bank: a read past a row or the bank shows in the result)
    bnh[guard:-guard] = bits16(D["W"]).ravel()
    bn = dev(bnh)
    b_d = dev(D["bvec"].astype(np.float32)) if bias else None
    c = Rows(M, rpb, N // 2, t0=5, gap=7).upload()
    nrow2 = rpb - c2_first
    c2r = Rows(D["nb"] * nrow2, nrow2, N // 2, t0=2, gap=3).upload()
    tag = "taps %d M %d R %d N %d d %d t_min %s (%s)" % (taps, M, R, N, d, tmin, mode)
    rc = kb.kb_taps_bf16(_stream(), taps, *xmap, d, D["t_min"], R, bn.data_ptr() + 2 * guard, N, b_d.data_ptr() if bias else None, *c.map(), M, rpb,
                         *c2r.map(), c2_first)
    assert rc == 0, tag + ": launch error %d" % rc
    torch.cuda.synchronize()
    got = c.got()
    qq, tt = c.rows()
    vals = got[qq, tt, :N // 2]
    err = np.abs(vals.view(np.float32).astype(np.float64) - z)
    print("%s: max |z - z64| = %.3g (bar %.3g)" % (tag, np.nanmax(err), D["bar"]))
    assert not np.isnan(vals.view(np.float32)).any(), tag + ": NaN in z (a hidden row was read)"
    assert (err <= D["bar"]).all(), tag + ": %d element(s) beyond the bar %.3g, worst %.3g" % ((err > D["bar"]).sum(), D["bar"], err.max())
    e = c.h.copy()
    e[qq, tt, :N // 2] = vals
    assert_bits(got, e, tag + " z guards")
    on = rem >= c2_first
    got2 = c2r.got()
    ev = c2r.h.copy()
    q2, t2 = q[on], c2r.t0 + rem[on] - c2_first
    assert np.array_equal(got2[q2, t2, :N // 2], vals[on]), tag + ": c2 is not the copy of z on the skip rows"
    ev[q2, t2, :N // 2] = vals[on]
    assert_bits(got2, ev, tag + " c2 guards")

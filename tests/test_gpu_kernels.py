"""The training step's matrix-core kernels one at a time, through the product's own launchers (tests/kernels/wn_kernel_harness.hip includes
csrc/wn_runtime.hip), against float64 references at the shapes where tiles, splits and row windows have edges.

Three families of checks:
  * exact -- integer or dyadic operands whose every product and partial sum stays below 2^24 (and is a bf16 number where bf16 is staged):
    every summation order is exact, so the kernel must equal the float64 result BIT FOR BIT (np.array_equal of the raw bits, guard bands
    included).  Catches lost / doubled / shifted rows or columns, wrong windows, wrong batch mapping, lost splits, a wrong transpose,
    accumulation below fp32, and -- with outputs that need more than 8 bits -- any rounding to bf16 other than round-to-nearest-even.
  * rounding -- fp32 operands just below, on (ties, even and odd last bit) and just above the bf16 rounding points of values that keep the
    product exact: the kernel must equal the exact product of the RNE-rounded operands.
  * bounded -- the nonlinear epilogues (gate, cross-entropy, sums of non-integers) against float64 under a bound derived from the code's own
    arithmetic; the worst observed error of each family is printed at the end of the module.
Every output lives inside a buffer of sentinel NaNs (rows before t0, gaps between batch entries, columns past N) that must come back untouched;
every input row a kernel must not read (guards, row windows) holds NaN.

Branch table: each hipLaunchKernelGGL line of the launchers -> the cases (test ids) that take it.
  wn_launch_nn     wn_fwd_gemm_bf16<GATE, 8, true>          test_nn[bf16w-gate-a16-*]
                   wn_fwd_gemm_bf16<GATE, 8>                test_nn[bf16w-gate-*], test_gate_nonlinearity[bf16w]
                   wn_fwd_gemm_bf16<PLAIN, 8, true>         test_nn[bf16w-plain-a16-*]
                   wn_fwd_gemm_bf16<PLAIN, 8>               test_nn[bf16w-plain-*], test_bf16_rounding_nn[wide]
                   wn_fwd_gemm_bf16<GATE, 4>                test_nn[bf16-gate-*], test_gate_nonlinearity[bf16]
                   wn_fwd_gemm_bf16<GATE_BWD, 4>            test_nn[bf16-gatebwd-*], test_bwd_layer_pair (unfused form)
                   wn_fwd_gemm_bf16<PLAIN, 4, true>         test_nn[bf16-plain-a16-*], test_fused_layer (unfused form)
                   wn_fwd_gemm_bf16<PLAIN, 4>               test_nn[bf16-plain-*], test_bf16_rounding_nn[narrow]
                   wn_fwd_gemm<GATE>                        test_nn[f32-gate-*], test_gate_nonlinearity[f32]
                   wn_fwd_gemm<GATE_BWD>                    test_nn[f32-gatebwd-*]
                   wn_fwd_gemm<PLAIN>                       test_nn[f32-plain-*]
  wn_launch_layer  wn_fwd_layer_bf16                        test_fused_layer
  wn_launch_bwd_layer  wn_bwd_layer_bf16                    test_bwd_layer_pair
  wn_launch_tn     wn_bwd_wfg_bf16 (+ wn_tn_reduce)         test_tn_tall[wfg-*], test_tn_tall[tallskip-*], test_tn_window_2gb[wfg]
                   wn_bwd_gemm_tn_bf16<8, true, true>       test_tn[wide16-*], test_tn[notall-*]
                   wn_bwd_gemm_tn_bf16<8, false, true>      test_tn[wideb16-*]
                   wn_bwd_gemm_tn_bf16<8, false, false>     test_tn[wide32-*], test_bf16_rounding_tn
                   wn_bwd_gemm_tn_bf16<4, false, true>      test_tn[b16-*]
                   wn_bwd_gemm_tn_bf16<4, true, false>      test_tn[a16-*]
                   wn_bwd_gemm_tn_bf16<4, false, false>     test_tn[bf16-*]
                   wn_bwd_gemm_tn (+ wn_tn_reduce)          test_tn[f32-*], test_tn[idx-*], test_tn[relu-*], test_tn_window_2gb[f32]
  wn_launch_colsum wn_bwd_colsum<true> / <false>, wn_tn_reduce   test_colsum (N % 4 != 0: the atomics path in both modes)
  direct           wn_tn_reduce                             test_tn_reduce;  wn_bwd_gate<*>: test_gate_bwd;  wn_xent_rows/_reduce: test_xent
(The inference kernels -- wn_launch_taps, the score kernels, ring fill, the small layout kernels: tests/test_gpu_infer_kernels.py, with a table of its own.)
"""
import os

import numpy as np
import pytest
import torch

from kernel_lib import NOMAP, SENT16, SENT32, Rows, _bounded, _check_gate_out, _rounding_points, _stream, _worst, assert_bits, bits16, dev, from16, host, nan_rows, rne16
from kernel_lib import kh  # noqa: F401  (the session fixture)

pytestmark = pytest.mark.gpu

PLAIN, GATE, GATE_BWD = 0, 1, 2


# ---------------------------------------------------------------- NN products (wn_launch_nn)
def _nn_case(kh, form, epi, M, rpb, N, K, k_split=None, a16=False, lo=(0, 0), hi=(0, 0), bias=False, cin=False, cin_lo=0, relu_a=False,
             relu_c=False, mask=False, c_h=False, c_bf16=False, gates=False, packed=False, c2_first=None, sep_b1=False, seed=0):
    rs = np.random.RandomState(seed)
    bf16 = form != "f32"
    k_split = K if k_split is None else k_split
    if epi == GATE:   # dyadic operands: F, G exact, the nonlinearity is what is bounded
        A = rs.randint(-16, 17, (M, K)).astype(np.float32) / 64
        B = rs.randint(-16, 17, (N, K)).astype(np.float32) / 64
    else:
        A = rs.randint(-4, 5, (M, K)).astype(np.float32)
        B = rs.randint(-4, 5, (N, K)).astype(np.float32)
    rem = np.arange(M) % rpb
    # the two views of A: columns < k_split from view 0, the rest from view 1, each behind its own window
    v0 = (rem >= lo[0]) & (rem < rpb - hi[0])
    v1 = (rem >= lo[1]) & (rem < rpb - hi[1])
    Aeff = A.astype(np.float64).copy()
    Aeff[~v0, :k_split] = 0
    Aeff[~v1, k_split:] = 0
    if relu_a:
        Aeff = np.maximum(Aeff, 0)
    a0 = nan_rows(M, rpb, k_split, A[:, :k_split], bf16=a16, lo=lo[0], hi=hi[0], t0=2)
    a1 = nan_rows(M, rpb, K - k_split, A[:, k_split:], bf16=a16, lo=lo[1], hi=hi[1], t0=4) if K > k_split else None
    a1map = a1.map() if a1 else a0.map()
    acc = Aeff @ B.astype(np.float64).T   # [M][N]
    keep = []
    bt = bt1 = bn = bn1 = None
    ldb = 0
    if bf16:
        if sep_b1:   # two banks with a row length of their own
            ldb = K + 32
            b0 = np.full((N, ldb), 0x7FC0, np.uint16); b0[:, :k_split] = bits16(B[:, :k_split])
            b1 = np.full((N, ldb), 0x7FC0, np.uint16); b1[:, :K - k_split] = bits16(B[:, k_split:])
            bn, bn1 = dev(b0), dev(b1)
            keep += [bn, bn1]
        else:
            bn = dev(bits16(B)); keep.append(bn)
    else:
        if sep_b1:
            bt, bt1 = dev(np.ascontiguousarray(B[:, :k_split].T)), dev(np.ascontiguousarray(B[:, k_split:].T))
            keep += [bt, bt1]
        else:
            bt = dev(np.ascontiguousarray(B.T)); keep.append(bt)
    nout = N // 2 if epi == GATE else (2 * N if epi == GATE_BWD else N)
    b_d = None
    bvec = np.zeros(N, np.float64)
    if bias:
        bvec = rs.randint(-8, 9, N).astype(np.float64) / (64 if epi == GATE else 1)
        b_d = dev(bvec.astype(np.float32)); keep.append(b_d)
    out16 = c_bf16 and bf16
    c = Rows(M, rpb, nout, bf16=out16 and epi != GATE_BWD or (epi == GATE_BWD and out16), t0=5, gap=7).upload()
    cin_r, cinv = None, np.zeros((M, N))
    if cin:
        cv = rs.randint(-64, 65, (M, N)).astype(np.float32)
        cin_r = nan_rows(M, rpb, N, cv, lo=cin_lo, t0=1)
        cinv = cv.astype(np.float64); cinv[rem < cin_lo] = 0
    mask_r = None
    mv = np.ones((M, N))
    if mask:   # shares c's row layout
        mv = rs.randint(-1, 2, (M, N)).astype(np.float32)
        mask_r = Rows(M, rpb, N, t0=5, gap=7)
        mask_r.h[...] = np.float32(1).view(np.uint32)
        mask_r.put(mv).upload()
    ch_r = Rows(M, rpb, N, bf16=True, t0=5, gap=7).upload() if c_h else None
    if c_h:   # c_h shares c's layout: make it the same shape
        assert ch_r.T == c.T and ch_r.ld == c.ld
    gt = gg = None
    c2r = None
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    if epi == GATE:
        if gates:
            if packed:
                gt = dev(np.full((M, N // 2), SENT32, np.uint32))
            else:
                gt = dev(np.full((M, N // 2), SENT32, np.uint32)); gg = dev(np.full((M, N // 2), SENT32, np.uint32))
        if c2_first is not None:
            nrow2 = rpb - c2_first
            c2r = Rows(((M - 1) // rpb + 1) * nrow2, nrow2, N // 2, bf16=out16, t0=2, gap=3).upload()
    if epi == GATE_BWD:
        tq = rs.randint(-7, 8, (M, N)).astype(np.float32) / 8
        sq = rs.randint(1, 8, (M, N)).astype(np.float32) / 8
        if packed:
            gt = dev(((bits16(sq).astype(np.uint32) << 16) | bits16(tq).astype(np.uint32)))
        else:
            gt, gg = dev(tq), dev(sq)
        if c2_first is not None:
            nrow2 = rpb - c2_first
            nb = (M - 1) // rpb + 1
            c2v = rs.randint(-64, 65, (nb * nrow2, N)).astype(np.float32)
            c2r = nan_rows(nb * nrow2, nrow2, N, c2v, bf16=out16, t0=2)
    kh.call("kh_nn", _stream(), epi, *a0.map(), *a1map, k_split, K, ptr(bt), ptr(bt1), N, ptr(b_d),
            *(cin_r.map() if cin_r else NOMAP), *c.map(), M, rpb, int(relu_a), int(relu_c), ptr(mask_r.d) if mask_r else None,
            ptr(gt), ptr(gg), *(c2r.map() if c2r else NOMAP), c2_first or 0, int(packed), lo[0], lo[1], hi[0], hi[1], cin_lo,
            int(a16), int(c_bf16), ptr(ch_r.d) if ch_r else None, ptr(bn), ptr(bn1), ldb)
    torch.cuda.synchronize()
    tag = "%s epi %d M %d rpb %d N %d K %d" % (form, epi, M, rpb, N, K)
    if epi == PLAIN:
        v = acc + bvec + cinv
        if relu_c:
            v = np.maximum(v, 0)
        v = np.where(mv > 0, v, 0)
        v32 = v.astype(np.float32)
        assert np.array_equal(v32.astype(np.float64), v), "case leaves the exact range"
        assert_bits(c.got(), c.expect(rne16(v32) if c.bf16 else v32), tag + " c")
        if ch_r:
            assert_bits(ch_r.got(), ch_r.expect(rne16(v32)), tag + " c_h")
    elif epi == GATE_BWD:
        dz = acc.copy()
        if c2r is not None:
            nrow2 = rpb - c2_first
            on = rem >= c2_first
            idx = (np.arange(M) // rpb) * nrow2 + rem - c2_first
            c2v64 = c2v.astype(np.float64)
            dz[on] += c2v64[idx[on]]
        t64, s64 = tq.astype(np.float64), sq.astype(np.float64)
        df, dg = dz * s64 * (1 - t64 * t64), dz * t64 * s64 * (1 - s64)
        out = np.empty((M, 2 * N))
        for j in range(N // 32):
            out[:, 64 * j:64 * j + 32] = df[:, 32 * j:32 * j + 32]
            out[:, 64 * j + 32:64 * j + 64] = dg[:, 32 * j:32 * j + 32]
        o32 = out.astype(np.float32)
        assert np.array_equal(o32.astype(np.float64), out), "case leaves the exact range"
        assert_bits(c.got(), c.expect(rne16(o32) if c.bf16 else o32), tag + " [dF|dG]")
    else:
        v = acc + bvec
        F = np.concatenate([v[:, 64 * j:64 * j + 32] for j in range(N // 64)], axis=1)
        G = np.concatenate([v[:, 64 * j + 32:64 * j + 64] for j in range(N // 64)], axis=1)
        th, sg = np.tanh(F), 1 / (1 + np.exp(-G))
        z = th * sg
        _check_gate_out(c, z, tag + " z", c.bf16)
        if c2r is not None:
            on = rem >= c2_first
            ev = c2r.h.copy()
            nrow2 = rpb - c2_first
            got = c2r.got()
            q = np.arange(M) // rpb
            qq, tt = q[on], c2r.t0 + rem[on] - c2_first
            gotv = got[qq, tt, :N // 2]
            ref = c.got()[q[on], c.t0 + rem[on], :N // 2]
            assert np.array_equal(gotv, ref), tag + " c2 is not the copy of z on the skip rows"
            ev[qq, tt, :N // 2] = ref
            assert_bits(got, ev, tag + " c2 guards")
        if gt is not None:
            if packed:
                g = host(gt, np.uint32)
                gth, gsg = from16(g & 0xFFFF), from16(g >> 16)
                _bounded("gate tanh (bf16)", gth, th, 2.0 ** -8)
                _bounded("gate sigmoid (bf16)", gsg, sg, 2.0 ** -8)
            else:
                _bounded("gate tanh", host(gt, np.float32), th, 0)
                _bounded("gate sigmoid", host(gg, np.float32), sg, 0)
    del keep


NN_FORMS = [   # (id, form, epi, a16)
    ("f32-plain", "f32", PLAIN, False), ("f32-gate", "f32", GATE, False), ("f32-gatebwd", "f32", GATE_BWD, False),
    ("bf16-plain", "bf16", PLAIN, False), ("bf16-gate", "bf16", GATE, False), ("bf16-gatebwd", "bf16", GATE_BWD, False),
    ("bf16-plain-a16", "bf16", PLAIN, True),
    ("bf16w-plain", "bf16", PLAIN, False), ("bf16w-plain-a16", "bf16", PLAIN, True),
    ("bf16w-gate", "bf16", GATE, False), ("bf16w-gate-a16", "bf16", GATE, True),
]
NN_SHAPES = [   # (M, rows_per_batch): around the 128-row tiles, rows_per_batch not dividing 128
    (1, 1), (31, 40), (127, 50), (128, 100), (129, 129), (383, 97), (4097, 300)]


def _nn_n(fid, i):
    """N for the form: the wide forms need N % 256 == 0, the narrow bf16 ones N % 256 != 0 (else the launcher takes the wide tile)"""
    if fid.startswith("bf16w"):
        return (256, 512)[i % 2]
    if fid.startswith("bf16") and "gatebwd" not in fid:
        return (32, 96, 128, 160)[i % 4] if "gate" not in fid else (64, 128, 192)[i % 3]
    return (32, 96, 128, 160, 256)[i % 5] if "gate" not in fid or "gatebwd" in fid else (64, 128, 256)[i % 3]


@pytest.mark.parametrize("fid,form,epi,a16", NN_FORMS, ids=[f[0] for f in NN_FORMS])
@pytest.mark.parametrize("si", range(len(NN_SHAPES)), ids=["M%d" % s[0] for s in NN_SHAPES])
def test_nn(kh, fid, form, epi, a16, si):
    M, rpb = NN_SHAPES[si]
    N = _nn_n(fid, si)
    K = (64, 128, 256)[si % 3]
    ks = K // 2 if si % 2 else K
    lo = (min(rpb - 1, 37), 0) if si % 3 == 1 else (0, 0)
    hi = (0, min(rpb - 1, 45)) if si % 3 == 2 and ks < K else (0, 0)
    opts = dict(k_split=ks, a16=a16, lo=lo, hi=hi, seed=si, sep_b1=si % 2 == 1)
    if epi == PLAIN:
        opts.update(bias=True, cin=si % 2 == 0, cin_lo=min(rpb - 1, 33) if si % 4 == 0 else 0, relu_a=(si % 3 == 0 and not a16),
                    relu_c=si % 3 == 1, mask=(si % 3 == 2 and not (form != "f32" and si % 2)), c_h=si % 2 == 1, c_bf16=(form != "f32" and si % 4 == 3))
        if opts["c_bf16"]:
            opts["mask"] = False; opts["c_h"] = False
    elif epi == GATE:
        opts.update(bias=si % 2 == 0, gates=True, packed=si % 2 == 1 or form != "f32", c_bf16=form != "f32" and si % 3 != 0,
                    c2_first=(rpb // 3 if rpb > 1 else None))
    else:
        opts.update(packed=si % 2 == 0, c_bf16=form != "f32", c2_first=(rpb // 2 if si % 3 else None))
    _nn_case(kh, form, epi, M, rpb, N, K, **opts)


@pytest.mark.parametrize("form", ["f32", "bf16", "bf16w"])
def test_gate_nonlinearity(kh, form):
    """A = 0: the pre-activations are the bias, swept over the regimes of tanh / sigmoid (and NaN, which must stay NaN)"""
    N = 256 if form == "bf16w" else 128
    sweep = np.array([0, 1e-6, -1e-6, 1, -1, 9, -9, 44, -44, 89, -89, 1e4, -1e4, np.inf, -np.inf, np.nan], np.float32)
    bvec = np.resize(sweep, N).astype(np.float32)
    bvec[32:64] = np.roll(bvec[32:64], 5)
    M, rpb, K = 40, 40, 64
    a0 = nan_rows(M, rpb, K, np.zeros((M, K), np.float32))
    c = Rows(M, rpb, N // 2).upload()
    b_d = dev(bvec)
    bt = dev(np.zeros((K, N), np.float32)) if form == "f32" else None
    bn = dev(np.zeros((N, K), np.uint16)) if form != "f32" else None
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    kh.call("kh_nn", _stream(), GATE, *a0.map(), *a0.map(), K, K, ptr(bt), None, N, b_d.data_ptr(), *NOMAP, *c.map(), M, rpb, 0, 0, None,
            None, None, *NOMAP, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, ptr(bn), None, 0)
    torch.cuda.synchronize()
    F = np.concatenate([bvec[64 * j:64 * j + 32] for j in range(N // 64)]).astype(np.float64)
    G = np.concatenate([bvec[64 * j + 32:64 * j + 64] for j in range(N // 64)]).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        z = np.tanh(F) / (1 + np.exp(-G))
    z = np.broadcast_to(z, (M, N // 2))
    got = c.got()[c.rows()[0], c.rows()[1], :N // 2].view(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(z)), "NaN where the reference has none, or a NaN lost: %s" % got[0]
    _check_gate_out(c, z, "gate sweep", False)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_bf16_rounding_nn(kh, wide):
    """the fp32-stored A of the bf16 products is rounded to nearest even on its way to LDS"""
    rs = np.random.RandomState(5)
    M, rpb, K, N = 200, 70, 64, 256 if wide else 128
    A = _rounding_points((M, K), rs)
    B = rs.randint(-4, 5, (N, K)).astype(np.float32)
    exact = rne16(A).astype(np.float64) @ B.T.astype(np.float64)
    a0 = nan_rows(M, rpb, K, A)
    c = Rows(M, rpb, N).upload()
    bn = dev(bits16(B))
    kh.call("kh_nn", _stream(), PLAIN, *a0.map(), *a0.map(), K, K, None, None, N, None, *NOMAP, *c.map(), M, rpb, 0, 0, None,
            None, None, *NOMAP, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, bn.data_ptr(), None, 0)
    torch.cuda.synchronize()
    e32 = exact.astype(np.float32)
    assert np.array_equal(e32.astype(np.float64), exact)
    assert_bits(c.got(), c.expect(e32), "bf16 rounding of A")
    trunc = (A.view(np.uint32) & 0xFFFF0000).view(np.float32).astype(np.float64) @ B.T.astype(np.float64)
    assert not np.array_equal(trunc, exact), "the case does not tell rounding from truncation"


# ---------------------------------------------------------------- weight-gradient products (wn_launch_tn)
TN_KINDS = {   # id -> (bf16 step, Ka, Nb, a_bf16, b_bf16, ka_split, extra): the launcher's dispatch picks the kernel named in the branch table
    "f32": (0, 96, 160, 0, 0, 0, dict(a_skip_lo=5)),
    "relu": (0, 128, 64, 0, 0, 0, dict(relu_a=1)),
    "idx": (0, 256, 64, 0, 0, 0, dict(a_idx=True)),
    "bf16": (1, 160, 96, 0, 0, 0, dict(relu_a=1, a_skip_lo=3)),
    "a16": (1, 128, 128, 1, 0, 0, dict(a_skip_lo=9)),
    "b16": (1, 96, 192, 0, 1, 0, dict(c_trans=1)),
    "wide32": (1, 128, 256, 0, 0, 0, dict(a_skip_lo=2)),
    "wideb16": (1, 256, 512, 0, 1, 0, dict(c_trans=1)),
    "wide16": (1, 128, 256, 1, 1, 0, dict(a_skip_lo=4)),
    "wfg": (1, 256, 256, 1, 1, 128, dict(a_skip_lo=11)),
    "notall": (1, 256, 256, 1, 1, 128, dict(a_skip_lo=6, env={"WN_NO_TALL_WFG": "1"})),
    "tallskip": (1, 512, 256, 1, 1, 0, dict(c_trans=1, env={"WN_TALL_SKIP": "1"})),
}
# (id, M, rows_per_batch, splits): M < 32, splits starting inside batch entries with gaps, counts that are not multiples of 8, last splits of 1 / 31 rows
TN_SPLITS = [("m20", 20, 7, 1), ("s2", 700, 130, 2), ("s7", 1900, 333, 7), ("s8last1", 1793, 250, 8), ("s8last31", 1823, 131, 8), ("s16", 3841, 97, 16)]
TALL_SPLITS = [("m20", 20, 7, 1), ("s2last31", 63, 10, 2), ("s7last1", 193, 50, 7), ("s8last31", 255, 40, 8), ("s16", 481, 33, 16), ("s7", 1900, 333, 7)]


def _tn_env(kind, Ka, Nb, splits, env):
    """force the split count through the launcher's own A/B switches (honoured with WN_TESTING=1)"""
    e = dict(env)
    e["WN_TN_WANT"] = str(splits * ((Ka + 127) // 128) * ((Nb + 127) // 128))
    e["WN_TN_WANT_WIDE"] = str(splits * ((Ka + 127) // 128) * ((Nb + 255) // 256))
    e["WN_TALL_WANT"] = str(splits * max(1, Ka // 256) * max(1, Nb // 256))
    return e


class _Env:
    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _tn_run(kh, kind, M, rpb, splits, seed=0, scale=1.0):
    bf16, Ka, Nb, a16, b16, ka_split, extra = TN_KINDS[kind]
    extra = dict(extra)
    env = extra.pop("env", {})
    rs = np.random.RandomState(seed)
    rem = np.arange(M) % rpb
    lo = extra.get("a_skip_lo", 0)
    relu = extra.get("relu_a", 0)
    c_trans = extra.get("c_trans", 0)
    B = rs.randint(-4, 5, (M, Nb)).astype(np.float32)
    b = nan_rows(M, rpb, Nb, B, bf16=bool(b16), t0=3)
    idx_d = None
    if extra.get("a_idx"):
        cls = rs.randint(0, 256, M).astype(np.int32)
        cls[:2] = (0, 255); cls[-1] = 255
        Aeff = np.zeros((M, Ka)); Aeff[np.arange(M), cls] = 1
        T = 2 + rpb + 4
        ih = np.full(((M + rpb - 1) // rpb, T), 5, np.int32)   # (guards: a valid class -- a wrong read adds to its column)
        ih[np.arange(M) // rpb, 2 + rem] = cls
        idx_d = dev(ih)
        amap, a1map = (None, T, 1, 2), NOMAP
    else:
        A = rs.randint(-4, 5, (M, Ka)).astype(np.float32)
        Aeff = A.astype(np.float64)
        first = ka_split if ka_split else Ka
        Aeff[rem < lo, :first] = 0
        if relu:
            Aeff = np.maximum(Aeff, 0)
        a = nan_rows(M, rpb, first, A[:, :first], bf16=bool(a16), lo=lo, t0=4)
        amap = a.map()
        a1 = nan_rows(M, rpb, Ka - first, A[:, first:], bf16=bool(a16), t0=1) if ka_split else None
        a1map = a1.map() if a1 else NOMAP
    exact = Aeff.T @ B.astype(np.float64)   # [Ka][Nb]
    if c_trans:
        exact = exact.T
    rows_c, cols_c = exact.shape
    ldc = cols_c + 8
    c0 = (rs.randint(-1000, 1001, (rows_c, ldc)) * scale).astype(np.float32)   # C is NOT zero on entry: the product adds to it
    full = np.full((rows_c + 2, ldc), SENT32, np.uint32)
    full[1:-1] = c0.view(np.uint32)
    full[1:-1, cols_c:] = SENT32
    want = full.copy()
    w = (c0[:, :cols_c].astype(np.float64) + exact).astype(np.float32)
    assert np.array_equal(w.astype(np.float64), c0[:, :cols_c].astype(np.float64) + exact), "case leaves the exact range"
    want[1:-1, :cols_c] = w.view(np.uint32)
    outs = []
    with _Env(_tn_env(kind, Ka, Nb, splits, env)):
        for det in (0, 1, 1):
            c = dev(full)
            kh.call("kh_tn", _stream(), det, bf16, *amap, None if idx_d is None else idx_d.data_ptr(), *b.map(), Ka, Nb, c.data_ptr() + 4 * ldc,
                    ldc, M, rpb, relu, *a1map, ka_split, a16, b16, c_trans, lo)
            torch.cuda.synchronize()
            outs.append(host(c, np.uint32))
    tag = "%s M %d rpb %d splits %d" % (kind, M, rpb, splits)
    assert_bits(outs[0], want, tag + " atomics")
    assert_bits(outs[1], want, tag + " deterministic")
    assert np.array_equal(outs[1], outs[2]), tag + ": two deterministic runs differ"


@pytest.mark.parametrize("sp", TN_SPLITS, ids=[s[0] for s in TN_SPLITS])
@pytest.mark.parametrize("kind", [k for k in TN_KINDS if k not in ("wfg", "tallskip")])
def test_tn(kh, kind, sp):
    _, M, rpb, splits = sp
    bf16, Ka, Nb = TN_KINDS[kind][:3]
    if kind != "notall":   # (the plan the launcher takes for this shape: the count the case is named for)
        wide = bf16 and Nb % 256 == 0
        tiles = ((Ka + 127) // 128) * ((Nb + 255) // 256 if wide else (Nb + 127) // 128)
        got = kh.tn_grid(M, Ka, Nb, 256 if wide else 128, splits * tiles)
        assert got[0] == splits, "plan %s for %d splits" % (got, splits)
    _tn_run(kh, kind, M, rpb, splits, seed=M)


@pytest.mark.parametrize("sp", TALL_SPLITS, ids=[s[0] for s in TALL_SPLITS])
@pytest.mark.parametrize("kind", ["wfg", "tallskip"])
def test_tn_tall(kh, kind, sp):
    _, M, rpb, splits = sp
    _tn_run(kh, kind, M, rpb, splits, seed=M + 1)


@pytest.mark.parametrize("kind", ["bf16", "wide32"])
def test_bf16_rounding_tn(kh, kind):
    """both fp32-stored operands of the bf16 weight-gradient products are rounded to nearest even on their way to LDS"""
    bf16, Ka, Nb = TN_KINDS[kind][:3]
    rs = np.random.RandomState(11)
    M, rpb = 100, 37
    A = _rounding_points((M, Ka), rs)
    B = rs.randint(-4, 5, (M, Nb)).astype(np.float32)
    B[::3] = _rounding_points(B[::3].shape, rs) * 128   # (some rows of B off the bf16 grid too: after rounding 9 + 9 bits a product, 100 rows)
    exact = rne16(A).astype(np.float64).T @ rne16(B).astype(np.float64)
    e32 = exact.astype(np.float32)
    assert np.array_equal(e32.astype(np.float64), exact)
    a, b = nan_rows(M, rpb, Ka, A), nan_rows(M, rpb, Nb, B)
    with _Env(_tn_env(kind, Ka, Nb, 2, {})):
        for det in (0, 1):
            c = dev(np.zeros((Ka, Nb), np.float32))
            kh.call("kh_tn", _stream(), det, 1, *a.map(), None, *b.map(), Ka, Nb, c.data_ptr(), Nb, M, rpb, 0, *NOMAP, 0, 0, 0, 0, 0)
            torch.cuda.synchronize()
            assert_bits(host(c, np.uint32), e32.view(np.uint32), "%s rounding det=%d" % (kind, det))


@pytest.mark.parametrize("kind", ["f32", "wfg"])
def test_tn_window_2gb(kh, kind):
    """One split (forced) whose span of A is 2-3 GB: the launcher must split the rows so that every split's buffer descriptor covers them
    (rows past the 2 GB window of a descriptor read as zeros by design -- no fault, a silently wrong gradient)."""
    free, _ = torch.cuda.mem_get_info()
    if free < 4 * 2 ** 30:
        pytest.fail("needs 4 GB of free device memory, %.1f GB free" % (free / 2 ** 30))
    bf16, Ka, Nb, a16, b16, ka_split = TN_KINDS[kind][:6]
    esize = 2 if a16 else 4
    M, rpb = 320, 320
    row_stride = (5 * 2 ** 29) // (M * esize) // 64 * 64   # span of the rows: ~2.5 GB
    big = torch.empty(row_stride * M * esize + 2 ** 20, dtype=torch.uint8, device="cuda")
    rs = np.random.RandomState(3)
    A = rs.randint(-4, 5, (M, Ka)).astype(np.float32)
    B = rs.randint(-4, 5, (M, Nb)).astype(np.float32)
    vals = bits16(A).view(np.uint8) if a16 else A.view(np.uint8)
    rows = torch.from_numpy(vals.reshape(M, -1)).cuda()
    big[: row_stride * M * esize].view(M, row_stride * esize)[:, : Ka * esize].copy_(rows)
    first = ka_split if ka_split else Ka
    amap = (big.data_ptr(), 0, row_stride, 0)
    a1map = (big.data_ptr() + first * esize, 0, row_stride, 0) if ka_split else NOMAP
    b = nan_rows(M, rpb, Nb, B, bf16=bool(b16))
    exact = (A.astype(np.float64).T @ B.astype(np.float64)).astype(np.float32)
    with _Env(_tn_env(kind, Ka, Nb, 1, {})):
        for det in (0, 1):
            c = dev(np.zeros((Ka, Nb), np.float32))
            kh.call("kh_tn", _stream(), det, bf16, *amap, None, *b.map(), Ka, Nb, c.data_ptr(), Nb, M, rpb, 0, *a1map, ka_split, a16, b16, 0, 0)
            torch.cuda.synchronize()
            assert_bits(host(c, np.uint32), exact.view(np.uint32), "%s over a 2.5 GB span det=%d" % (kind, det))
    del big


# ---------------------------------------------------------------- column sums (wn_launch_colsum) and the split reduce
@pytest.mark.parametrize("M", [1, 511, 512, 513, 1537])
@pytest.mark.parametrize("N,x16", [(32, False), (36, False), (256, True), (44, True), (30, False)])
def test_colsum(kh, M, N, x16):
    """out[n] += sum of column n over the rows (gaps between entries); N % 4 != 0 takes the atomics path in both modes"""
    rs = np.random.RandomState(M + N)
    rpb = 200
    X = rs.randint(-64, 65, (M, N)).astype(np.float32)
    x = nan_rows(M, rpb, N, X, bf16=x16)
    o0 = rs.randint(-999, 1000, N + 8).astype(np.float32)
    o0[N:] = np.nan
    want = o0.copy()
    want[:N] = (o0[:N].astype(np.float64) + X.astype(np.float64).sum(0)).astype(np.float32)
    outs = []
    for det in (0, 1, 1):
        o = dev(o0)
        kh.call("kh_colsum", _stream(), det, *x.map(), M, rpb, N, o.data_ptr(), int(x16))
        torch.cuda.synchronize()
        outs.append(host(o, np.uint32))
    for det, got in enumerate(outs[:2]):
        assert_bits(got, want.view(np.uint32), "colsum M %d N %d det=%d" % (M, N, det))
    assert np.array_equal(outs[1], outs[2])
    # non-integers: bounded (fp32 sums of up to 512 rows, then the blocks in order / atomics)
    Xf = rs.standard_normal((M, N)).astype(np.float32)
    if x16:
        Xf = rne16(Xf)
    xf = nan_rows(M, rpb, N, Xf, bf16=x16)
    o = dev(np.zeros(N, np.float32))
    kh.call("kh_colsum", _stream(), 1, *xf.map(), M, rpb, N, o.data_ptr(), int(x16))
    torch.cuda.synchronize()
    ref = Xf.astype(np.float64).sum(0)
    err = np.abs(host(o, np.float32) - ref) / (np.abs(Xf).astype(np.float64).sum(0) + 1e-30)
    _worst("colsum (relative to sum |x|)", err.max())
    assert err.max() <= (512 + 4) * 2.0 ** -24   # (a sequential fp32 sum of 512 terms, then M / 512 <= 4 partial sums)


@pytest.mark.parametrize("c_trans", [0, 1])
def test_tn_reduce(kh, c_trans):
    """wn_tn_reduce adds the splits in order and ADDS the result to C (the atomics of the other mode do the same)"""
    rs = np.random.RandomState(7 + c_trans)
    S, Ka, Nb = 5, 96, 36
    part = rs.randint(-999, 1000, (S, Ka, Nb)).astype(np.float32)
    rows_c, cols_c = (Nb, Ka) if c_trans else (Ka, Nb)
    ldc = cols_c + 4
    c0 = rs.randint(-999, 1000, (rows_c, ldc)).astype(np.float32)
    c0[:, cols_c:] = np.nan
    s = part.astype(np.float64).sum(0)
    want = c0.copy()
    want[:, :cols_c] = (c0[:, :cols_c] + (s.T if c_trans else s)).astype(np.float32)
    p, c = dev(part), dev(c0)
    kh.call("kh_tn_reduce", _stream(), p.data_ptr(), S, Ka, Nb, c.data_ptr(), ldc, c_trans)
    torch.cuda.synchronize()
    assert_bits(host(c, np.uint32), want.view(np.uint32), "tn_reduce c_trans=%d" % c_trans)


# ---------------------------------------------------------------- gate derivative (wn_bwd_gate) and cross-entropy
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("D,M,rows,out_len,with_dz", [(32, 37, 37, 5, True), (64, 171, 57, 19, False), (128, 99, 33, 33, True), (64, 16, 16, 0, True)])
def test_gate_bwd(kh, packed, D, M, rows, out_len, with_dz):
    """[dF|dG] = dz * {s (1 - t^2), t s (1 - s)} in the [F(32) | G(32)] packing, dzg added on the last out_len rows of each entry (ldg > D);
    exact operands (t, s multiples of 1/8, integer dz): bit equality, and the bf16 outputs are RNE of the exact values"""
    rs = np.random.RandomState(D + M)
    dz = rs.randint(-300, 301, (M, D)).astype(np.float32) if with_dz else np.zeros((M, D), np.float32)
    t = rs.randint(-7, 8, (M, D)).astype(np.float32) / 8
    s = rs.randint(1, 8, (M, D)).astype(np.float32) / 8
    nb = M // rows
    ldg = D + 32 if out_len else 0
    dzg = rs.randint(-64, 65, (nb * max(out_len, 1), ldg or D)).astype(np.float32)
    d = dz.astype(np.float64).copy()
    if out_len:
        for m in range(M):
            n, tt = divmod(m, rows)
            if tt >= rows - out_len:
                d[m] += dzg[n * out_len + tt - (rows - out_len), :D]
    df, dg = d * s * (1 - t.astype(np.float64) ** 2), d * t * s * (1 - s.astype(np.float64))
    out = np.empty((M, 2 * D))
    for j in range(D // 32):
        out[:, 64 * j:64 * j + 32], out[:, 64 * j + 32:64 * j + 64] = df[:, 32 * j:32 * j + 32], dg[:, 32 * j:32 * j + 32]
    o32 = out.astype(np.float32)
    assert np.array_equal(o32.astype(np.float64), out)
    if packed:
        th = dev((bits16(s).astype(np.uint32) << 16) | bits16(t).astype(np.uint32))
        sg = None
        dzg_d = dev(bits16(dzg)) if out_len else None
        dfg = dev(np.full(M * 2 * D + 64, SENT16, np.uint16))
    else:
        th, sg = dev(t), dev(s)
        dzg_d = dev(dzg) if out_len else None
        dfg = dev(np.full(M * 2 * D + 64, SENT32, np.uint32))
    dz_d = dev(dz) if with_dz else None
    ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    kh.call("kh_gate_bwd", _stream(), int(packed), ptr(dz_d), th.data_ptr(), ptr(sg), dfg.data_ptr(), M, D, ptr(dzg_d), ldg, rows, out_len)
    torch.cuda.synchronize()
    if packed:
        want = np.full(M * 2 * D + 64, SENT16, np.uint16); want[:M * 2 * D] = bits16(rne16(o32)).ravel()
        assert_bits(host(dfg, np.uint16), want, "gate_bwd packed")
    else:
        want = np.full(M * 2 * D + 64, SENT32, np.uint32); want[:M * 2 * D] = o32.view(np.uint32).ravel()
        assert_bits(host(dfg, np.uint32), want, "gate_bwd")


@pytest.mark.parametrize("M", [1, 3, 4, 5, 1023])
def test_xent(kh, M):
    rs = np.random.RandomState(M)
    x = rs.standard_normal((M, 256)).astype(np.float32) * 3
    tg = rs.randint(0, 256, M).astype(np.int64)
    tg[0] = 255
    if M > 1:
        tg[1] = 0
    for m in range(M):   # the row kinds: one dominant logit, uniform, tied maxima, +-1e4
        k = m % 5
        if k == 1:
            x[m, rs.randint(256)] = 80
        elif k == 2:
            x[m] = 0.25
        elif k == 3:
            x[m, [3, 77, 200]] = x[m].max() + 1
        elif k == 4:
            x[m, rs.randint(256)] = 1e4 if m % 2 else -1e4
    x64 = x.astype(np.float64)
    mx = x64.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(x64 - mx).sum(1))
    rl = lse - x64[np.arange(M), tg]
    p = np.exp(x64 - lse[:, None])
    dl = p.copy(); dl[np.arange(M), tg] -= 1; dl /= M
    xd, td = dev(x), dev(tg)
    losses = []
    for _ in range(2):
        row = torch.empty(M, device="cuda"); dlog = torch.empty(M, 256, device="cuda"); loss = torch.empty(1, device="cuda")
        kh.call("kh_xent", _stream(), xd.data_ptr(), td.data_ptr(), M, row.data_ptr(), dlog.data_ptr(), loss.data_ptr())
        torch.cuda.synchronize()
        losses.append(loss.cpu().numpy().copy())
    # bounds: expf / logf to ~2 ulp on arguments <= 0, a 256-term fp32 sum: |row loss error| <= 4e-7 (|lse| + 1); dlogits to 1e-6 of 1/M
    e_row = np.abs(row.cpu().numpy() - rl) / (np.abs(lse) + np.abs(x64[np.arange(M), tg]) + 1)
    e_dl = np.abs(dlog.cpu().numpy() - dl).max() * M
    _worst("xent row loss (relative)", e_row.max())
    _worst("xent dlogits (x M)", e_dl)
    assert e_row.max() <= 1e-6 and e_dl <= 2e-6
    assert abs(float(losses[0][0]) - rl.mean()) <= 1e-6 * (abs(rl.mean()) + 1)
    assert np.array_equal(losses[0].view(np.uint32), losses[1].view(np.uint32)), "the loss is not bit-reproducible"
    if M >= 3:   # an invalid target: only its own row and the mean are NaN
        tg2 = tg.copy(); tg2[M // 2] = 256
        td2 = dev(tg2)
        kh.call("kh_xent", _stream(), xd.data_ptr(), td2.data_ptr(), M, row.data_ptr(), dlog.data_ptr(), loss.data_ptr())
        torch.cuda.synchronize()
        r = row.cpu().numpy()
        assert np.isnan(r[M // 2]) and not np.isnan(np.delete(r, M // 2)).any() and np.isnan(loss.cpu().numpy()[0])
        assert not np.isnan(dlog.cpu().numpy()).any()


# ---------------------------------------------------------------- the fused layer kernels (wn_launch_layer / wn_launch_bwd_layer)
LAYER_M = [128 * k + e for k in (1, 7, 8, 9, 17) for e in (-1, 1)]


@pytest.mark.parametrize("M", LAYER_M)
def test_fused_layer(kh, M):
    """wn_fwd_layer_bf16 at 128 / 128: z, the packed gates, the copy on the skip rows, x' and its bf16 shadow bit-equal to the two-launch form
    (the same harness, WN_NO_FUSED_LAYER=1), whose products test_nn checks against float64"""
    rs = np.random.RandomState(M)
    R = D = 128
    rpb = 300 if M > 300 else M
    d = 4
    X = rs.randint(-16, 17, (M + d, R)).astype(np.float32) / 64   # (the tap view x(t - d): d rows further up)
    xh = nan_rows(M, rpb, R, X[d:], bf16=True, t0=d + 2)
    q, t = xh.rows()
    xh.h[q, t - d, :R] = bits16(X[:M])   # (rows t0 - d .. of every entry hold x(t - d))
    xh.upload()
    Wfg = rs.randint(-16, 17, (2 * D, 2 * R)).astype(np.float32) / 64
    Wres = rs.randint(-8, 9, (R, D)).astype(np.float32) / 8
    bfg = rs.randint(-8, 9, 2 * D).astype(np.float32) / 64
    bres = rs.randint(-8, 9, R).astype(np.float32)
    xin = nan_rows(M, rpb, R, rs.randint(-64, 65, (M, R)).astype(np.float32), t0=1)
    bn_fg, bn_res = dev(bits16(Wfg)), dev(bits16(Wres))
    bfg_d, bres_d = dev(bfg), dev(bres)
    c2_first = rpb // 2
    outs = {}
    for fused in (True, False):
        z = Rows(M, rpb, D, bf16=True).upload()
        gates = dev(np.full((M, D), SENT32, np.uint32))
        nrow2 = rpb - c2_first
        c2 = Rows(((M - 1) // rpb + 1) * nrow2, nrow2, D, bf16=True).upload()
        x = Rows(M, rpb, R, t0=2).upload()
        x_h = Rows(M, rpb, R, bf16=True, t0=2).upload()
        if fused:
            kh.call("kh_layer", _stream(), *xh.map(-d), *xh.map(), R, 2 * R, bn_fg.data_ptr(), bfg_d.data_ptr(), *z.map(), M, rpb, gates.data_ptr(),
                    *c2.map(), c2_first, 0, 0, bn_res.data_ptr(), bres_d.data_ptr(), *xin.map(), *x.map(), x_h.d.data_ptr())
        else:
            with _Env({"WN_NO_FUSED_LAYER": "1"}):
                assert kh.dll.kh_layer(_stream(), *xh.map(-d), *xh.map(), R, 2 * R, bn_fg.data_ptr(), bfg_d.data_ptr(), *z.map(), M, rpb,
                                       gates.data_ptr(), *c2.map(), c2_first, 0, 0, bn_res.data_ptr(), bres_d.data_ptr(), *xin.map(), *x.map(),
                                       x_h.d.data_ptr()) == -1, "WN_NO_FUSED_LAYER=1 is not honoured"
            kh.call("kh_nn", _stream(), GATE, *xh.map(-d), *xh.map(), R, 2 * R, None, None, 2 * D, bfg_d.data_ptr(), *NOMAP, *z.map(), M, rpb, 0, 0,
                    None, gates.data_ptr(), None, *c2.map(), c2_first, 1, 0, 0, 0, 0, 0, 1, 1, None, bn_fg.data_ptr(), None, 0)
            kh.call("kh_nn", _stream(), PLAIN, *z.map(), *z.map(), D, D, None, None, R, bres_d.data_ptr(), *xin.map(), *x.map(), M, rpb, 0, 0,
                    None, None, None, *NOMAP, 0, 0, 0, 0, 0, 0, 0, 1, 0, x_h.d.data_ptr(), bn_res.data_ptr(), None, 0)
        torch.cuda.synchronize()
        outs[fused] = [z.got(), host(gates, np.uint32), c2.got(), x.got(), x_h.got()]
    for name, f, u in zip(("z", "gates", "c2", "x'", "x' shadow"), outs[True], outs[False]):
        assert np.array_equal(f, u), "fused layer M %d: %s differs from the two-launch form" % (M, name)


@pytest.mark.parametrize("M", LAYER_M)
def test_bwd_layer_pair(kh, M):
    """wn_bwd_layer_bf16: dx (two row-windowed views of a bf16 [dF|dG], banks with a row length of their own, the addend dx') and the layer
    below's [dF|dG] (packed gates, bf16 dzg on the skip rows): exact operands, bit equality with float64 and with the two-launch form"""
    rs = np.random.RandomState(M + 1)
    R = D = 128
    rpb = 300 if M > 300 else M
    d, sh = 3, 2
    P = rs.randint(-4, 5, (M + 8, 2 * D)).astype(np.float32)    # [dF|dG] of layer l (bf16 numbers)
    dfg_r = Rows(M + 8, M + 8, 2 * D, bf16=True, t0=2)
    dfg_r.h[...] = 0x7FC0
    dfg_r.put(P).upload()
    W = rs.randint(-4, 5, (2 * R, 2 * D)).astype(np.float32)      # native [2R][2D]: rows 0..R-1 tap 0, R.. tap 1 -> bn = tap 1, bn1 = tap 0, ldb = 2D
    wbank = dev(bits16(W))
    Wres = rs.randint(-4, 5, (D, R)).astype(np.float32)          # [D][R]: bn_res of the gate-derivative product (N = D, K = R)
    wres_d = dev(bits16(Wres))
    dxn = nan_rows(M, rpb, R, rs.randint(-64, 65, (M, R)).astype(np.float32), t0=1, lo=sh)
    tq = rs.randint(-7, 8, (M, D)).astype(np.float32) / 8
    sq = rs.randint(1, 8, (M, D)).astype(np.float32) / 8
    gates = dev((bits16(sq).astype(np.uint32) << 16) | bits16(tq).astype(np.uint32))
    c2_first = rpb - rpb // 3
    nrow2 = rpb - c2_first
    nb = (M - 1) // rpb + 1
    dzg = nan_rows(nb * nrow2, nrow2, D, rs.randint(-16, 17, (nb * nrow2, D)).astype(np.float32), bf16=True)
    # view 0 = dfg(t) from row rem - sh (valid from rem = sh), view 1 = dfg(t + d) (valid while rem < rpb - d): rows addressed through one entry per batch
    # entry would need the batch layout; use a single batch-strided matrix: entry q starts at row q * rpb of P
    base = dfg_r.d.data_ptr()
    ld = dfg_r.ld
    a0 = (base, rpb * ld, ld, dfg_r.t0 - sh)
    a1 = (base, rpb * ld, ld, dfg_r.t0 + d - sh)
    outs = {}
    for fused in (True, False):
        dx = Rows(M, rpb, R, t0=2).upload()
        dfo = Rows(M, rpb, 2 * D, bf16=True).upload()
        args_a = (*a0, *a1, 2 * D, 4 * D, wbank.data_ptr() + 2 * R * D * 2, wbank.data_ptr(), 2 * D)
        if fused:
            kh.call("kh_bwd_layer", _stream(), *args_a, *dxn.map(), *dx.map(-sh), M, rpb, sh, 0, 0, d, sh, wres_d.data_ptr(), gates.data_ptr(),
                    *dzg.map(), c2_first, *dfo.map())
        else:
            kh.call("kh_nn", _stream(), PLAIN, *a0, *a1, 2 * D, 4 * D, None, None, R, None, *dxn.map(), *dx.map(-sh), M, rpb, 0, 0, None, None, None,
                    *NOMAP, 0, 0, sh, 0, 0, d, sh, 1, 0, None, wbank.data_ptr() + 2 * R * D * 2, wbank.data_ptr(), 2 * D)
            kh.call("kh_nn", _stream(), GATE_BWD, *dx.map(-sh), *dx.map(-sh), R, R, None, None, D, None, *NOMAP, *dfo.map(), M, rpb, 0, 0, None,
                    gates.data_ptr(), None, *dzg.map(), c2_first, 1, 0, 0, 0, 0, 0, 0, 1, None, wres_d.data_ptr(), None, 0)
        torch.cuda.synchronize()
        outs[fused] = [dx.got(), dfo.got()]
    for name, f, u in zip(("dx", "[dF|dG]"), outs[True], outs[False]):
        assert np.array_equal(f, u), "fused backward pair M %d: %s differs from the two-launch form" % (M, name)
    # float64: dx on rows m (entry q, rem): dx'(rem >= sh) + P[q*rpb + rem - sh] . W1^T (rem >= sh) + P[q*rpb + rem + d - sh] . W0^T (rem < rpb - d)
    m = np.arange(M)
    q, rem = m // rpb, m % rpb
    P64 = P.astype(np.float64)
    v0 = np.where((rem >= sh)[:, None], P64[np.clip(q * rpb + rem - sh, 0, None)], 0)
    v1 = np.where((rem < rpb - d)[:, None], P64[q * rpb + rem + d - sh], 0)
    W64 = W.astype(np.float64)
    dxv = v0 @ W64[R:].T + v1 @ W64[:R].T
    cin = dxn.h[q, dxn.t0 + rem, :R].view(np.float32).astype(np.float64)
    dxv += np.where((rem >= sh)[:, None], cin, 0)
    dx32 = dxv.astype(np.float32)
    assert np.array_equal(dx32.astype(np.float64), dxv)
    got_dx = outs[True][0]
    dxr = Rows(M, rpb, R, t0=2)
    dxr.t0 = 2 - sh
    e = dxr.expect(dx32)
    assert_bits(got_dx, e, "fused backward dx")

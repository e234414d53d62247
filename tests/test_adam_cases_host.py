"""CPU: the host restatement of the fused Adam step (tests/adam_cases.py) anchored without touching the code under test --
  * fma32 against libm's fmaf, bit for bit, on inputs built to land on and next to fp32 rounding midpoints
  * adam_reference(addcdiv="cpu") against torch.optim.Adam on CPU tensors, bit for bit, over consecutive steps (both foreach modes)
  * clip_coef / norm32 against torch.nn.utils.clip_grad_norm_ on CPU tensors, bit for bit
  * the families' own conditions: exact sums, coverings, the sizes / offsets / positions they name."""
import ctypes
import ctypes.util

import numpy as np
import pytest
import torch

import adam_cases as ac
from kernel_lib import _pairwise


def _bits_equal(a, b):
    return np.array_equal(ac.bits(a), ac.bits(b))


# ---------------------------------------------------------------- fma32
def _fma_inputs():
    rs = np.random.RandomState(1)
    out = []
    n = 40000
    # (1) a * b is an odd 25-bit integer (a k-bit times a (25 - k)-bit odd factor): an exact fp32 midpoint; c is nothing, or far below one fp64 ulp
    #     of the product (the double sum is inexact: round to odd decides), or a last-place nudge
    k = rs.randint(2, 23, 4 * n)
    A = (rs.randint(0, 1 << 30, 4 * n).astype(np.int64) % (1 << (k - 1)) + (1 << (k - 1))) | 1
    B = (rs.randint(0, 1 << 30, 4 * n).astype(np.int64) % (1 << (24 - k)) + (1 << (24 - k))) | 1
    P = A * B
    mid = (P >= 1 << 24) & (P < 1 << 25)
    A, B, P = A[mid][:n], B[mid][:n], P[mid][:n]
    assert len(A) >= n // 2
    ea, eb = rs.randint(-30, 30, len(A)), rs.randint(-30, 30, len(A))
    a, b = np.ldexp(A.astype(np.float64), ea).astype(np.float32), np.ldexp(B.astype(np.float64), eb).astype(np.float32)
    scale = np.ldexp(P.astype(np.float64), ea + eb)
    for k in (None, 30, 60, 100):
        c = np.zeros(len(a)) if k is None else rs.choice([-1.0, 1.0], len(a)) * np.ldexp(scale, -k)
        out.append((a, b, c.astype(np.float32)))
    # (2) a * b fits 24 bits (12-bit factors); c is half an ulp of it, exactly and one ulp of c to either side, in both signs
    a = rs.randint(1 << 11, 1 << 12, n).astype(np.float32)
    b = rs.randint(1 << 11, 1 << 12, n).astype(np.float32)
    p = (a.astype(np.float64) * b).astype(np.float32)
    half = (np.spacing(p) / 2).astype(np.float32)
    for s in (-1.0, 1.0):
        for c in (half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(np.inf))):
            out.append((a, b, (s * c).astype(np.float32)))
    # (3) anything: wide exponents (overflow, denormal results), cancellation c ~ -a * b, zeros and infinities
    def wide(m):
        return (rs.choice([-1.0, 1.0], m) * np.ldexp(rs.uniform(1, 2, m), rs.randint(-80, 70, m))).astype(np.float32)
    a, b = wide(n), wide(n)
    out.append((a, b, wide(n)))
    with np.errstate(all="ignore"):
        near = -(a.astype(np.float64) * b)
        out.append((a, b, near.astype(np.float32)))
        out.append((a, b, np.nextafter(near.astype(np.float32), np.float32(0))))
    sp = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 2.0 ** -149, 2.0 ** -126, 3.4e38], dtype=np.float32)
    g = np.array(np.meshgrid(sp, sp, sp)).reshape(3, -1)
    out.append((g[0], g[1], g[2]))
    return tuple(np.concatenate([o[i] for o in out]) for i in range(3))


def test_fma32_is_libm_fmaf_bit_for_bit():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    libm.fmaf.restype = ctypes.c_float
    a, b, c = _fma_inputs()
    assert len(a) >= 100000
    want = np.array([libm.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], dtype=np.float32)
    got = ac.fma32(a, b, c)
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(got))
    bad = (ac.bits(got) != ac.bits(want)) & ~nan
    assert bad.sum() == 0, "%d of %d differ, first (a, b, c) = %r" % (bad.sum(), len(a), (a[bad][:1], b[bad][:1], c[bad][:1]))
    # the inputs do what they were built for: a plain fp64 multiply-add, rounded twice, gets some of them wrong
    with np.errstate(all="ignore"):
        twice = (a.astype(np.float64) * b + c).astype(np.float32)
    assert ((ac.bits(twice) != ac.bits(want)) & ~nan).sum() > 1000


# ---------------------------------------------------------------- adam_reference against torch's CPU optimiser
def _torch_cpu_sqrt(x):
    """torch's CPU sqrt of a contiguous tensor goes to a vector math library whose result is within an ulp but not always the correctly rounded
    one (about 0.6 % of these elements differ); the comparison with torch's CPU Adam takes that one operation from torch, so that every OTHER
    rounding of the restatement is held to torch bit for bit.  The square root itself is anchored to IEEE below."""
    return torch.from_numpy(np.ascontiguousarray(x)).sqrt().numpy()


def test_numpy_sqrt_is_the_correctly_rounded_one():
    rs = np.random.RandomState(3)
    v = np.ldexp(rs.uniform(1, 2, 200000), rs.randint(-140, 40, 200000)).astype(np.float32)
    want = np.sqrt(v.astype(np.float64)).astype(np.float32)    # (the fp64 root rounded again is the correctly rounded fp32 root: 53 >= 2 * 24 + 2)
    assert np.array_equal(ac.bits(np.sqrt(v)), ac.bits(want))
    theirs = _torch_cpu_sqrt(v)
    assert (np.abs(ac.bits(theirs).astype(np.int64) - ac.bits(want).astype(np.int64)) <= 1).all()


@pytest.mark.parametrize("foreach", [False, True])
@pytest.mark.parametrize("beta1,wd", [(0.9, 0.0), (0.4, 0.01), (0.5, 0.1), (0.9, 0.01)])
def test_reference_is_torch_cpu_adam_bit_for_bit(beta1, wd, foreach):
    n, steps = 50000, 7
    rs = np.random.RandomState(7)
    hp = dict(lr=1e-3, beta1=beta1, beta2=0.999, eps=1e-8, weight_decay=wd)
    p = (rs.standard_normal(n) * 0.1).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=hp["lr"], betas=(beta1, hp["beta2"]), eps=hp["eps"], weight_decay=wd, foreach=foreach)
    for step in range(1, steps + 1):
        g = (rs.choice([-1.0, 1.0], n) * np.ldexp(rs.uniform(1, 2, n), rs.randint(-20, 2, n))).astype(np.float32)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, _, m, v = ac.adam_reference(p, g, m, v, step=step, addcdiv="cpu", sqrt=_torch_cpu_sqrt, **hp)
        st = opt.state[tp]
        for name, mine, theirs in (("p", p, tp.detach()), ("exp_avg", m, st["exp_avg"]), ("exp_avg_sq", v, st["exp_avg_sq"])):
            bad = int((ac.bits(mine) != ac.bits(theirs.numpy())).sum())
            assert bad == 0, "step %d: %d elements of %s differ" % (step, bad, name)


# ---------------------------------------------------------------- clip_coef against clip_grad_norm_
def _exact_grads(rs, sums):
    """tensors of +-2^-4 whose sums of squares are the given multiples of 2^-8: torch's norm of norms is exact on them when the sums are squares"""
    return [(rs.choice([-1.0, 1.0], int(round(s * 256))) * 2.0 ** -4).astype(np.float32) for s in sums]


@pytest.mark.parametrize("sums,total", [((4.0, 4.0, 1.0), 3.0), ((16.0, 9.0), 5.0), ((0.25, 0.25, 0.0625), 0.75)])
def test_clip_coef_is_clip_grad_norm_bit_for_bit(sums, total):
    rs = np.random.RandomState(11)
    gs = _exact_grads(rs, sums)
    assert ac.norm32(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in gs)) == np.float32(total)
    norms = [float(x) for x in rs.uniform(0.01, 1.5 * total, 60)] + [ac.max_norm_with_c(total, w) for w in (-1, 0, 1)] + [1e-3, 100.0]
    differ_from_division = 0
    for max_norm in norms:
        ps = [torch.nn.Parameter(torch.zeros(len(g))) for g in gs]
        for q, g in zip(ps, gs):
            q.grad = torch.from_numpy(g.copy())
        ret = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        assert _bits_equal(ret.numpy(), np.float32(total))
        coef = ac.clip_coef(np.float32(total), max_norm)
        for q, g in zip(ps, gs):
            assert _bits_equal(q.grad.numpy(), g * coef), "max_norm %r" % max_norm
        with np.errstate(all="ignore"):
            differ_from_division += int(min(np.float32(max_norm) / (np.float32(total) + np.float32(1e-6)), np.float32(1)) != coef)
    assert ac.raw_c(total, ac.max_norm_with_c(total, 0)) == 1 and ac.raw_c(total, ac.max_norm_with_c(total, -1)) < 1 < ac.raw_c(total, ac.max_norm_with_c(total, 1))
    # (the cases tell the reciprocal-and-multiply of Tensor.__rdiv__ from a division)
    assert differ_from_division > 0
    assert np.isnan(ac.clip_coef(np.float32(np.nan), 1.0))


# ---------------------------------------------------------------- the families
def _covers(cases, sizes):
    nf = len(sizes)
    for a in range(nf):
        for b in range(a + 1, nf):
            seen = {(c[a], c[b]) for c in cases}
            assert len(seen) == sizes[a] * sizes[b], "factors %d and %d: %d of %d pairs" % (a, b, len(seen), sizes[a] * sizes[b])


def test_family_a_holds_its_sizes_offsets_and_positions():
    ent = ac.family_a(_pairwise)
    st = [t for t in ent if t.stepped]
    assert len(st) >= ac.A_MIN_TENSORS > 2 * ac.BATCH + 1          # the 48th, 49th, 96th and 97th stepped tensors exist
    _covers([(ac.A_SIZES.index(t.size),) + t.offs for t in st], [len(ac.A_SIZES), 4, 4, 4, 4])
    for pos in (0, 47, 48, len(ent) - 1):
        assert not ent[pos].stepped
    assert {t.tag for t in ent if not t.stepped} == {"no gradient", "size 0"}
    assert sum(t.vec_chunks for t in st) >= 20 and any(t.vec_chunks == 0 and t.size >= ac.CHUNK for t in st)   # both launch paths, also on full chunks
    assert any(t.offs == (0, 0, 0, 0) and t.size % ac.CHUNK and t.size > ac.CHUNK for t in st)                  # a float4 chunk and a scalar tail in one tensor
    assert sum(t.size for t in st) < 1000000
    g = np.concatenate([t.g for t in st])
    v = np.concatenate([t.v for t in st])
    m = np.concatenate([t.m for t in st])
    mag = np.abs(g[(g != 0) & (np.abs(g) < 1e19)])
    assert mag.min() < 2.0 ** -38 and mag.max() > 2.0 ** 8 and (g > 0).any() and (g < 0).any() and (g == 0).any()
    assert (v >= 0).all() and ((v == 0) & (g != 0)).any() and ((v == 0) & (g == 0) & (m == 0)).any() and (np.abs(g) == np.float32(1e20)).any()


def test_family_a_reference_overflows_to_inf_and_leaves_dead_elements():
    st = [t for t in ac.family_a(_pairwise) if t.stepped]
    some_inf = False
    for t in st:
        p, gw, m, v = ac.adam_reference(t.p, t.g, t.m, t.v, step=ac.A_STEP, **ac.DEFAULTS)
        assert not np.isnan(np.concatenate([p, m, v])).any()
        dead = (t.g == 0) & (t.m == 0) & (t.v == 0)
        assert _bits_equal(p[dead], t.p[dead]) and _bits_equal(gw, t.g)
        inf = np.isinf(v)
        some_inf |= bool(inf.any())
        assert _bits_equal(p[inf], t.p[inf])      # v = inf: the update is 0
    assert some_inf


def test_family_b_is_a_covering_on_both_lerp_branches_without_nan():
    cases = ac.family_b(_pairwise)
    _covers([c[3] for c in cases], [len(f) for f in ac.B_FACTORS])
    assert ac.lerp_hi(0.5) and ac.lerp_hi(ac.B1_BELOW_HALF) and not ac.lerp_hi(ac.B1_OTHER_BRANCH) and not ac.lerp_hi(0.9) and ac.lerp_hi(0.4)
    assert np.float32(1.0 - ac.B1_OTHER_BRANCH) == np.nextafter(np.float32(0.5), np.float32(0))   # the two branches' nearest weights
    for hp, step, t, _ in cases:
        assert t.size == ac.CHUNK + 257 and t.vec_chunks == 1
        out = ac.adam_reference(t.p, t.g, t.m, t.v, step=step, **hp)
        assert not np.isnan(np.concatenate(out)).any(), (hp, step)


def test_family_c1_sums_are_exact_at_every_partial_sum():
    ent, total = ac.family_c1()
    assert total == ac.sumsq64(ent)
    assert any(t.size % ac.CHUNK for t in ent) and any(t.vec_chunks for t in ent) and any(t.offs[1] for t in ent)
    for t in ent:
        assert set(np.abs(t.g).tolist()) <= {2.0 ** -k for k in range(4, 10)}
        for i0 in range(0, t.size, ac.CHUNK):
            sq = t.g[i0:i0 + ac.CHUNK].astype(np.float64) ** 2
            for order in (sq, sq[::-1], np.sort(sq)):
                assert np.array_equal(np.cumsum(order.astype(np.float32), dtype=np.float32).astype(np.float64), np.cumsum(order))
    # every sum of at most 4096 squares is a multiple of 2^-18 below 2^4: 22 bits
    assert ac.CHUNK * 2.0 ** -8 <= 2.0 ** 4


def test_family_c2_has_tails_and_mixed_alignment():
    ent = ac.family_c2()
    assert len(ent) >= 60 > ac.BATCH
    assert sum(t.offs == (0, 0, 0, 0) for t in ent) >= 10 and sum(t.offs[1] != 0 for t in ent) >= 10
    assert any(t.vec_chunks and t.size % ac.CHUNK for t in ent)
    assert (12.5 + 0.5) * 2.0 ** -24 <= ac.C2_NORM_REL


def test_denormal_tensor_holds_denormals():
    t = ac.denormal_tensor()
    tiny = np.float32(2.0 ** -126)
    for x in (t.g, t.m, t.v):
        assert (np.abs(x) < tiny).all() and (x != 0).any()

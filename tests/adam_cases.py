"""TEST INFRASTRUCTURE: the fused Adam step (csrc/wn_optim.h, wn_optim.inl) restated on the host one fp32 rounding at a time, and the case
families of tests/test_gpu_adam_kernels.py.  numpy only: no torch, no GPU.  tests/test_adam_cases_host.py anchors the restatement to libm's fmaf
and to torch's CPU optimiser and checks that the families hold what they claim to hold.

Every device operation of wn_opt_adam is a correctly rounded IEEE operation (__fmul_rn, __fmaf_rn, __fsub_rn, __fadd_rn, __fdiv_rn, __fsqrt_rn), and
so is every numpy operation on float32 arrays; the one operation numpy lacks is the fused multiply-add (fma32).  The expected output of a case is
therefore a bit pattern, not a neighbourhood.

The families draw a covering selection with tests/kernel_lib.py's _pairwise, which the caller hands in (kernel_lib imports torch; this file does not).
"""
import math

import numpy as np

F32 = np.float32
CHUNK = 4096       # WN_OPT_CHUNK: elements per workgroup
BATCH = 48         # WN_OPT_TENSORS: tensors per launch
GUARD = 64         # sentinel words in front of and behind every tensor (a multiple of 4: the guard itself keeps 16-byte alignment)
NORM_ONLY, NORM_KEEP, NORM_GIVEN = 1, 2, 4


# ---------------------------------------------------------------- arithmetic
def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, on arrays: the product of two fp32 numbers is exact in fp64; the sum with c is formed with a TwoSum
    and, where it is inexact and its last bit is even, moved one ulp towards the true value (round to odd: 53 bits >= 24 + 2, so the cast to fp32
    then rounds as if from the exact value)."""
    a, b, c = (np.asarray(x, dtype=F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fin = np.isfinite(s)
        even = (s.view(np.int64) & 1) == 0
        up = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
        s = np.where(fin & (e != 0) & even, up, s)
        return s.astype(F32)


def scalars(lr, beta1, beta2, eps, weight_decay, step):
    """the fp32 scalars of a step: each is the double torch forms in Python, rounded once (wn_optim.inl, WnAdamScalars)"""
    bc1 = 1.0 - math.pow(beta1, float(step))
    bc2 = 1.0 - math.pow(beta2, float(step))
    return dict(neg_step=F32(-(lr / bc1)), sqrt_bc2=F32(math.sqrt(bc2)), omb1=F32(1.0 - beta1), b2=F32(beta2), omb2=F32(1.0 - beta2), eps=F32(eps),
                wd=F32(weight_decay))


def lerp_hi(beta1):
    """ATen's lerp evaluates b - (b - a) * (1 - w) from w = 0.5 up; w is the fp32 weight 1 - beta1"""
    return bool(F32(1.0 - beta1) >= F32(0.5))


def adam_reference(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, coef=1.0, addcdiv="fma", denom="div", sqrt=np.sqrt):
    """-> (p', g_written, m', v'): the formulas of csrc/wn_optim.h, one rounding at a time.
    addcdiv: "fma", the kernel's form and torch's on the device: v = fma(1 - beta2, g * g, v * beta2), p = fma(neg_step, m / denom, p); or "cpu",
        torch's CPU kernels: v = fma((1 - beta2) * g, g, v * beta2) (addcmul is self + value * t1 * t2 there), p = p + (neg_step * m) / denom.
    denom: "div", sqrt(v) / sqrt_bc2 (the kernel, torch's foreach form, torch on the CPU); or "rcp", sqrt(v) * fl32(1 / sqrt_bc2) with the
        reciprocal formed in double: what `tensor / python_scalar` computes on the device, torch's single-tensor form there.
    sqrt: the square root of fp32 arrays; numpy's is the correctly rounded one (tests/test_adam_cases_host.py hands in torch's CPU one, a vector
        library's, where it compares with torch's CPU Adam)."""
    assert addcdiv in ("fma", "cpu") and denom in ("div", "rcp")
    k = scalars(lr, beta1, beta2, eps, weight_decay, step)
    p, g, m, v = (np.asarray(x, dtype=F32) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        g = g * F32(coef)
        gw = g.copy()
        if k["wd"] != 0:
            g = fma32(k["wd"], p, g)
        if lerp_hi(beta1):
            m = fma32(-(g - m), F32(1) - k["omb1"], g)
        else:
            m = fma32(k["omb1"], g - m, m)
        v = v * k["b2"]
        v = fma32(k["omb2"], g * g, v) if addcdiv == "fma" else fma32(k["omb2"] * g, g, v)
        if denom == "div":
            d = sqrt(v) / k["sqrt_bc2"] + k["eps"]
        else:
            d = sqrt(v) * F32(1.0 / math.sqrt(1.0 - math.pow(beta2, float(step)))) + k["eps"]
        if addcdiv == "fma":
            p = fma32(k["neg_step"], m / d, p)
        else:
            p = p + (k["neg_step"] * m) / d
    return p, gw, m, v


def clip_coef(total32, max_norm):
    """the clip coefficient in fp32: c = max_norm * (1 / (total + 1e-6f)) -- what Python's `max_norm / (total_norm + 1e-6)` computes on a tensor
    (Tensor.__rdiv__ is reciprocal() * other) -- and coef = c unless c >= 1.  A NaN stays a NaN."""
    with np.errstate(all="ignore"):
        c = (F32(1) / (F32(total32) + F32(1e-6))) * F32(max_norm)
    return c if not (c >= 1) else F32(1)


def raw_c(total32, max_norm):
    with np.errstate(all="ignore"):
        return (F32(1) / (F32(total32) + F32(1e-6))) * F32(max_norm)


def max_norm_with_c(total32, want):
    """-> a max_norm next to total + 1e-6f whose c is exactly 1 (want = 0), the largest below 1 (-1) or the smallest above 1 (+1)"""
    x = F32(total32) + F32(1e-6)
    cands = [x]
    for _ in range(8):
        cands = [np.nextafter(cands[0], F32(0))] + cands + [np.nextafter(cands[-1], F32(np.inf))]
    if want == 0:
        hits = [c for c in cands if raw_c(total32, c) == 1]
        return float(hits[len(hits) // 2])
    if want < 0:
        return float(max(c for c in cands if raw_c(total32, c) < 1))
    return float(min(c for c in cands if raw_c(total32, c) > 1))


def norm32(sumsq64):
    return F32(np.sqrt(np.float64(sumsq64)))


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


# ---------------------------------------------------------------- element values of the bit-exact families
def values(rs, n, dead=True, huge=True):
    """-> p, g, m, v of n elements: gradients of 2^-40 .. 2^10 in both signs with exact zeros, v >= 0 with v = 0 beside g != 0, a few |g| of 1e20
    and 1e22 (g * g, scaled by 1 - beta2, overflows: v becomes inf and the update 0), and -- dead=True -- elements with v = g = m = 0.
    dead=False (eps = 0): no exact-zero gradient either, so that no 0 / 0 arises (torch's NaN too, but a payload is not worth pinning)."""
    def spread(lo, hi):
        return (rs.choice([-1.0, 1.0], n) * np.ldexp(rs.uniform(1, 2, n), rs.randint(lo, hi + 1, n))).astype(F32)
    p, g, m = spread(-12, 2), spread(-40, 9), spread(-40, 9)
    v = np.ldexp(rs.uniform(1, 2, n), rs.randint(-80, 19, n)).astype(F32)
    kind = rs.randint(0, 32, n)
    v[kind == 0] = 0                                   # v = 0, g != 0
    if dead:
        g[kind == 1] = 0                               # exact-zero gradients
        z = kind == 2
        g[z] = 0; m[z] = 0; v[z] = 0                   # nothing to do: p must come back bit-identical (eps > 0)
    if huge and n >= 4:
        i = rs.choice(n, min(4, n), replace=False)
        g[i] = np.array([1e20, -1e20, 1e22, -1e22], dtype=F32)[:len(i)]
        v[i] = np.abs(v[i]) + F32(1)
    return p, g, m, v


class Tensor:
    """one entry of a call's argument arrays: its inputs, the element offsets of its four buffers from a 16-byte boundary, and whether it is stepped"""

    def __init__(self, size, offs=(0, 0, 0, 0), p=None, g=None, m=None, v=None, has_grad=True, tag=""):
        self.size, self.offs, self.has_grad, self.tag = size, tuple(offs), has_grad, tag
        self.p, self.g, self.m, self.v = p, g, m, v

    @property
    def stepped(self):
        return self.has_grad and self.size > 0

    @property
    def vec_chunks(self):
        """the workgroups that take the float4 path: all four pointers 16-byte aligned and a full chunk (wn_opt_adam's `vec`)"""
        return self.size // CHUNK if self.offs == (0, 0, 0, 0) else 0


DEFAULTS = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0)


# ---------------------------------------------------------------- A: sizes, alignment and batching
A_SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289)
A_STEP = 3
A_MIN_TENSORS = 100


def family_a(pairwise, seed=101):
    """-> the entries of ONE call: a covering of (size, offset of p, of g, of m, of v), all-aligned copies of 4096 and 8192 up to at least
    A_MIN_TENSORS stepped tensors, and entries without a gradient / of size 0 at positions 0, 47, 48 and last."""
    rs = np.random.RandomState(seed)
    sel = pairwise([len(A_SIZES), 4, 4, 4, 4], seed=seed)
    stepped = [(A_SIZES[s], (a, b, c, d)) for s, a, b, c, d in sel]
    k = 0
    while len(stepped) < A_MIN_TENSORS:
        stepped.append(((4096, 8192)[k % 2], (0, 0, 0, 0)))
        k += 1
    stepped += [(size, (0, 0, 0, 0)) for size in (4097, 8193, 12289)]    # float4 chunks and a scalar tail in one tensor
    order = rs.permutation(len(stepped))
    stepped = [stepped[i] for i in order]
    entries = []
    for size, offs in stepped:
        p, g, m, v = values(rs, size)
        entries.append(Tensor(size, offs, p, g, m, v))

    def skipped(j):
        if j % 2 == 0:    # no gradient: the size is real, the gradient pointer NULL
            p, g, m, v = values(rs, 300)
            return Tensor(300, (0, 1, 2, 3), p, None, m, v, has_grad=False, tag="no gradient")
        p, g, m, v = values(rs, 8)   # size 0: the pointers are real (eight elements the call must not touch)
        return Tensor(0, (1, 0, 3, 2), p, g, m, v, tag="size 0")
    # positions of the final array: 0, 47, 48 and last (inserted in increasing order, so each lands where it is named)
    for j, pos in enumerate((0, 47, 48)):
        entries.insert(pos, skipped(j))
    entries.append(skipped(3))
    return entries


# ---------------------------------------------------------------- B: hyper-parameters
B_SIZE = CHUNK + 257
# beta1 around 0.5: the branch follows the fp32 weight.  The double next below 0.5 gives the weight 0.5 + 2^-54, which rounds to the fp32 0.5: the
# same branch as 0.5 itself.  0.5 + 2^-25 is the nearest beta1 whose fp32 weight (0.5 - 2^-25, exact) lies below 0.5: the other branch.
B1_BELOW_HALF, B1_OTHER_BRANCH = float(np.nextafter(0.5, 0.0)), 0.5 + 2.0 ** -25
B_BETA1 = (0.0, 0.4, 0.5, B1_BELOW_HALF, B1_OTHER_BRANCH, 0.9)
B_BETA2 = (0.0, 0.9, 0.999)
B_EPS = (0.0, 1e-8, 1e-3)
B_WD = (0.0, 0.01)
B_STEP = (1, 2, 1000, 10 ** 6)
B_LR = (1e-3, 1.0)
B_FACTORS = (B_BETA1, B_BETA2, B_EPS, B_WD, B_STEP, B_LR)


def family_b(pairwise, seed=202):
    """-> [(hyper-parameters, step, Tensor)]: one aligned tensor of a full chunk and a tail per case of a pairwise covering"""
    out = []
    for n, idx in enumerate(pairwise([len(f) for f in B_FACTORS], seed=seed)):
        b1, b2, eps, wd, step, lr = (f[i] for f, i in zip(B_FACTORS, idx))
        rs = np.random.RandomState(seed + 1 + n)
        p, g, m, v = values(rs, B_SIZE, dead=eps > 0)
        out.append((dict(lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd), step, Tensor(B_SIZE, (0, 0, 0, 0), p, g, m, v), idx))
    return out


# ---------------------------------------------------------------- C1 / C3: gradients whose sum of squares is exact
C1_SIZES = (4097, 4095, 8192, 100)
C1_OFFS = ((0, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 0), (2, 3, 1, 0))


def family_c1(seed=303, sizes=C1_SIZES, offs=C1_OFFS):
    """gradients of +-2^-k, k in 4 .. 9: the squares are 2^-8 .. 2^-18, so every sum of at most 4096 of them is a multiple of 2^-18 below 2^4 = 22
    bits, exact in fp32 in whatever order it is formed; the fp64 total of the workgroups' partials is exact too.  -> (entries, the exact sum)"""
    rs = np.random.RandomState(seed)
    entries, total = [], 0.0
    for size, o in zip(sizes, offs):
        p, _, m, v = values(rs, size, huge=False)
        g = (rs.choice([-1.0, 1.0], size) * np.ldexp(1.0, -rs.randint(4, 10, size))).astype(F32)
        entries.append(Tensor(size, o, p, g, m, v))
        total += float(np.sum(g.astype(np.float64) ** 2))
    return entries, total


def sumsq64(entries):
    return float(sum(np.sum(t.g.astype(np.float64) ** 2) for t in entries if t.stepped))


# ---------------------------------------------------------------- C2: random gradients
C2_TENSORS = 60
# The sum of squares the kernel reports: every term passes through at most 25 fp32 roundings before it reaches the fp64 atomic (recounted from
# wn_opt_sumsq: 1 for the square; on the scalar path up to 4096 / 256 = 16 adds of a thread's running sum -- on the float4 path 2 adds inside the
# float4 and up to 4 of the running sum --; 6 levels of wn_wave_sum; 2 adds of the four wave partials; a contraction of square and add into an FMA
# only removes roundings; 1 + 16 + 6 + 2 = 25 is the recount, one more than the issue's 24).  All partial sums are non-negative, so the sum is within
# 25 * 2^-24 relative, the norm within half of that, plus half an ulp for the cast of the double root: (12.5 + 0.5) * 2^-24 < 2^-20.
C2_NORM_REL = 2.0 ** -20


def family_c2(seed=404):
    rs = np.random.RandomState(seed)
    sizes = [1, 257, 4095, 4096, 4097, 8193] + [int(s) for s in rs.randint(1, 3 * CHUNK, C2_TENSORS - 6)]
    entries = []
    for n, size in enumerate(sizes):
        offs = (0, 0, 0, 0) if n % 3 == 0 else tuple(int(x) for x in rs.randint(0, 4, 4))
        p, _, m, v = values(rs, size, huge=False)
        g = (rs.standard_normal(size) * np.ldexp(1.0, rs.randint(-12, 3))).astype(F32)
        entries.append(Tensor(size, offs, p, g, m, v))
    return entries


# ---------------------------------------------------------------- D: a tensor of fp32 denormals
def denormal_tensor(seed=505, size=CHUNK + 100):
    """g, m and v hold fp32 denormals (exp_avg gets there after a few hundred steps of zero gradient: 1e-3 * 0.9^n is denormal from n ~ 770)"""
    rs = np.random.RandomState(seed)
    tiny = lambda: (rs.choice([-1.0, 1.0], size) * rs.randint(1, 1 << 23, size) * 2.0 ** -149).astype(F32)   # noqa: E731
    p = (rs.standard_normal(size) * 0.1).astype(F32)
    g, m, v = tiny(), tiny(), np.abs(tiny())
    g[::3] = 0
    return Tensor(size, (0, 0, 0, 0), p, g, m, v)

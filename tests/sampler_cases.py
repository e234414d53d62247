"""The cases of the sampler kernel tests and their references; numpy only, no GPU (tests/test_sampler_cases_host.py checks the cases themselves,
tests/test_gpu_sampler_kernels.py runs them through wn_sample_1w and wn_sample).

References
  * draw64: wavenet_model.py:280-294 on the same float32 inputs.  x = fl32(logits - reg), x = fl32(x / T) when not greedy -- both operations are
    correctly rounded in numpy and on the GPU, so the inputs to exp are the same bits --, then float64: p = exp(x - max), cdf = cumsum(p) / cdf[-1],
    idx = min(searchsorted(cdf, u, 'right'), C - 1); greedy: the first index of the maximum of x.  One thing of float32 is kept: a mass whose
    x - max lies below -104 is 0.0, as it is in the reference's float32 softmax (float64 would keep e^-200 = 1e-87 alive, and u = 0.0 would then
    stop at class 0 instead of passing the leading zero-mass classes as the reference does).  No family has a mass between that cut and the
    smallest normal float, so nothing else depends on where exactly it lies.
  * the reference's float32 pipeline is parity_common.softmax_cdf (the host test holds it to draw64 on every decided and every exact row).

Decision rule (the band of parity_common.py: 1e-6).  With identical exp inputs the factor 1/sum cancels in cdf / cdf[-1]; a mass then carries the ulp
of expf and one product rounding (~1.8e-7 relative), a few 1e-7 absolute on a CDF value.  A sampled row is DECIDED when u is farther than BAND from
every float64 CDF value: there the kernel's index is draw64's.  On an undecided row the kernel may return any class whose CDF interval reaches
within BAND of u.  The rows of the exact families (b, c, d, e) have no band: masses and sums are the same numbers in every order and every precision.

Families (fixed seeds; every one for C = 256 and both kernels, for the generic kernel also C = 128, 100, 40: at 100 and 40 the last of the 16 groups
are empty, chunk 7 and 3)
  a  spread: randn * s logits, temperatures with and without the division, with and without the regulariser; per logits row random uniforms, the
     midpoint of every class of mass > 1e-5, and that class's upper boundary -/+ 4e-6 (the upper one where the next class has mass > 1e-5 as well,
     so that both are decided by construction)
  b  ties: k classes share the maximum, the others sit 200 below (expf gives exactly 0); masses fl32(1/k), cdf_j / total == j / k as Python
     computes it; u = j/k and nextafter(j/k, 0), with u = 0.0, nextafter(1.0, 0) and 1.0 (the clamp) among them
  c  one-hot by temperature: top-2 gap >= 0.25 at T = 1e-3
  d  zero-mass runs inside the support: masses 0 or within 2^-20 of the maximum; midpoints, and (with all live masses equal, so that the value is
     the same number on both sides) u on the CDF value that a class and the zero-mass run behind it share
  e  greedy: the flag, T = 0 and T < 0 (the flag the samplers get is their callers' `greedy != 0 || !(T > 0)`), ties on every seam, -0.0 against +0.0,
     a tie only the regulariser breaks, values that only the division would tie
The tied classes and the zero runs lie on the structural seams: classes 3|4 (lane), 63|64 and 191|192 (16-lane DPP row), 127|128 (row_bcast:31), 0 and
255 for wn_sample_1w; both sides of every chunk boundary in use and the last class for wn_sample.

Out of scope: NaN and infinite logits (not reachable from finite weights), and masses in the denormal range -- every family keeps x - max out of
(-104, -87]."""
import functools
import math

import numpy as np

BAND = 1e-6
KERNELS = ("one_wave", "generic")
FAMILIES = ("a", "b", "c", "d", "e")
EXACT = ("b", "c", "d", "e")
GROUPS = 16            # WN_SAMPLER_GROUPS
REGULARIZE = 0.002
FAR = np.float32(200.0)
ONE_BELOW = math.nextafter(1.0, 0.0)
UNDERFLOW = -104.0     # x - max below which a float32 mass IS zero (half the smallest denormal, 2^-150, is e^-103.97): see draw64 in the docstring


def class_counts(kernel):
    return (256,) if kernel == "one_wave" else (256, 128, 100, 40)


def case_ids():
    return [(k, f, C) for k in KERNELS for f in FAMILIES for C in class_counts(k)]


def unit(kernel, C):
    """classes per scan unit: a lane's four, or a group's chunk"""
    return 4 if kernel == "one_wave" else (C + GROUPS - 1) // GROUPS


def seams(kernel, C):
    """boundaries b (the seam lies between class b - 1 and class b)"""
    if kernel == "one_wave":
        return [4, 64, 128, 192]
    ch = unit(kernel, C)
    return list(range(ch, C, ch))


def regularizer(C):
    import c_oracle
    return c_oracle.regularizer_array(C, REGULARIZE)


# ---------------------------------------------------------------- references
def x32(logits32, reg32, T32, greedy):
    x = np.asarray(logits32, dtype=np.float32)
    if reg32 is not None:
        x = (x - np.asarray(reg32, dtype=np.float32)).astype(np.float32)
    if not greedy:
        x = (x / np.float32(T32)).astype(np.float32)
    return x


def cdf64(x, shift_unit=0):
    """float64 CDF of the softmax of the float32 row x.  shift_unit > 0: the WRONG scan whose units (lanes, chunks) take their prefix from one unit too
    early -- for the host test, which shows that the data can tell it."""
    d = x.astype(np.float64) - float(x.max())
    p = np.where(d < UNDERFLOW, 0.0, np.exp(d))
    c = np.cumsum(p)
    tot = c[-1]
    if shift_unit:
        g = np.arange(len(x)) // shift_unit
        ut = np.bincount(g, weights=p)
        c = c - np.where(g > 0, ut[np.maximum(g - 1, 0)], 0.0)
    return c / tot


def pick(cdf, u, side="right", clamp=True):
    """searchsorted(cdf, u, side), said as a count so that it also has a meaning on the non-monotone CDF of a wrong scan"""
    i = int(np.count_nonzero(cdf <= u if side == "right" else cdf < u))
    return min(i, len(cdf) - 1) if clamp else i


def draw64(logits32, reg32, T32, u, greedy):
    x = x32(logits32, reg32, T32, greedy)
    if greedy:
        return int(np.argmax(x))
    return pick(cdf64(x), u)


def margin(cdf, u):
    return float(np.abs(cdf - u).min())


def allowed_undecided(cdf, u, idx):
    """the class idx reaches within BAND of u"""
    lo = cdf[idx - 1] if idx > 0 else 0.0
    return lo - BAND <= u <= cdf[idx] + BAND


# ---------------------------------------------------------------- containers
class Part:
    """the rows of a family that one launch takes: one regulariser (or none)"""

    def __init__(self, C, reg):
        self.C, self.reg = C, reg
        self.rows = []      # (logits32, T32, u, greedy flag the sampler gets, expected index, kind, base)
        self.bases = []     # family a: the float64 CDF of every logits row

    def add(self, logits, T, u, greedy, expect, kind, base=-1):
        self.rows.append((np.asarray(logits, dtype=np.float32), np.float32(T), float(u), int(bool(greedy)), int(expect), kind, base))

    def finish(self):
        r = self.rows
        self.n = len(r)
        self.logits = np.ascontiguousarray(np.stack([q[0] for q in r]))
        self.temp = np.array([q[1] for q in r], dtype=np.float32)
        self.u = np.array([q[2] for q in r], dtype=np.float64)
        self.greedy = np.array([q[3] for q in r], dtype=np.int32)
        self.expect = np.array([q[4] for q in r], dtype=np.int32)
        self.kind = [q[5] for q in r]
        self.base = np.array([q[6] for q in r], dtype=np.int64)
        self.cdf = np.stack(self.bases) if self.bases else None
        del self.rows
        return self


class Family:
    def __init__(self, name, kernel, C, parts):
        self.name, self.kernel, self.C, self.exact = name, kernel, C, name in EXACT
        self.parts = [p.finish() for p in parts if p.rows]
        self.n = sum(p.n for p in self.parts)


def _seed(name, kernel, C):
    return 1000 * (FAMILIES.index(name) + 1) + 10 * C + KERNELS.index(kernel)


def _out_of_denormals(logits, reg, T):
    """push the classes whose mass would be a denormal (x - max in (-104, -87]) further down: 20 T in the logit is 20 in x"""
    for _ in range(8):
        x = x32(logits, reg, T, False)
        d = x.astype(np.float64) - float(x.max())
        bad = (d > -104.5) & (d <= -86.5)
        if not bad.any():
            return logits
        logits = np.where(bad, logits - np.float32(20.0) * np.float32(T), logits).astype(np.float32)
    raise AssertionError("denormal masses remain")


# ---------------------------------------------------------------- a: spread
RANDOM_PER_ROW = 10


def _family_a(kernel, C):
    rs = np.random.RandomState(_seed("a", kernel, C))
    parts = [Part(C, None), Part(C, regularizer(C))]
    for part in parts:
        for s in (0.3, 3.0, 30.0):
            for T in (1.0, 0.8, 2.5, 0.05):
                logits = _out_of_denormals((rs.standard_normal(C) * s).astype(np.float32), part.reg, T)
                cdf = cdf64(x32(logits, part.reg, T, False))
                base = len(part.bases)
                part.bases.append(cdf)
                mass = np.diff(cdf, prepend=0.0)
                for u in rs.random_sample(RANDOM_PER_ROW):
                    part.add(logits, T, u, 0, pick(cdf, u), "random", base)
                for i in np.nonzero(mass > 1e-5)[0]:
                    part.add(logits, T, 0.5 * ((cdf[i - 1] if i else 0.0) + cdf[i]), 0, i, "mid", base)
                    part.add(logits, T, cdf[i] - 4e-6, 0, i, "below", base)
                    if i + 1 < C and mass[i + 1] > 1e-5:
                        part.add(logits, T, cdf[i] + 4e-6, 0, i + 1, "above", base)
    return Family("a", kernel, C, parts)


# ---------------------------------------------------------------- b: ties
def _tie_sets(kernel, C, k, rs):
    sets = set()
    if k == 1:
        for b in seams(kernel, C):
            sets.add((b - 1,)); sets.add((b,))
        sets.add((0,)); sets.add((C - 1,))
    else:
        for b in seams(kernel, C):
            st = min(max(b - k // 2, 0), C - k)
            sets.add(tuple(range(st, st + k)))
        sets.add(tuple(range(k)))
        sets.add(tuple(range(C - k, C)))
        sets.add(tuple(sorted(rs.choice(C, k, replace=False).tolist())))    # scattered: zero-mass classes between the tied ones
    return sorted(sets)


def _family_b(kernel, C):
    rs = np.random.RandomState(_seed("b", kernel, C))
    part = Part(C, None)
    seam_classes = set(seams(kernel, C)) | {b - 1 for b in seams(kernel, C)} | {0, C - 1}
    top = np.float32(1.5)
    n = 0
    for k in sorted({k for k in (1, 2, 3, 4, 5, 8, 64, C - 1, C) if 1 <= k <= C}):
        for tied in _tie_sets(kernel, C, k, rs):
            T = (1.0, 0.5)[n % 2]    # (1.0: the form of wn_sample_1w without the division; 0.5: an exact division, -200 -> -400)
            n += 1
            logits = np.full(C, top - FAR, np.float32)
            logits[list(tied)] = top
            if k <= 8:
                js = range(k + 1)
            else:
                js = {0, 1, k // 2, k - 1, k}
                for j, c in enumerate(tied):
                    if c in seam_classes:
                        js |= {j, j + 1}
                js = sorted(j for j in js if j <= k)
            for j in js:
                u = j / k
                part.add(logits, T, u, 0, tied[j] if j < k else C - 1, "on")           # u = 1.0: the clamp
                if j > 0:
                    part.add(logits, T, math.nextafter(u, 0.0), 0, tied[j - 1], "under")
    return Family("b", kernel, C, [part])


# ---------------------------------------------------------------- c: one-hot by temperature
def _family_c(kernel, C):
    rs = np.random.RandomState(_seed("c", kernel, C))
    part = Part(C, None)
    T = np.float32(1e-3)
    hot = sorted(set(seams(kernel, C)) | {b - 1 for b in seams(kernel, C)} | {0, C - 1}) + rs.randint(0, C, 24).tolist()
    for i in hot:
        logits = (rs.standard_normal(C) * 3).astype(np.float32)
        logits[i] = np.float32(np.delete(logits, i).max()) + np.float32(0.25) + np.float32(rs.randint(0, 64)) / np.float32(64)
        for u in (0.0, 0.5, ONE_BELOW):
            part.add(logits, T, u, 0, i, "onehot")
    return Family("c", kernel, C, [part])


# ---------------------------------------------------------------- d: zero-mass runs inside the support
def _zero_runs(kernel, C):
    runs = set()
    for b in seams(kernel, C):
        for L in (1, 2, 5, 2 * unit(kernel, C) + 1):
            st = min(max(b - (L + 1) // 2, 1), C - 1 - L)
            if st >= 1:
                runs.add((st, st + L))
        runs.add((b, b + 1))
    for L in (1, 5):
        if L < C - 1:
            runs.add((0, L)); runs.add((C - L, C))      # leading and trailing runs
    return sorted(r for r in runs if 0 <= r[0] < r[1] <= C)


def _family_d(kernel, C):
    rs = np.random.RandomState(_seed("d", kernel, C))
    part = Part(C, None)
    top = np.float32(1.5)
    for n, (a, b) in enumerate(_zero_runs(kernel, C)):
        live = np.ones(C, bool)
        live[a:b] = False
        if n % 3 == 0 and a > 12:      # a second run further down
            live[a - 9:a - 6] = False
        k = int(live.sum())
        # equal live masses: every CDF value is count / k on both sides
        eq = np.where(live, top, top - FAR).astype(np.float32)
        cnt = np.cumsum(live)
        if a > 0:
            part.add(eq, 1.0, cnt[a - 1] / k, 0, b if b < C else C - 1, "shared")           # class a-1 and the whole run are passed at once (b == C: the clamp)
            part.add(eq, 1.0, math.nextafter(cnt[a - 1] / k, 0.0), 0, a - 1, "under")
        else:
            part.add(eq, 1.0, 0.0, 0, b, "shared")                                           # leading run: cdf == 0.0 <= u
        # live masses within 2^-20 of the maximum: midpoints, decided by ~1 / (2 k)
        near = np.where(live, top - rs.randint(0, 5, C).astype(np.float32) * np.float32(2.0 ** -22), top - FAR).astype(np.float32)
        near[np.nonzero(live)[0][rs.randint(0, k)]] = top
        cdf = cdf64(x32(near, None, 1.0, False))
        for i in sorted({a - 1, b, int(np.nonzero(live)[0][0]), int(np.nonzero(live)[0][-1]), int(np.nonzero(live)[0][rs.randint(0, k)])}):
            if 0 <= i < C and live[i]:
                part.add(near, 1.0, 0.5 * ((cdf[i - 1] if i else 0.0) + cdf[i]), 0, i, "mid")
    return Family("d", kernel, C, [part])


# ---------------------------------------------------------------- e: greedy
def tie_by_division(T=3.0):
    """two adjacent floats a < b with fl32(a / T) == fl32(b / T): the maximum is b's class only as long as nobody divides"""
    a = np.float32(1.5)
    for _ in range(64):
        b = np.nextafter(a, np.float32(4))
        if np.float32(a / np.float32(T)) == np.float32(b / np.float32(T)):
            return a, b
        a = b
    raise AssertionError("no pair found")


def _family_e(kernel, C):
    rs = np.random.RandomState(_seed("e", kernel, C))
    plain, withreg = Part(C, None), Part(C, regularizer(C))
    sm = seams(kernel, C)

    def low():
        return (rs.standard_normal(C) * 3 - 20).astype(np.float32)

    def add(part, logits, kind, T=0.7, flag=1):
        greedy = bool(flag) or not (T > 0)          # the samplers' callers
        assert greedy
        part.add(logits, T, 0.0, 1, draw64(logits, part.reg, T, 0.0, True), kind)

    for T, flag in ((0.7, 1), (1.0, 1), (0.0, 0), (-1.0, 0), (0.0, 1)):
        for _ in range(8):
            add(plain, (rs.standard_normal(C) * 3).astype(np.float32), "random", T, flag)
            add(withreg, (rs.standard_normal(C) * 3).astype(np.float32), "random", T, flag)
    for b in sm:
        for tied in ((b - 1, b), (b, C - 1), (b - 1, b, C - 1), (0, b)):
            x = low(); x[list(tied)] = np.float32(2.25)
            add(plain, x, "tie")
    for T, flag in ((0.7, 1), (0.0, 0)):
        add(plain, np.full(C, np.float32(-3.5)), "equal", T, flag)
        add(plain, np.zeros(C, np.float32), "equal", T, flag)
    i, j = sm[0] - 1, sm[-1]
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):
        x = np.full(C, np.float32(-1)); x[i] = np.float32(first); x[j] = np.float32(second)
        add(plain, x, "zeros")
    x = low(); x[C - 1] = np.float32(1)
    add(plain, x, "last")
    x = low(); x[0] = np.float32(1)
    add(plain, x, "first")
    # the regulariser grows with |c - C/2|: of two equal logits the one nearer the middle wins; at equal distance the tie stays and the first wins
    for tied in ((1, C // 2), (C // 2 + 3, C - 1), (C // 2 - 2, C // 2 + 2), (sm[0] - 1, sm[0])):
        x = low(); x[list(tied)] = np.float32(40)
        add(withreg, x, "regtie")
    # greedy x is NOT divided: a division would tie the two largest values (and the earlier class would win), or turn the order round (T < 0)
    a, bb = tie_by_division(3.0)
    for lo_c, hi_c in ((sm[0] - 1, sm[0]), (0, C - 1)):
        x = low(); x[lo_c] = a; x[hi_c] = bb
        add(plain, x, "undivided", 3.0, 1)
    return Family("e", kernel, C, [plain, withreg])


_BUILD = {"a": _family_a, "b": _family_b, "c": _family_c, "d": _family_d, "e": _family_e}


@functools.lru_cache(maxsize=None)
def family(name, kernel, C):
    return _BUILD[name](kernel, C)

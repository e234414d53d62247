"""The cases of the sampling-filter tests (top-k, nucleus / top-p: include/wn_abi.h wn_set_sampling) and their float64 reference; numpy only, no GPU.
tests/test_sampler_filter_cases_host.py checks the cases themselves, tests/test_gpu_sampler_filter_kernels.py runs them through wn_sample_1w<true> and
wn_sample, tests/test_gpu_sampling_filters.py replays whole jobs through draw64_filtered.  Everything the unfiltered draw needs -- x32, cdf64's UNDERFLOW
cut, pick, the seams, the band -- is tests/sampler_cases.py's, imported.

Reference
  filter64(x, top_k, top_p) -> (keep, membership_decided) on the float32 row x the samplers form:
    top_k (0 and >= C: off): tau = the k-th largest x, keep x_i >= tau -- float32 values that are the same bits on host and device: exact, no band.
    top_p (0 and >= 1: off; rounded to float32 first, as the C ABI takes a float), on the survivors: m_i = exp(x_i - max) in float64 (0 below UNDERFLOW
      and for the dropped), T = sum m, G_i = sum of the m_j with x_j > x_i strictly, keep iff G_i < top_p * T.
    membership_decided: |G_i / T - top_p| > BAND for every surviving class of non-zero mass.  The kernels sum float32 masses in float64: their G_i / T
      differs by the ulp of expf (~2.4e-7 on a quotient), so on a decided row they keep the same classes.
  draw64_filtered: sampler_cases.draw64 with the dropped classes' masses at 0.0.
A row is DECIDED when its membership is decided and u is farther than BAND from every filtered CDF value (or the row is exact: tied survivors, whose
CDF values are j / a in every precision).  On an undecided row the kernel may return any class that one of the memberships the band allows keeps and
whose CDF interval under that membership reaches within BAND of u (allowed_filtered).

Families (fixed seeds; wn_sample_1w at C = 256, wn_sample at C = 256, 100 and 40 -- empty trailing groups, chunks of 7 and 3), every one placed on the
seams sampler_cases.seams() gives, class 0 and the last class:
  f  two levels, x = 0 on a classes (A) and x = -0.7 on b classes (B), the rest 200 below; top_k = a cuts between the levels.  The survivors are tied:
     u = j / a and one ulp below have exact answers.  B classes sit between A classes on both sides of every seam -- zero-mass runs made by the filter.
  g  top_k strictly inside a tied level: inside A (all of A stays, B goes: exact ties) and inside B (A and B stay: midpoints, decided by ~1 / (2 (a + b)))
  h  the two levels cut by top_p, at least 0.05 away from a / (a + b e^-0.7) on either side: B dropped (exact ties) / B kept (midpoints); and three
     levels with top_k dropping the third and top_p between a / T(all) and a / T(survivors), 0.05 from both: B goes only if top_p sees the survivors' total
  i  top_k = 1 on a unique maximum: the argmax for u = 0.0, 0.5 and 1 - ulp
  j  the off values (0, 0), top_k = C, top_k = C + 7, top_p = 1.0 on the decided rows of sampler_cases' family a: draw64's index
  k  spread rows (randn * s, s in 0.5 .. 8, T in 0.5, 1, 1.7; with and without the regulariser) under (top_k, top_p) in K_FILTERS; random uniforms and
     the midpoint of every kept class of mass > 1e-5.  At most UNDECIDED_CAP of its rows may be undecided: a condition on these inputs (asserted on
     the host), not a measurement of a kernel.
  e  sampler_cases' greedy family with a filter set: the filter is ignored
Mutants (host test): `>` for `>=` in top_k, `<=` for `<` in top_p, top_p before top_k, top_p over the unfiltered total.  The second one can only show
where G_i == top_p * T EXACTLY, and no two levels of a float row have masses exp() makes commensurable: it is told apart with a mass function that
weighs two levels the same (filter64's `mass` argument), the others on rows of g and h."""
import functools
import math

import numpy as np

import sampler_cases as sc

BAND = sc.BAND
KERNELS = sc.KERNELS
FAMILIES = ("f", "g", "h", "i", "j", "k", "e")
BY_CONSTRUCTION = ("f", "g", "h", "i", "j", "e")     # no undecided row
TIE_KINDS = ("on", "under", "argmax")                 # rows whose survivors are tied (or one): the CDF values are j / a in every precision, u may sit ON one
K_FILTERS = ((0, 0.9), (0, 0.5), (40, 0.95), (5, 0.0), (0, 0.999), (0, 1e-3))
UNDECIDED_CAP = 0.01
LOW = np.float32(-0.7)
LOWER = np.float32(-1.4)
FAR = sc.FAR


def class_counts(kernel):
    return (256,) if kernel == "one_wave" else (256, 100, 40)


def case_ids():
    return [(k, f, C) for k in KERNELS for f in FAMILIES for C in class_counts(k)]


# ---------------------------------------------------------------- reference
def _mass64(d):
    return np.where(d < sc.UNDERFLOW, 0.0, np.exp(d))


def top_k_on(top_k, C):
    return 0 < top_k < C


def top_p_on(top_p):
    return 0.0 < float(np.float32(top_p)) < 1.0


def quotients(x, keep, mass=_mass64):
    """(G_i / T per class, the survivors' masses) of the float32 row x after top_k left `keep`"""
    m = np.where(keep, mass(x.astype(np.float64) - float(x.max())), 0.0)
    order = np.argsort(-x, kind="stable")
    xs, cs = x[order], np.cumsum(m[order])
    above = np.searchsorted(-xs, -x, side="left")           # classes strictly greater than x_i
    G = np.where(above > 0, cs[np.maximum(above - 1, 0)], 0.0)
    return G, float(m.sum()), m


def filter64(x, top_k, top_p, mass=_mass64, k_strict=False, p_inclusive=False, p_first=False, p_total_all=False):
    """-> (keep mask, membership decided).  The keyword switches are the MUTANTS of the host test, never the contract."""
    x = np.asarray(x, dtype=np.float32)
    C = len(x)
    keep_k = np.ones(C, bool)
    if top_k_on(top_k, C):
        tau = np.sort(x)[C - top_k]
        keep_k = (x > tau) if k_strict else (x >= tau)
    if not top_p_on(top_p):
        return keep_k, True
    p = float(np.float32(top_p))
    G, T, m = quotients(x, np.ones(C, bool) if (p_first or p_total_all) else keep_k, mass)
    if T == 0.0:
        return np.zeros(C, bool), True                       # (a mutant that dropped everything)
    keep_p = (G <= p * T) if p_inclusive else (G < p * T)
    live = keep_k & (m > 0)
    decided = bool((np.abs(G[live] / T - p) > BAND).all())
    return keep_k & keep_p, decided


def memberships(x, top_k, top_p):
    """the keep masks the band allows: the float64 one, and the ones with top_p moved by BAND either way"""
    out = [filter64(x, top_k, top_p)[0]]
    if top_p_on(top_p):
        x = np.asarray(x, dtype=np.float32)
        keep_k = filter64(x, top_k, 0.0)[0]
        G, T, _ = quotients(x, keep_k)
        for q in (float(np.float32(top_p)) - BAND, float(np.float32(top_p)) + BAND):
            out.append(keep_k & (G / T < q))
    return out


def cdf64_filtered(x, keep):
    p = np.where(keep, _mass64(x.astype(np.float64) - float(x.max())), 0.0)
    c = np.cumsum(p)
    return c / c[-1]


def draw64_filtered(logits32, reg32, T32, u, greedy, top_k, top_p):
    x = sc.x32(logits32, reg32, T32, greedy)
    if greedy:
        return int(np.argmax(x))
    return sc.pick(cdf64_filtered(x, filter64(x, top_k, top_p)[0]), u)


def allowed_filtered(x, top_k, top_p, u, idx):
    """an undecided row: class idx is kept by a membership the band allows and reaches within BAND of u under it"""
    for keep in memberships(x, top_k, top_p):
        if keep[idx] and keep.any() and sc.allowed_undecided(cdf64_filtered(x, keep), u, idx):
            return True
    return False


# ---------------------------------------------------------------- containers
class FPart(sc.Part):
    """the rows one launch takes: one regulariser (or none) and ONE filter (the run carries it)"""

    def __init__(self, C, reg, top_k, top_p):
        super().__init__(C, reg)
        self.top_k, self.top_p = int(top_k), float(np.float32(top_p))
        self.keeps, self.mdec, self.xs = [], [], []

    def base_of(self, logits, T, greedy=False):
        """registers a logits row with its temperature: filtered CDF, keep mask, membership verdict -> its index"""
        x = sc.x32(logits, self.reg, T, greedy)
        keep, dec = filter64(x, self.top_k, self.top_p)
        self.bases.append(cdf64_filtered(x, keep))
        self.keeps.append(keep)
        self.mdec.append(dec)
        self.xs.append(x)
        return len(self.bases) - 1

    def finish(self):
        super().finish()
        self.keep = np.stack(self.keeps) if self.keeps else None
        self.mdecided = np.array(self.mdec, dtype=bool)
        self.x = np.stack(self.xs) if self.xs else None
        del self.keeps, self.mdec, self.xs
        return self

    def decided(self):
        """per row: membership decided and the uniform off every CDF value, or a tie row"""
        tie = np.array([k in TIE_KINDS for k in self.kind])
        dist = np.abs(self.cdf[self.base] - self.u[:, None]).min(axis=1)
        return (self.greedy != 0) | (self.mdecided[self.base] & (tie | (dist > BAND)))      # (a greedy row never looks at the filter)


class Family:
    def __init__(self, name, kernel, C, parts):
        self.name, self.kernel, self.C = name, kernel, C
        self.parts = [p.finish() for p in parts if p.rows]
        self.n = sum(p.n for p in self.parts)


def _seed(name, kernel, C):
    return 7000 * (FAMILIES.index(name) + 1) + 10 * C + KERNELS.index(kernel)


# ---------------------------------------------------------------- level sets on the seams
def _level_sets(kernel, C, rs):
    """(A classes, B classes): B between A on both sides of a seam, B on the seam itself, the ends, and a scattered pair of sets"""
    out = []
    ok = lambda s: sorted({c for c in s if 0 <= c < C})  # noqa: E731
    for b in sc.seams(kernel, C):
        out.append((ok({b - 3, b - 1, b, b + 2}), ok({b - 2, b + 1, b + 3})))      # the seam between two kept classes, dropped ones around
        out.append((ok({b - 2, b + 1}), ok({b - 1, b})))                           # the seam between two dropped classes
    out.append(([0, 2, C - 1], [1, C - 2]))
    out.append(([1, C - 2], [0, C - 1]))
    n = min(64, C // 3)
    perm = rs.permutation(C)
    out.append((sorted(perm[:n].tolist()), sorted(perm[n:2 * n].tolist())))
    return [(a, b) for a, b in out if len(a) >= 2 and len(b) >= 2 and not set(a) & set(b)]


def _levels(C, A, B, Cc=()):
    x = np.full(C, -FAR, np.float32)
    x[list(A)] = np.float32(0)
    x[list(B)] = LOW
    if len(Cc):
        x[list(Cc)] = LOWER
    return x


def _tie_rows(part, x, T, tied, C):
    """survivors `tied`, all of mass 1: u = j / a and one ulp below, as sampler_cases' family b"""
    a = len(tied)
    base = part.base_of(x, T)
    js = range(a + 1) if a <= 8 else sorted({0, 1, a // 2, a - 1, a})
    for j in js:
        u = j / a
        part.add(x, T, u, 0, tied[j] if j < a else C - 1, "on", base)            # u = 1.0: the clamp
        if j > 0:
            part.add(x, T, math.nextafter(u, 0.0), 0, tied[j - 1], "under", base)


def _mid_rows(part, x, T, classes):
    base = part.base_of(x, T)
    cdf = part.bases[base]
    for i in classes:
        part.add(x, T, 0.5 * ((cdf[i - 1] if i else 0.0) + cdf[i]), 0, i, "mid", base)


def ratio(a, b, c=0):
    """a / T of the level rows in float64"""
    return a / (a + b * math.exp(float(LOW)) + c * math.exp(float(LOWER)))


# ---------------------------------------------------------------- f, g, h
def _family_f(kernel, C):
    rs = np.random.RandomState(_seed("f", kernel, C))
    parts = []
    for n, (A, B) in enumerate(_level_sets(kernel, C, rs)):
        part = FPart(C, None, len(A), 0.0)
        _tie_rows(part, _levels(C, A, B), (1.0, 0.5)[n % 2], A, C)                 # (0.5: an exact division; level B moves to -1.4 and is dropped all the same)
        parts.append(part)
    return Family("f", kernel, C, parts)


def _family_g(kernel, C):
    rs = np.random.RandomState(_seed("g", kernel, C))
    parts = []
    for A, B in _level_sets(kernel, C, rs):
        x = _levels(C, A, B)
        for k in sorted({1, len(A) - 1}):                                          # inside A: tau = 0, all of A stays
            part = FPart(C, None, k, 0.0)
            _tie_rows(part, x, 1.0, A, C)
            parts.append(part)
        for k in sorted({len(A) + 1, len(A) + len(B) - 1}):                        # inside B: tau = -0.7, A and B stay
            part = FPart(C, None, k, 0.0)
            _mid_rows(part, x, 1.0, sorted(A + B))
            parts.append(part)
    return Family("g", kernel, C, parts)


def _family_h(kernel, C):
    rs = np.random.RandomState(_seed("h", kernel, C))
    parts = []
    for A, B in _level_sets(kernel, C, rs):
        x = _levels(C, A, B)
        r = ratio(len(A), len(B))
        assert 0.06 < r < 0.94
        part = FPart(C, None, 0, r - 0.05)                                         # G_B / T = r >= top_p: B goes
        _tie_rows(part, x, 1.0, A, C)
        parts.append(part)
        part = FPart(C, None, 0, r + 0.05)                                         # r < top_p: B stays
        _mid_rows(part, x, 1.0, sorted(A + B))
        parts.append(part)
        # a third level that top_k drops: top_p between a / T(all) and a / T(survivors)
        free = [c for c in range(C) if c not in A and c not in B]
        Cc = sorted(rs.choice(free, min(len(free), 2 * len(A) + 4), replace=False).tolist())
        r_all, r_surv = ratio(len(A), len(B), len(Cc)), r
        if r_surv - r_all >= 0.12:
            part = FPart(C, None, len(A) + len(B), 0.5 * (r_all + r_surv))
            _tie_rows(part, _levels(C, A, B, Cc), 1.0, A, C)
            part.order_row = True
            parts.append(part)
    return Family("h", kernel, C, parts)


# ---------------------------------------------------------------- i: top_k = 1
def _family_i(kernel, C):
    rs = np.random.RandomState(_seed("i", kernel, C))
    parts = {T: FPart(C, None, 1, 0.0) for T in (1.0, 0.7)}
    sm = sc.seams(kernel, C)
    hot = sorted(set(sm) | {b - 1 for b in sm} | {0, C - 1}) + rs.randint(0, C, 8).tolist()
    for n, i in enumerate(hot):
        T = (1.0, 0.7)[n % 2]
        logits = (rs.standard_normal(C) * 3).astype(np.float32)
        logits[i] = np.float32(np.delete(logits, i).max()) + np.float32(0.25) + np.float32(rs.randint(0, 64)) / np.float32(64)
        base = parts[T].base_of(logits, T)
        for u in (0.0, 0.5, sc.ONE_BELOW):
            parts[T].add(logits, T, u, 0, i, "argmax", base)
    return Family("i", kernel, C, list(parts.values()))


# ---------------------------------------------------------------- j: the off values on family a
def _family_j(kernel, C):
    fa = sc.family("a", kernel, C)
    parts = []
    for top_k, top_p in ((0, 0.0), (C, 0.0), (C + 7, 0.0), (0, 1.0), (C, 1.0)):
        for src in fa.parts:
            part = FPart(C, src.reg, top_k, top_p)
            dist = np.abs(src.cdf[src.base] - src.u[:, None]).min(axis=1)
            bases = {}
            for r in np.nonzero(dist > BAND)[0][::3]:                              # (a third of the decided rows per off value: the launches stay small)
                b = int(src.base[r])
                if b not in bases:
                    bases[b] = part.base_of(src.logits[r], src.temp[r])
                part.add(src.logits[r], src.temp[r], src.u[r], 0, src.expect[r], "off", bases[b])
            parts.append(part)
    return Family("j", kernel, C, parts)


# ---------------------------------------------------------------- k: spread rows under real filters
K_RANDOM = 12


def _family_k(kernel, C):
    rs = np.random.RandomState(_seed("k", kernel, C))
    parts = []
    for top_k, top_p in K_FILTERS:
        if top_k >= C:
            top_k = C // 2
        for reg in (None, sc.regularizer(C)):
            part = FPart(C, reg, top_k, top_p)
            for s in (0.5, 1.0, 2.0, 4.0, 8.0):
                for T in (0.5, 1.0, 1.7):
                    logits = sc._out_of_denormals((rs.standard_normal(C) * s).astype(np.float32), reg, T)
                    base = part.base_of(logits, T)
                    cdf = part.bases[base]
                    mass = np.diff(cdf, prepend=0.0)
                    for u in rs.random_sample(K_RANDOM):
                        part.add(logits, T, u, 0, sc.pick(cdf, u), "random", base)
                    for i in np.nonzero(mass > 1e-5)[0]:
                        part.add(logits, T, 0.5 * ((cdf[i - 1] if i else 0.0) + cdf[i]), 0, i, "mid", base)
            parts.append(part)
    return Family("k", kernel, C, parts)


# ---------------------------------------------------------------- e: greedy rows with a filter set
def _family_e(kernel, C):
    fe = sc.family("e", kernel, C)
    parts = []
    for (top_k, top_p), src in zip(((5, 0.5), (1, 0.0)), fe.parts):
        part = FPart(C, src.reg, top_k, top_p)
        for r in range(src.n):
            base = part.base_of(src.logits[r], src.temp[r], greedy=True)
            part.add(src.logits[r], src.temp[r], src.u[r], 1, src.expect[r], "greedy", base)
        parts.append(part)
    return Family("e", kernel, C, parts)


_BUILD = {"f": _family_f, "g": _family_g, "h": _family_h, "i": _family_i, "j": _family_j, "k": _family_k, "e": _family_e}


@functools.lru_cache(maxsize=None)
def family(name, kernel, C):
    return _BUILD[name](kernel, C)

"""The cases of the kernel-level tests of the samplers' log-probability and forced forms (wn_sample_1w_lp<true, true>; wn_sample + the forced fork +
wn_sample_logp); numpy only, no GPU.  tests/test_logp_kernel_cases_host.py checks the cases themselves, tests/test_gpu_logp_kernels.py runs them through
the harness's kf_logp_* wrappers.

No statement of the contract is written here: a row's expectation is logprob_cases' -- kept64 for the membership, the log-softmax behind logp64 for the
value (Base.logp: the two halves of logp64, the first computed once per logits row; the host test holds it to logp64 itself) -- on sampler_cases' x32,
under sampler_filter_cases' filter64.  A row is (logits row, T, greedy flag, u, forced class); a part is the rows of one launch: one regulariser (or none)
and one filter.  The mode (logprob_cases.MODES) is the launch's, so a part runs in every mode of part.modes.

Families (fixed seeds; wn_sample_1w_lp at C = 256, the generic path at C = 256, 128, 100 and 40)
  P  positions, BIT EXACT.  Class j at 0.0, class i != j at -105 - i / 2: every fp32 mass but one is exactly 0 (x - max <= sampler_cases.UNDERFLOW - 1), the
     kept sum is 1.0f, logf(1.0f) = +0.0f, and the value of a forced class i is fl32(x_i - max) bit for bit -- a different number for every class, so a
     value read from another element, lane or chunk shows.  Every class is forced once per row; j sits on both sides of every seam (sampler_cases.seams),
     on class 0 and on the last class; sampled at T = 1 and at T = 0.5 (dyadic values: x / T is exact) and greedy.  A second part carries the regulariser and
     T = 0.7 and runs in model mode alone, which ignores both: fl32(l_i - max l).
  M  membership, exact -inf.  The level rows of sampler_filter_cases' families f, g and h under their own cuts (top_k between and inside the levels, top_p
     either side of the ratio, both together), dropped classes between kept ones across every seam: every class forced (a dropped one gives exactly -inf, a
     kept one a finite value within the bound), the clamp u = 1.0 (class C - 1, dropped or not), greedy rows (never -inf); in model mode everything is finite.
  U  underflowed but kept.  Three classes tied at -110 and two at -120 under a maximum of 0.0, around every seam; every other class has a real mass.  With
     the filters off they are kept (finite: fl32(x_i - max) - logf(sum)); any top_p drops them; top_k keeps a class iff fewer than k classes are strictly
     greater -- k on both sides of C - 5 (the -110 level, whose ties at the threshold all stay) and of C - 2 (the -120 level).
  S  spread rows: sampler_cases' family a under the six filters of sampler_filter_cases.K_FILTERS, free (the value is the returned class's) and forced to a
     uniformly drawn class, within logprob_cases.bound.  Rows whose membership filter64 cannot decide are left out: at most UNDECIDED_CAP of a family.
judge() is the one verdict on a launch's output, shared by the GPU module and by the host module's planted errors (planted())."""
import functools
import math

import numpy as np

import logprob_cases as lc
import sampler_cases as sc
import sampler_filter_cases as fc

KERNELS = sc.KERNELS
FAMILIES = ("P", "M", "U", "S")
MODES = lc.MODES
MODE_BITS = {"sampling": 1, "model": 2}        # r.logp & WN_RUN_LOGP_MASK: 1 + WN_LOGP_*
NEG_INF = np.uint32(0xFF800000)
UNDECIDED_CAP = fc.UNDECIDED_CAP
FREE = -1                                       # forced: a free position; cls: the draw's own class, known only from the kernel
U_HI, U_LO = np.float32(-110.0), np.float32(-120.0)
PLANTS = ("neighbour_element", "next_lane", "mass_membership")


def class_counts(kernel):
    return sc.class_counts(kernel)


def case_ids():
    return [(k, f, C) for k in KERNELS for f in FAMILIES for C in class_counts(k)]


def a_of(kernel, C):
    return lc.A_ONE_WAVE if kernel == "one_wave" else lc.a_generic(C)


def bits32(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- one logits row as one launch sees it
class Base:
    def __init__(self, logits, reg, T, greedy, top_k, top_p):
        self.logits, self.reg, self.T, self.greedy = np.asarray(logits, dtype=np.float32), reg, np.float32(T), bool(greedy)
        self.top_k, self.top_p = top_k, top_p
        self._kept, self._memo = None, {}

    def kept(self):
        """logprob_cases.kept64 of the row: (x, keep, membership decided)"""
        if self._kept is None:
            self._kept = lc.kept64(self.logits, self.reg, self.T, self.greedy, self.top_k, self.top_p)
        return self._kept

    def view(self, mode):
        """(v, keep) of logp64's two modes"""
        if mode == "model":
            return self.logits, np.ones(len(self.logits), bool)
        x, keep, _ = self.kept()
        return x, keep

    def decided(self, mode):
        return mode == "model" or self.kept()[2]

    def logp(self, idx, mode):
        """logprob_cases.logp64(..., idx, mode); the value depends on idx through v[idx] and keep[idx] alone"""
        v, keep = self.view(mode)
        key = (mode, float(v[idx]), bool(keep[idx]))
        if key not in self._memo:
            self._memo[key] = lc._logsoftmax_at(v, keep, int(idx))
        return self._memo[key]

    def exact32(self, idx, mode):
        """fl32(v_i - max v): the value of a row whose kept sum is 1.0f"""
        v, _ = self.view(mode)
        return np.float32(v[idx]) - np.float32(v.max())


class LPart:
    def __init__(self, C, reg, top_k, top_p, modes=MODES):
        self.C, self.reg, self.top_k, self.top_p, self.modes = C, reg, int(top_k), float(np.float32(top_p)), tuple(modes)
        self.bases, self.rows, self._exp = [], [], {}

    def base_of(self, logits, T, greedy=False):
        self.bases.append(Base(logits, self.reg, T, greedy, self.top_k, self.top_p))
        return len(self.bases) - 1

    def add(self, base, u, forced=FREE, cls=None, exact=False):
        """cls: the class the row returns (default: the forced one; FREE: the draw's own)"""
        self.rows.append((base, float(u), int(forced), int(forced if cls is None else cls), bool(exact)))

    def finish(self):
        r = self.rows
        self.n = len(r)
        self.base = np.array([q[0] for q in r], dtype=np.int64)
        self.u = np.array([q[1] for q in r], dtype=np.float64)
        self.forced = np.array([q[2] for q in r], dtype=np.int32)
        self.cls = np.array([q[3] for q in r], dtype=np.int32)
        self.exact = np.array([q[4] for q in r], dtype=bool)
        self.logits = np.ascontiguousarray(np.stack([b.logits for b in self.bases])[self.base])
        self.temp = np.array([b.T for b in self.bases], dtype=np.float32)[self.base]
        self.greedy = np.array([b.greedy for b in self.bases], dtype=np.int32)[self.base]
        del self.rows
        return self

    def expect(self, mode):
        """-> (logp64 per row, NaN on a free row; fl32(v_i - max v) per row; membership decided per row)"""
        if mode not in self._exp:
            want = np.full(self.n, np.nan)
            ex = np.zeros(self.n, np.float32)
            for r in np.nonzero(self.cls >= 0)[0]:
                b = self.bases[self.base[r]]
                want[r] = b.logp(self.cls[r], mode)
                if self.exact[r]:
                    ex[r] = b.exact32(self.cls[r], mode)
            dec = np.array([b.decided(mode) for b in self.bases], dtype=bool)[self.base]
            self._exp[mode] = (want, ex, dec)
        return self._exp[mode]


class Family:
    def __init__(self, name, kernel, C, parts):
        self.name, self.kernel, self.C = name, kernel, C
        self.parts = [p.finish() for p in parts if p.rows]
        self.n = sum(p.n for p in self.parts)


def _seed(name, kernel, C):
    return 9000 * (FAMILIES.index(name) + 1) + 10 * C + KERNELS.index(kernel)


def seam_classes(kernel, C):
    sm = sc.seams(kernel, C)
    return sorted(set(sm) | {b - 1 for b in sm} | {0, C - 1})


# ---------------------------------------------------------------- the verdict on one launch
def judge(part, mode, A, idx, bits):
    """idx: the indices the launch returned, bits: the uint32 words of its log-probabilities -> (failures, worst err / bound of the bounded rows)"""
    want, ex, dec = part.expect(mode)
    want = want.copy()
    idx = np.asarray(idx)
    fails = []
    known = part.cls >= 0
    for r in np.nonzero(known & (idx != part.cls))[0][:4]:
        fails.append("row %d: class %d returned, %d expected (forced %d, u %r)" % (r, idx[r], part.cls[r], part.forced[r], part.u[r]))
    for r in np.nonzero(~known)[0]:
        if not 0 <= idx[r] < part.C:
            fails.append("row %d: class %d is outside the classes" % (r, idx[r]))
            return fails, 0.0
        want[r] = part.bases[part.base[r]].logp(int(idx[r]), mode)
    if fails:
        return fails, 0.0
    got = np.asarray(bits, dtype=np.uint32).view(np.float32).astype(np.float64)
    inf = dec & np.isneginf(want)
    exact = dec & part.exact & ~inf
    bounded = dec & ~part.exact & ~inf
    for r in np.nonzero(inf & (bits != NEG_INF))[0][:4]:
        fails.append("row %d class %d: a dropped class must give -inf, got %r" % (r, idx[r], got[r]))
    for r in np.nonzero(exact & (bits != bits32(ex)))[0][:4]:
        fails.append("row %d class %d: %s for fl32(v_i - max v) = %s (%r)" % (r, idx[r], hex(int(bits[r])), hex(int(bits32(ex)[r])), float(ex[r])))
    worst = 0.0
    if bounded.any():
        bnd = np.array([lc.bound(w, part.C, A) for w in want[bounded]])
        with np.errstate(invalid="ignore"):
            err = np.abs(got[bounded] - want[bounded])
        bad = ~(np.isfinite(got[bounded]) & (err <= bnd))
        for r in np.nonzero(bounded)[0][bad][:4]:
            fails.append("row %d class %d: %r for %r, bound %.3g" % (r, idx[r], got[r], want[r], lc.bound(want[r], part.C, A)))
        ok = np.isfinite(err)
        worst = float((err[ok] / bnd[ok]).max()) if ok.any() else 0.0
    return fails, worst


def planted(part, mode, plant):
    """the (idx, bits) a kernel with one PLANTED error would return on the part's rows of known class: the float64 value rounded to fp32, from
    neighbour_element: the value of class idx ^ 1;  next_lane: the value of class idx + 4 (the next lane's element, lane 63 wrapping as a readlane's
    index does);  mass_membership: membership taken from `mass != 0` instead of the kept set"""
    out = np.zeros(part.n, np.float32)
    C = part.C
    for bi, b in enumerate(part.bases):
        rows = np.nonzero((part.base == bi) & (part.cls >= 0))[0]
        c = part.cls[rows].astype(np.int64)
        v, keep = b.view(mode)
        v64 = v.astype(np.float64)
        m = float(v64.max())
        mass = np.where(keep, fc._mass64(v64 - m), 0.0)
        src = {"neighbour_element": np.minimum(c ^ 1, C - 1), "next_lane": (c + 4) % C, "mass_membership": c}[plant]
        member = keep[c] if plant != "mass_membership" or mode == "model" or b.greedy else mass[c] != 0
        out[rows] = np.where(member, v64[src] - m - math.log(mass.sum()), -np.inf).astype(np.float32)
    return part.cls.copy(), out.view(np.uint32)


# ---------------------------------------------------------------- P: positions, bit exact
P_MODEL_T = 0.7


def p_logits(C, j):
    x = (np.float32(-105.0) - np.arange(C, dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    x[j] = np.float32(0.0)
    return x


def _family_p(kernel, C):
    sampling = LPart(C, None, 0, 0.0)                                      # (runs in model mode as well: the logits themselves are such a row)
    model = LPart(C, sc.regularizer(C), 0, 0.0, modes=("model",))
    ends = (0, C - 1)
    for n, j in enumerate(seam_classes(kernel, C)):
        x = p_logits(C, j)
        every = kernel == "one_wave" or j in ends                          # (the generic path's many seams take the three forms in turn)
        for v, (T, greedy) in enumerate(((1.0, False), (0.5, False), (0.5, True))):
            if every or n % 3 == v:
                b = sampling.base_of(x, T, greedy)
                for i in range(C):
                    sampling.add(b, 0.5, i, exact=True)
        for v, greedy in enumerate((False, True)):
            if every or n % 2 == v:
                b = model.base_of(x, P_MODEL_T, greedy)
                for i in range(C):
                    model.add(b, 0.5, i, exact=True)
    return Family("P", kernel, C, [sampling, model])


# ---------------------------------------------------------------- M: membership
M_SOURCES = ("f", "g", "h")


def _family_m(kernel, C):
    parts = []
    for name in M_SOURCES:
        for src in fc.family(name, kernel, C).parts:
            assert len(src.x) == 1
            r0 = int(np.nonzero(src.base == 0)[0][0])
            logits, T = src.logits[r0], src.temp[r0]
            part = LPart(C, None, src.top_k, src.top_p)
            part.source = name
            b = part.base_of(logits, T)
            for i in range(C):
                part.add(b, 0.5, i)
            part.add(b, 1.0, FREE, cls=C - 1)                                # the clamp
            g = part.base_of(logits, T, greedy=True)
            for i in sorted(set(np.nonzero(logits > -100)[0].tolist()) | {0, C - 1}):
                part.add(g, 0.0, i)
            parts.append(part)
    return Family("M", kernel, C, parts)


# ---------------------------------------------------------------- U: underflowed but kept
def u_filters(C):
    """(top_k, top_p): off in every spelling, top_p alone, top_k on both sides of the two counts (C - 5 above the -110 level, C - 2 above the -120 level), both"""
    return ((0, 0.0), (C, 0.0), (C + 7, 0.0), (0, 1.0), (0, 0.999), (0, 0.3), (C - 5, 0.0), (C - 4, 0.0), (C - 3, 0.0), (C - 2, 0.0), (C - 1, 0.0),
            (C - 4, 0.999), (C - 1, 0.3))


U_FORCE_ALL = 3          # every class is forced under these many of the filters, in turn over the placements; the underflowed and a few others under the rest


def u_placements(kernel, C):
    """(classes at -110, classes at -120): around every seam, and on the ends"""
    out = [([0, 2, C - 1], [1, C - 2])]
    for b in sc.seams(kernel, C):
        out.append((sorted({(b - 1) % C, b % C, (b + 2) % C}), sorted({(b - 2) % C, (b + 1) % C})))
    return out


def u_logits(C, hi, lo, rs):
    free = np.array([c for c in range(C) if c not in hi and c not in lo])
    pick = rs.permutation(free)
    x = np.full(C, fc.LOWER, np.float32)
    x[pick[:3]] = np.float32(0.0)
    x[pick[3:8]] = fc.LOW
    x[hi] = U_HI
    x[lo] = U_LO
    return x, pick[:8]


def _family_u(kernel, C):
    rs = np.random.RandomState(_seed("U", kernel, C))
    parts = []
    filters = u_filters(C)
    for n, (hi, lo) in enumerate(u_placements(kernel, C)):
        x, levels = u_logits(C, hi, lo, rs)
        few = sorted(set(hi) | set(lo) | set(levels[[0, 3, 7]].tolist()) | {int(rs.randint(C))})
        for f, (top_k, top_p) in enumerate(filters):
            part = LPart(C, None, top_k, top_p)
            part.hi, part.lo = hi, lo
            everything = (f + n) % len(filters) < U_FORCE_ALL or (n == 0 and top_k == C - 4)
            for T in (1.0, 0.5):
                b = part.base_of(x, T)
                for i in (range(C) if everything and T == 1.0 else few):
                    part.add(b, 0.5, i)
            g = part.base_of(x, 1.0, greedy=True)
            for i in hi + lo:
                part.add(g, 0.0, i)
            parts.append(part)
    return Family("U", kernel, C, parts)


# ---------------------------------------------------------------- S: spread rows
S_STRIDE = 16


def _family_s(kernel, C):
    rs = np.random.RandomState(_seed("S", kernel, C))
    fa = sc.family("a", kernel, C)
    parts = []
    for top_k, top_p in fc.K_FILTERS:
        if top_k >= C:
            top_k = C // 2
        for src in fa.parts:
            part = LPart(C, src.reg, top_k, top_p)
            other = [r for r in range(src.n) if src.kind[r] != "random"]
            bases = {}
            for r in sorted([r for r in range(src.n) if src.kind[r] == "random"] + other[::S_STRIDE]):
                sb = int(src.base[r])
                if sb not in bases:
                    bases[sb] = part.base_of(src.logits[r], src.temp[r])
                part.add(bases[sb], src.u[r])
                part.add(bases[sb], src.u[r], int(rs.randint(C)))
            parts.append(part)
    return Family("S", kernel, C, parts)


_BUILD = {"P": _family_p, "M": _family_m, "U": _family_u, "S": _family_s}


@functools.lru_cache(maxsize=None)
def family(name, kernel, C):
    return _BUILD[name](kernel, C)

"""The cases of tests/test_gpu_prime_kernels.py, the batched-priming kernels one at a time (csrc/wn_forward.h: wn_fwd_gemm_ragged, wn_fwd_gemm_taps_ragged,
wn_fwd_start_ragged, wn_fill_ring_at, wn_prime_gather_history): the row tables, the device helpers restated in Python (wn_ragged_find, wn_ragged_row,
wn_ring_slot, wn_prime_hist_time) with the wrong variants a test must tell from them, the float64 or bit references and the expected images.  No torch,
no engine; tests/test_prime_kernel_cases_host.py checks all of it without a GPU.

A row table is rows per stream and t_end = n; start = the prefix sums.  Row m belongs to the LAST stream s with start[s] <= m and stands for the time
n - rows_s + (m - start[s]) of that stream.  Every matrix of a case is addressed by (stream, time): a Layout of [streams][pre + n + gap][cols + pad] words
whose time 0 is the physical row `pre`.  Inputs hold NaN in every row the kernel must not read, outputs the sentinel in every word it must not write."""
import numpy as np

import ragged_cases as rc

GATE_ABS = 1e-6                   # kernel_lib.GATE_ABS (the host test holds them equal)
SENSITIVE = 1000 * GATE_ABS       # what a wrong mapping must move some output by (the threshold of _taps_case, tests/test_gpu_infer_kernels.py)
SENT32 = np.uint32(0x7FC0DEAD)    # kernel_lib.SENT32
NAN32 = np.uint32(0x7FC00000)
PLAIN, GATE = 0, 1                # WN_EPI_PLAIN, WN_EPI_GATE
TILE = 128


# ---------------------------------------------------------------- row tables
class Table:
    def __init__(self, name, rows, n):
        self.name, self.rows, self.n, self.ns = name, [int(r) for r in rows], int(n), len(rows)
        self.start = [0] + [int(v) for v in np.cumsum(self.rows, dtype=np.int64)]
        self.M = self.start[-1]
        assert all(0 <= r <= n for r in self.rows) and self.M >= 1

    def first_time(self, s):
        return self.n - self.rows[s]


_MINI3 = rc.plan(rc.MINI3_DIL, 2, rc.MINI3_LENGTHS)
PLAN_LAYER = 0   # table 1 + 0 of MINI3: need[1] = 14 < the lengths 127 .. 300, the rows of a stream are fewer than its samples
TABLES = {t.name: t for t in (
    Table("a", [1], 1),                                                  # a search with no iteration, M = 1
    Table("b", rc.MINI3_LENGTHS, 300),                                    # M = 696: seams inside tiles, a stream of exactly one tile
    Table("brev", rc.MINI3_LENGTHS[::-1], 300),
    Table("c", [0, 0, 3, 0, 0, 0, 130, 0], 130),                          # empty runs at the front, in the middle, at the end; a last tile of 5 rows
    Table("d", [64, 64, 128], 128),                                       # seams exactly on tile boundaries, M = 256
    Table("e", [[1, 0, 2][i % 3] for i in range(171)], 2),                # not a power of two; 128 rows of 86 streams in one tile
    Table("plan", _MINI3["rows"][1 + PLAN_LAYER], _MINI3["n"]),           # the engine's own: trailing min(need, length) rows
)}


# ---------------------------------------------------------------- the device helpers restated, and their wrong variants
# the variants of the row map (section "Mutants" of the host test: 1 .. 4), by name
MAP_MUTANTS = ["first stream", "strict <", "left-aligned", "time - 1", "time + 1"]


def ragged_find(start, ns, m, mutant=None):
    """wn_ragged_find, line by line -> (stream, its first row, its row count)"""
    if mutant == "first stream":
        lo = min(i for i in range(ns) if start[i] <= m)
    else:
        lo, hi = 0, ns
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if (start[mid] < m) if mutant == "strict <" else (start[mid] <= m):
                lo = mid
            else:
                hi = mid
    return lo, start[lo], start[lo + 1] - start[lo]


def ragged_row(tab, m, mutant=None):
    """wn_ragged_row -> (stream, time)"""
    s, first, rows = ragged_find(tab.start, tab.ns, m, mutant)
    t = tab.n - rows + (m - first)
    if mutant == "left-aligned":
        t = m - first
    return s, t + {"time - 1": -1, "time + 1": 1}.get(mutant, 0)


_MAPS = {}


def row_map(tab, mutant=None):
    """(stream [M], time [M]) of a table's rows under wn_ragged_row or a variant of it"""
    if (tab.name, mutant) not in _MAPS:
        st = [ragged_row(tab, m, mutant) for m in range(tab.M)]
        _MAPS[tab.name, mutant] = (np.array([v[0] for v in st], np.int64), np.array([v[1] for v in st], np.int64))
    return _MAPS[tab.name, mutant]


def contract_map(tab):
    """the same from the contract's own words (ragged_cases.find: the LAST stream whose start is <= m)"""
    s = np.array([rc.find(tab.start, m)[0] for m in range(tab.M)], np.int64)
    first, rows = np.asarray(tab.start)[s], np.asarray(tab.rows)[s]
    return s, tab.n - rows + (np.arange(tab.M) - first)


def division_map(tab):
    """mutant 5: the epilogue's (q, rem) by division, rows_per_batch = M as wn_prime_pass sets it"""
    m = np.arange(tab.M, dtype=np.int64)
    return m // tab.M, m % tab.M


def ring_slot(t, ML, mutant=None):
    """wn_ring_slot for Python integers of any size; 'c %': the remainder of C, which takes the sign of t"""
    if mutant == "c %":
        return -((-t) % ML) if t < 0 else t % ML
    return t % ML


def hist_time(n, n_append, j, Lp, mutant=None):
    """wn_prime_hist_time -> the pass time of history row j, or None: dropped"""
    t = (n - n_append) - j
    return None if (t < -Lp and mutant != "no drop") else t


# ---------------------------------------------------------------- layouts and images
class Layout:
    def __init__(self, ns, n, cols, pre, gap=3, pad=8):
        self.ns, self.n, self.cols, self.pre, self.T, self.ld = ns, n, cols, pre, pre + n + gap, cols + pad

    def full(self, word):
        return np.full((self.ns, self.T, self.ld), word, np.uint32)

    def inside(self, s, t):
        return (s >= 0) & (s < self.ns) & (t + self.pre >= 0) & (t + self.pre < self.T)

    def map(self, ptr):
        """the row map (base at time 0 of stream 0, batch_stride, row_stride, t0 = 0) of the image uploaded at `ptr`"""
        return (ptr + 4 * self.pre * self.ld, self.T * self.ld, self.ld, 0)

    def put(self, img, s, t, vals32):
        img[s, t + self.pre, :self.cols] = np.ascontiguousarray(vals32, np.float32).view(np.uint32)

    def take64(self, img, s, t):
        """the float64 rows (s, t) of an input image; a row outside the image reads as NaN"""
        out = np.full((len(s), self.cols), np.nan)
        ok = self.inside(s, t)
        out[ok] = img[s[ok], t[ok] + self.pre, :self.cols].view(np.float32).astype(np.float64)
        return out

    def written(self, s, t, vals):
        """(float64 image with NaN where nothing is written, rows that leave the image)"""
        img = np.full((self.ns, self.T, self.ld), np.nan)
        ok = self.inside(s, t)
        img[s[ok], t[ok] + self.pre, :self.cols] = vals[ok]
        return img, int((~ok).sum())


def gate64(v, N):
    """kernel_lib._gate64: columns [F(32) | G(32)] per 64 -> (z, tanh, sigmoid)"""
    F = np.concatenate([v[:, 64 * j:64 * j + 32] for j in range(N // 64)], axis=1)
    G = np.concatenate([v[:, 64 * j + 32:64 * j + 64] for j in range(N // 64)], axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        th, sg = np.tanh(F), 1 / (1 + np.exp(-G))
    return th * sg, th, sg


def _dyadic(rs, shape, nonzero=False):
    v = rs.randint(1, 17, shape) * rs.choice([-1, 1], shape) if nonzero else rs.randint(-16, 17, shape)
    return v.astype(np.float32) / 64


# ---------------------------------------------------------------- the products
class Product:
    """One ragged product.  kind 'gate2': z = gate([x(t - d) | x(t)] . W^T + b) (wn_layer_fg, kernel_size 2; the d rows in front of a stream's first row
    hold the append form's history, finite and non-zero, which the kernel reads without a predicate); 'taps': the same of kernel_size taps = 3 / 4 with
    t_min = -Lp, Lp = d + 1: the rows [-Lp, n) in reach of a stream's taps are finite, a tap below -Lp reads as zero; 'plain': x' = z . W^T + b + x(t)
    (wn_layer_res; small integers, exact).  `data`: 'exact' (dyadic / integers) or 'normal' (standard_normal: the same-bits-as-the-rectangle family)."""

    def __init__(self, kind, tab, K1, N, d=0, taps=2, bias=True, seed=0, data="exact"):
        self.kind, self.tab, self.K1, self.N, self.d, self.taps, self.bias, self.seed = kind, tab, K1, N, d, taps, bias, seed
        rs = np.random.RandomState(seed)
        ns, n = tab.ns, tab.n
        self.epi = PLAIN if kind == "plain" else GATE
        self.K = K1 * (1 if kind == "plain" else taps)
        self.ncols = N if kind == "plain" else N // 2
        self.s, self.t = contract_map(tab)
        k1 = taps - 1
        self.Lp = d + 1 if kind == "taps" else k1 * d
        self.t_min = -self.Lp
        self.reach = k1 * d
        normal = data == "normal"
        if kind == "plain":
            assert self.K * 16 < 2 ** 24
            self.xl = Layout(ns, n, K1, pre=2)
            vals = rs.standard_normal((ns, self.xl.T, K1)).astype(np.float32) if normal else rs.randint(-4, 5, (ns, self.xl.T, K1)).astype(np.float32)
            self.W = rs.standard_normal((N, self.K)).astype(np.float32) if normal else rs.randint(-4, 5, (N, self.K)).astype(np.float32)
            self.cl = Layout(ns, n, N, pre=1, gap=2, pad=4)
            cv = rs.standard_normal((ns, self.cl.T, N)).astype(np.float32) if normal else rs.randint(-64, 65, (ns, self.cl.T, N)).astype(np.float32)
            self.cin = self.cl.full(NAN32)
        else:
            assert self.K * 256 < 2 ** 24   # integers / 64: every product and partial sum is an exact multiple of 2^-12 below 2^12
            self.xl = Layout(ns, n, K1, pre=self.reach + 2)
            vals = rs.standard_normal((ns, self.xl.T, K1)).astype(np.float32) if normal else _dyadic(rs, (ns, self.xl.T, K1))
            hist = rs.standard_normal((ns, self.xl.T, K1)).astype(np.float32) if normal else _dyadic(rs, (ns, self.xl.T, K1), nonzero=True)
            self.W = rs.standard_normal((N, self.K)).astype(np.float32) if normal else _dyadic(rs, (N, self.K))
        self.x = self.xl.full(NAN32)
        tau = np.arange(self.xl.T) - self.xl.pre
        for s in range(ns):
            if tab.rows[s] == 0:
                continue   # a stream without rows: nothing of it may be read
            f = tab.first_time(s)
            own = (tau >= f) & (tau < n)
            self.x[s, own, :K1] = vals[s, own].view(np.uint32)
            if kind == "plain":
                ownc = (np.arange(self.cl.T) - self.cl.pre >= f) & (np.arange(self.cl.T) - self.cl.pre < n)
                self.cin[s, ownc, :N] = cv[s, ownc].view(np.uint32)
            else:
                before = (tau >= max(f - self.reach, self.t_min)) & (tau < f)
                self.x[s, before, :K1] = hist[s, before].view(np.uint32)
        if bias:
            self.bvec = rs.standard_normal(N).astype(np.float32) if normal else (rs.randint(-8, 9, N) / (1.0 if kind == "plain" else 64.0)).astype(np.float32)
        else:
            self.bvec = None
        self.ol = Layout(ns, n, self.ncols, pre=4, gap=5)
        self.W64 = self.W.astype(np.float64)
        self.ref = None if normal else self.values(self.s, self.t)
        self.tag = "%s table %s K1 %d N %d d %d taps %d bias %d" % (kind, tab.name, K1, N, d, taps, int(bias))

    # ---- the reference
    def views(self, s, t):
        """the float64 A operand as its views, oldest first: what the loaders read for the rows (s, t); a row that must not be read is NaN"""
        if self.kind == "plain":
            return [self.xl.take64(self.x, s, t)]
        out = []
        for j in range(self.taps):
            tj = t - (self.taps - 1 - j) * self.d
            v = self.xl.take64(self.x, s, tj)
            if self.kind == "taps":
                v[tj < self.t_min] = 0.0
            out.append(v)
        return out

    def of_views(self, views, s, t, cin=True):
        with np.errstate(invalid="ignore"):
            acc = sum(v @ self.W64[:, j * self.K1:(j + 1) * self.K1].T for j, v in enumerate(views))
        if self.bvec is not None:
            acc = acc + self.bvec.astype(np.float64)
        if self.kind == "plain":
            return acc + self.cl.take64(self.cin, s, t) if cin else acc
        return gate64(acc, self.N)[0]

    def values(self, s, t):
        return self.of_views(self.views(s, t), s, t)

    def ref32(self):
        """PLAIN: the exact result as fp32"""
        v32 = self.ref.astype(np.float32)
        assert np.array_equal(v32.astype(np.float64), self.ref), "case leaves the exact range"
        return v32

    def expect_plain(self):
        e = self.ol.full(SENT32)
        self.ol.put(e, self.s, self.t, self.ref32())
        return e

    # ---- what the data can tell
    def wrong_views(self):
        """name -> (values of a product that maps its rows right and forms its operand wrong, the rows whose operand it changes)"""
        v = self.views(self.s, self.t)
        every = np.ones(self.tab.M, bool)
        if self.kind == "plain":
            return {"cin dropped": (self.of_views(v, self.s, self.t, cin=False), every)}
        out = {"views reversed": (self.of_views(v[::-1], self.s, self.t), every)}
        for j in range(self.taps):   # (a tap below t_min is zero already)
            out["view %d zeroed" % j] = (self.of_views(v[:j] + [np.zeros_like(v[j])] + v[j + 1:], self.s, self.t), (v[j] != 0).any(axis=1))
        return out

    def check_sensitive(self):
        """each wrong mapping moves some output by >= SENSITIVE in every 128-row tile it touches; raises AssertionError"""
        assert not np.isnan(self.ref).any()
        for name, (w, touched) in self.wrong_views().items():
            self._moved(name, np.abs(w - self.ref).max(axis=1), touched)
        for mu in MAP_MUTANTS:
            s, t = row_map(self.tab, mu)
            with np.errstate(invalid="ignore"):
                dz = np.abs(self.values(s, t) - self.ref)
            dz[np.isnan(dz)] = np.inf   # (a NaN row was read)
            self._moved(mu, dz.max(axis=1), (s != self.s) | (t != self.t))

    def _moved(self, name, dz, touched):
        for r0 in range(0, self.tab.M, TILE):
            sl = slice(r0, r0 + TILE)
            if touched[sl].any():
                assert dz[sl][touched[sl]].max() >= SENSITIVE, "%s: the data cannot tell '%s' in the tile at row %d" % (self.tag, name, r0)

    def tells(self, mutant):
        """does this case's expected output differ from the mutant's -- in where it is written, or by >= SENSITIVE (PLAIN: at all) in a value"""
        if mutant == "division":
            rs_, rt = self.s, self.t
            ws, wt = division_map(self.tab)
        else:
            rs_, rt = row_map(self.tab, mutant)
            ws, wt = rs_, rt
        want, esc0 = self.ol.written(self.s, self.t, self.ref)
        got, esc = self.ol.written(ws, wt, self.values(rs_, rt))
        assert esc0 == 0
        if esc or not np.array_equal(np.isnan(want), np.isnan(got)):
            return True
        on = ~np.isnan(want)
        with np.errstate(invalid="ignore"):
            dv = np.abs(got[on] - want[on])
        return bool(np.isnan(dv).any() or (dv >= SENSITIVE).any() if self.epi == GATE else (dv != 0).any())


GATE2_R, GATE2_N, GATE2_D = [32, 128], [64, 192, 256], [1, 7, "big"]      # 4 / 16 K chunks of 16: the view switch on either LDS buffer; d big = n + 3
PLAIN_K, PLAIN_N = [32, 128], [32, 96, 160]
TAPS_R, TAPS_N, TAPS_D = [32, 96], [64, 192], [1, 7]
TABLE_IDS = sorted(TABLES)


def product_cases(pairwise):
    """[(id, kind, constructor arguments)]: tables by shapes, every pair of values of two factors in some case (kernel_lib._pairwise)"""
    out = []
    for ti, ri, ni, di, bi in pairwise([len(TABLE_IDS), len(GATE2_R), len(GATE2_N), len(GATE2_D), 2], seed=21):
        tab = TABLES[TABLE_IDS[ti]]
        d = tab.n + 3 if GATE2_D[di] == "big" else GATE2_D[di]
        out.append(("gate-%s-R%d-N%d-d%s-b%d" % (tab.name, GATE2_R[ri], GATE2_N[ni], GATE2_D[di], bi), "gate2",
                    dict(kind="gate2", tab=tab, K1=GATE2_R[ri], N=GATE2_N[ni], d=d, taps=2, bias=bool(bi), seed=100 + len(out))))
    for ti, ki, ni, bi in pairwise([len(TABLE_IDS), len(PLAIN_K), len(PLAIN_N), 2], seed=22):
        tab = TABLES[TABLE_IDS[ti]]
        out.append(("plain-%s-K%d-N%d-b%d" % (tab.name, PLAIN_K[ki], PLAIN_N[ni], bi), "plain",
                    dict(kind="plain", tab=tab, K1=PLAIN_K[ki], N=PLAIN_N[ni], bias=bool(bi), seed=200 + len(out))))
    for taps in (3, 4):
        for ti, ri, ni, di, bi in pairwise([len(TABLE_IDS), len(TAPS_R), len(TAPS_N), len(TAPS_D), 2], seed=20 + taps):
            tab = TABLES[TABLE_IDS[ti]]
            out.append(("k%d-%s-R%d-N%d-d%d-b%d" % (taps, tab.name, TAPS_R[ri], TAPS_N[ni], TAPS_D[di], bi), "taps%d" % taps,
                        dict(kind="taps", tab=tab, K1=TAPS_R[ri], N=TAPS_N[ni], d=TAPS_D[di], taps=taps, bias=bool(bi), seed=300 + len(out))))
    return out


_BUILT = {}


def product(cid, kw):
    """a case is built once per process"""
    if cid not in _BUILT:
        _BUILT[cid] = Product(**kw)
    return _BUILT[cid]


# ---------------------------------------------------------------- wn_fwd_start_ragged
def start_values(shape, bias_j, rs):
    """(start, final): final = start + bias in fp32 exactly, final on, just below and just above bf16 rounding points (bias_j / 128 per channel);
    wn_fwd_start's cases (tests/test_gpu_infer_kernels.py) take their values here too"""
    b = rs.randint(136, 248, shape).astype(np.float64)
    f = rs.choice([0.5 - 2.0 ** -16, 0.5, 0.5 + 2.0 ** -16, 0.25, 0.75, 0.0], shape)
    sgn = rs.choice([-1.0, 1.0], shape)
    final = sgn * (b + f) / 128
    start = final - bias_j / 128
    assert np.array_equal(start.astype(np.float32).astype(np.float64), start)
    return start.astype(np.float32), final.astype(np.float32)


PAD_CLASS = 255   # the class behind a stream's length: its column of start_t is NaN


class StartCase:
    """x(s, n - n_s + j) = start_t[idx[s][j]] (+ bias) for j < n_s; idx rows idx_stride apart, the pad behind a length = PAD_CLASS"""

    def __init__(self, tab, R, bias, seed=0):
        rs = np.random.RandomState(seed)
        self.tab, self.R = tab, R
        bj = rs.randint(0, 8, R).astype(np.float64) if bias else np.zeros(R)
        self.start_t, self.final = start_values((256, R), bj, rs)
        self.bvec = (bj / 128).astype(np.float32) if bias else None
        assert np.array_equal(self.start_t + (bj / 128).astype(np.float32), self.final)
        self.start_t[PAD_CLASS] = np.nan
        self.final[PAD_CLASS] = np.nan
        self.idx_stride = max(tab.rows) + 3
        self.idx = np.full((tab.ns, self.idx_stride), PAD_CLASS, np.int32)
        for s, r in enumerate(tab.rows):
            self.idx[s, :r] = rs.randint(0, PAD_CLASS, r)
        self.xl = Layout(tab.ns, tab.n, R, pre=2, gap=3, pad=0)   # x_stream_stride = (2 + n + 3) R > n R
        self.s, self.t = contract_map(tab)
        self.tag = "start table %s R %d bias %d" % (tab.name, R, int(bias))

    def values(self, s, j, mutant=None):
        """the rows the gather writes for sample j of stream s; a class read outside idx is the pad's NaN"""
        flat = self.idx.ravel()
        at = self.tab_first(s) + j if mutant == "no idx_stride" else s * self.idx_stride + j
        ok = (at >= 0) & (at < flat.size)
        cls = np.full(len(at), PAD_CLASS, np.int64)
        cls[ok] = flat[at[ok]]
        return self.final[cls]

    def tab_first(self, s):
        return np.asarray(self.tab.start)[s]

    def image(self, mutant=None):
        """(expected x as words, rows that leave the image) under the contract or a variant"""
        if mutant in MAP_MUTANTS:
            s, t = row_map(self.tab, mutant)
            first = np.array([ragged_find(self.tab.start, self.tab.ns, m, mutant)[1] for m in range(self.tab.M)], np.int64)
        else:
            s, t = self.s, self.t
            first = self.tab_first(s)
        j = np.arange(self.tab.M) - first
        vals = self.values(s, j, mutant)
        ok = self.xl.inside(s, t)
        e = self.xl.full(SENT32)
        self.xl.put(e, s[ok], t[ok], vals[ok])
        return e, int((~ok).sum())


START_TABLES, START_R = ["a", "c", "e"], [32, 96]


def start_cases():
    return [("%s-R%d-%s" % (t, R, "bias" if b else "nobias"), dict(tab=TABLES[t], R=R, bias=bool(b), seed=7 * R + b + len(t))) for t in START_TABLES for R in START_R
            for b in (0, 1)]


# ---------------------------------------------------------------- wn_fill_ring_at
FILL_ML = [2, 3, 17]
FILL_SHAPES = [(1, 1, 32), (2, 3, 96)]   # (P, streams, R)
T62 = 2 ** 62


def fill_times(ML):
    return sorted({1, ML - 1, ML, 2 * ML + 2})


def fill_bases(ML, n_time):
    return sorted({0, 1, ML - 1, ML, 37, 2 ** 40 + 5, T62 - n_time - 1})


class FillCase:
    """count = ML rows of every stream, the pass times [n_time - ML, n_time) -- the negative ones the gathered history --, to slot (t_base + t) mod ML of all
    P copies.  shared: x_batch_stride = 0, all streams take stream 0's rows."""

    def __init__(self, ML, n_time, t_base, P, ns, R, shared, seed=0):
        rs = np.random.RandomState(seed)
        self.ML, self.n_time, self.t_base, self.P, self.ns, self.R, self.shared = ML, n_time, t_base, P, ns, R, shared
        self.xl = Layout(1 if shared else ns, n_time, R, pre=ML + 2, gap=3, pad=0)
        self.X = rs.standard_normal((self.xl.ns, self.xl.T, R)).astype(np.float32)
        self.x = self.xl.full(NAN32)
        lo = self.xl.pre + n_time - ML
        self.x[:, lo:lo + ML] = self.X[:, lo:lo + ML].view(np.uint32)
        self.tag = "fill_ring_at ML %d n_time %d t_base %d P %d streams %d R %d shared %d" % (ML, n_time, t_base, P, ns, R, int(shared))

    def slots(self, mutant=None):
        """pass time -> ring slot; None: outside the ring"""
        out = {}
        for t in range(self.n_time - self.ML, self.n_time):
            q = t if mutant == "no t_base" else self.t_base + t
            sl = ring_slot(q, self.ML, mutant)
            out[t] = sl if 0 <= sl < self.ML else None
        return out

    def image(self, mutant=None, ring=None):
        """(the ring [P][streams][ML][R] as words after the fill -- from `ring` or the sentinel --, rows that leave it)"""
        e = np.full((self.P, self.ns, self.ML, self.R), SENT32, np.uint32) if ring is None else ring.copy()
        esc = 0
        for t, sl in self.slots(mutant).items():   # (ascending t: a later row of a wrong variant overwrites an earlier one)
            if sl is None:
                esc += 1
                continue
            for s in range(self.ns):
                e[:, s, sl] = self.X[0 if self.shared else s, self.xl.pre + t].view(np.uint32)[None]
        return e, esc


def fill_cases(ML, P, ns, R, shared):
    """every (n_time, t_base) of one ring shape"""
    return [FillCase(ML, n_time, t_base, P, ns, R, shared, seed=ML + n_time + R) for n_time in fill_times(ML) for t_base in fill_bases(ML, n_time)]


# ---------------------------------------------------------------- wn_prime_gather_history
GATHER_ML = [2, 3, 17]
GATHER_N = 5


def gather_bases(ML, n):
    return sorted({0, 1, ML - 1, ML, 2 ** 40 + 5, T62 - n - 1})


def gather_tables(n):
    """name -> n_append per stream (None: the rectangle form, start == NULL): 0 and n among them"""
    return {"null": None, "mixed": [0, n, 1, n - 1], "front0": [0, 0, n], "alln": [n, n]}


class GatherCase:
    """The ring [2][streams + 1][ML][R] holds values in copy 0 of the first `streams` streams and NaN elsewhere.  History row j = 1 .. ML of stream s, slot
    (t_base - j) mod ML, goes to the pass time (n - n_append[s]) - j of x; below -Lp it is dropped.  x: [streams][guard + Lp + n + gap][R] of sentinels."""

    def __init__(self, ML, Lp, n, t_base, n_append, ns, R, seed=0):
        rs = np.random.RandomState(seed)
        self.ML, self.Lp, self.n, self.t_base, self.R = ML, Lp, n, t_base, R
        self.n_append = None if n_append is None else list(n_append)
        self.ns = ns if n_append is None else len(n_append)
        self.start = None if n_append is None else np.asarray([0] + list(np.cumsum(n_append)), np.int32)
        self.ns_total = self.ns + 1
        self.V = rs.standard_normal((self.ns, ML, R)).astype(np.float32)
        self.ring = np.full((2, self.ns_total, ML, R), NAN32, np.uint32)
        self.ring[0, :self.ns] = self.V.view(np.uint32)
        self.guard = 3
        self.xl = Layout(self.ns, n, R, pre=Lp + self.guard, gap=2, pad=0)
        self.tag = "gather ML %d Lp %d n %d t_base %d n_append %s R %d" % (ML, Lp, n, t_base, self.n_append, R)

    def appended(self, s, mutant=None):
        if self.n_append is None:
            return self.n
        return int(self.start[s]) if mutant == "n_append = start[s]" else self.n_append[s]

    def image(self, mutant=None, x=None):
        """(x as words after the gather -- from `x` or the sentinel --, rows that leave the image or the ring, rows dropped)"""
        e = self.xl.full(SENT32) if x is None else x.copy()
        esc = dropped = 0
        for s in range(self.ns):
            for j in range(1, self.ML + 1):
                t = hist_time(self.n, self.appended(s, mutant), j, self.Lp, mutant)
                if t is None:
                    dropped += 1
                    continue
                q = {"slot + 1": self.t_base - j + 1, "slot t_base + j": self.t_base + j}.get(mutant, self.t_base - j)
                sl = ring_slot(q, self.ML, mutant)
                if not (0 <= sl < self.ML) or not self.xl.inside(np.array([s]), np.array([t]))[0]:
                    esc += 1
                    continue
                e[s, self.xl.pre + t, :self.R] = self.V[s, sl].view(np.uint32)
        return e, esc, dropped


def gather_cases(ML, R):
    """every (Lp, table, t_base) of one ring length: at Lp = ML - 1 the row j = ML of a stream that appends all n rows is dropped"""
    n = GATHER_N
    return [GatherCase(ML, Lp, n, t_base, n_append, 3, R, seed=ML + Lp + R) for Lp in (ML - 1, ML + 3) for _, n_append in sorted(gather_tables(n).items(), key=lambda kv: kv[0])
            for t_base in gather_bases(ML, n)]


# ---------------------------------------------------------------- the mutants of the host test
PRODUCT_KINDS = ("gate2", "plain", "taps3", "taps4")   # wn_fwd_gemm_ragged<GATE>, <PLAIN>, wn_fwd_gemm_taps_ragged<3>, <4>
MUTANTS = [   # (number in the host test's list, name, the kernels it concerns)
    ("1", "first stream", PRODUCT_KINDS + ("start",)),
    ("2", "strict <", PRODUCT_KINDS + ("start",)),
    ("3", "left-aligned", PRODUCT_KINDS + ("start",)),
    ("4a", "time - 1", PRODUCT_KINDS + ("start",)),
    ("4b", "time + 1", PRODUCT_KINDS + ("start",)),
    ("5", "division", PRODUCT_KINDS),
    ("6", "c %", ("fill", "gather")),
    ("7", "no t_base", ("fill",)),
    ("8", "slot + 1", ("gather",)),
    ("9", "slot t_base + j", ("gather",)),
    ("10", "no drop", ("gather",)),
    ("11", "n_append = start[s]", ("gather",)),
    ("12", "no idx_stride", ("start",)),
]

"""The cases of the batched-priming kernel tests (tests/prime_kernel_cases.py), checked without a GPU: the references agree with the project's own
restatements (ragged_cases.find / plan, append_cases.ring_slot / hist_time, and wn_ring_slot / wn_prime_hist_time written out as C computes them); every
case stays in the exact range; the data is sensitive (each wrong mapping moves some output by >= 1000 GATE_ABS in every 128-row tile it touches); and
the case data tells every mutant below from the contract.  A mutant is a wrong variant of the Python restatement -- never an altered kernel, whose
addresses could leave the test's allocations: its expected output must differ from the contract's for at least one case of a kernel it concerns.

   1  find the first stream with start <= m instead of the last          7  t_base ignored in the fill
   2  start[mid] < m in the search                                       8  the gather reads slot t_base - j + 1
   3  left-aligned time (m - first, without t_end - rows)                9  the gather reads slot t_base + j
   4  time off by one, either way                                       10  the drop at -Lp missing
   5  the epilogue's (q, rem) by division instead of the row map        11  n_append read from start[s] alone
   6  % of C instead of wn_ring_slot                                    12  the start gather indexes idx without idx_stride
"""
import numpy as np
import pytest

import append_cases as ac
import prime_kernel_cases as pk
import ragged_cases as rc
from kernel_lib import GATE_ABS, SENT32, _gate64, _pairwise

PRODUCTS = pk.product_cases(_pairwise)
FILL_SHAPES = [(ML, P, ns, R, sh) for ML in pk.FILL_ML for P, ns, R in pk.FILL_SHAPES for sh in (False, True)]


def test_constants():
    assert pk.GATE_ABS == GATE_ABS and pk.SENSITIVE == 1000 * GATE_ABS and pk.SENT32 == SENT32
    v = np.random.RandomState(0).standard_normal((5, 192))
    for a, b in zip(pk.gate64(v, 192), _gate64(v, 192)):
        assert np.array_equal(a, b)


def test_tables():
    T = pk.TABLES
    assert T["a"].M == 1 and T["a"].ns == 1
    assert T["b"].M == 696 and 128 in T["b"].rows and T["brev"].start != T["b"].start
    assert any(s % 128 for s in T["b"].start[1:-1]), "no seam inside a tile"
    assert T["c"].rows[:2] == [0, 0] and T["c"].rows[3:6] == [0, 0, 0] and T["c"].rows[-1] == 0 and T["c"].M % 128 == 5
    assert T["d"].M == 256 and all(s % 64 == 0 for s in T["d"].start) and 128 in T["d"].start
    e = T["e"]
    assert e.ns == 171 and e.ns & (e.ns - 1) and len(set(pk.contract_map(e)[0][:128])) == 86
    p = rc.plan(rc.MINI3_DIL, 2, rc.MINI3_LENGTHS)
    assert T["plan"].start == p["start"][1 + pk.PLAN_LAYER] and T["plan"].n == p["n"]
    assert any(r < length for r, length in zip(T["plan"].rows, rc.MINI3_LENGTHS)), "no stream with fewer rows than samples"
    used = {kw["tab"].name for _, _, kw in PRODUCTS}
    assert used == set(T), "a table without a product case"


@pytest.mark.parametrize("name", sorted(pk.TABLES))
def test_row_map(name):
    """the binary search restated from wn_ragged_find gives ragged_cases.find's stream, and the time lies inside the stream's rows"""
    tab = pk.TABLES[name]
    s, t = pk.row_map(tab)
    cs, ct = pk.contract_map(tab)
    assert np.array_equal(s, cs) and np.array_equal(t, ct)
    for m in range(tab.M):
        fs, first, rows = rc.find(tab.start, m)
        assert pk.ragged_find(tab.start, tab.ns, m) == (fs, first, rows) and rows > 0
        assert tab.n - rows <= t[m] < tab.n and t[m] == tab.first_time(fs) + m - first
    assert len({(a, b) for a, b in zip(s, t)}) == tab.M, "two rows of a table share a (stream, time)"


def _c_ring_slot(t, ML):
    """wn_ring_slot as C computes it: % truncates towards zero"""
    m = abs(t) % ML * (1 if t >= 0 else -1)
    return m + ML if m < 0 else m


def test_slots_and_history_times():
    for ML in sorted(set(pk.FILL_ML + pk.GATHER_ML)):
        for t in list(range(-3 * ML, 3 * ML)) + [2 ** 40 + 5, pk.T62 - 1, -(2 ** 40)]:
            assert pk.ring_slot(t, ML) == ac.ring_slot(t, ML) == _c_ring_slot(t, ML)
        assert any(pk.ring_slot(t, ML, "c %") != pk.ring_slot(t, ML) for t in range(-ML, 0))
        for n in (0, 1, pk.GATHER_N):
            for a in range(n + 1):
                for Lp in (ML - 1, ML + 3):
                    for j in range(1, ML + 1):
                        t = pk.hist_time(n, a, j, Lp)
                        assert t == ac.hist_time(n, a, j, Lp)
                        c = (n - a) - j   # wn_prime_hist_time: -Lp - 1 stands for "dropped", the kernel returns on t < -Lp
                        c = -Lp - 1 if c < -Lp else c
                        assert (t is None) == (c < -Lp) and (t is None or t == c)
    for ML in pk.FILL_ML:   # the kernels keep times in 64 bits: every time of a case fits
        for n_time in pk.fill_times(ML):
            for t_base in pk.fill_bases(ML, n_time):
                assert 0 <= t_base < pk.T62 - n_time and t_base + n_time < 2 ** 63
                ac.check_slots(ML, t_base, n_time)


@pytest.mark.parametrize("cid,kind,kw", PRODUCTS, ids=[c[0] for c in PRODUCTS])
def test_product_case(cid, kind, kw):
    p = pk.product(cid, kw)
    assert not np.isnan(p.ref).any(), "the reference reads a row that holds NaN"
    with np.errstate(invalid="ignore"):
        acc = sum(v @ p.W64[:, j * p.K1:(j + 1) * p.K1].T for j, v in enumerate(p.views(p.s, p.t)))
    if p.bvec is not None:
        acc = acc + p.bvec.astype(np.float64)
    assert np.array_equal(acc.astype(np.float32).astype(np.float64), acc), "the pre-activations leave the exact range"
    if kind == "plain":
        e = p.expect_plain()
        assert (e != SENT32).sum() == p.tab.M * p.N
    if kind != "plain":   # the history in front of a stream's first row is read, finite and non-zero
        for s in range(p.tab.ns):
            if p.tab.rows[s]:
                f = p.tab.first_time(s)
                lo = max(f - p.reach, p.t_min)
                h = p.xl.take64(p.x, np.full(f - lo, s), np.arange(lo, f))
                assert np.isfinite(h).all() and (h != 0).all()
                below = p.xl.take64(p.x, np.array([s]), np.array([lo - 1]))
                assert np.isnan(below).all()
    p.check_sensitive()


def _product_tells(kind):
    return lambda name: [cid for cid, k, kw in PRODUCTS if k == kind and pk.product(cid, kw).tells(name)]


def _start_tells(name):
    out = []
    for cid, kw in pk.start_cases():
        c = pk.StartCase(**kw)
        want, esc0 = c.image()
        got, esc = c.image(name)
        assert esc0 == 0
        if esc or not np.array_equal(want, got):
            out.append("start-" + cid)
    return out


def _fill_tells(name):
    out = []
    for ML, P, ns, R, sh in FILL_SHAPES:
        for c in pk.fill_cases(ML, P, ns, R, sh):
            want, esc0 = c.image()
            got, esc = c.image(name)
            assert esc0 == 0
            if esc or not np.array_equal(want, got):
                out.append(c.tag)
    return out


def _gather_tells(name):
    out = []
    for ML in pk.GATHER_ML:
        for c in pk.gather_cases(ML, 32):
            want, esc0, _ = c.image()
            got, esc, _ = c.image(name)
            assert esc0 == 0
            if esc or not np.array_equal(want, got):
                out.append(c.tag)
    return out


_TELLS = {"start": _start_tells, "fill": _fill_tells, "gather": _gather_tells}
_TELLS.update({kind: _product_tells(kind) for kind in pk.PRODUCT_KINDS})


def test_mutants():
    """every mutant is told from the contract by at least one case of every kernel it concerns (-s prints the table of profiles/r27_prime_kernels.txt)"""
    lines = []
    for num, name, kernels in pk.MUTANTS:
        for k in kernels:
            told = _TELLS[k](name)
            lines.append("mutant %-4s %-22s %-8s told by %3d case(s), e.g. %s" % (num, name, k, len(told), told[0] if told else "-"))
            assert told, "no %s case tells mutant %s (%s) from the contract" % (k, num, name)
    print("\n" + "\n".join(lines))


def test_copy_kernel_cases():
    """the copy kernels' expected images against a second derivation"""
    for cid, kw in pk.start_cases():
        c = pk.StartCase(**kw)
        e, esc = c.image()
        assert esc == 0 and c.idx_stride > max(c.tab.rows)
        w = e.view(np.float32)
        seen = 0
        for s, r in enumerate(c.tab.rows):
            for j in range(r):
                row = w[s, c.xl.pre + c.tab.n - r + j]
                assert np.array_equal(row, c.final[c.idx[s, j]]) and np.isfinite(row).all()
                seen += 1
        assert seen == c.tab.M and (e != SENT32).sum() == c.tab.M * c.R
        assert np.isnan(c.start_t[pk.PAD_CLASS]).all() and (c.idx[:, max(c.tab.rows):] == pk.PAD_CLASS).all()
    for ML, P, ns, R, sh in FILL_SHAPES:
        for c in pk.fill_cases(ML, P, ns, R, sh):
            e, esc = c.image()
            assert esc == 0 and not (e == SENT32).any(), "count = ML rewrites every slot"
            for t in range(c.n_time - ML, c.n_time):
                for s in range(ns):
                    src = c.x[0 if sh else s, c.xl.pre + t]
                    assert src[0] != pk.NAN32 and all(np.array_equal(e[k, s, ac.ring_slot(c.t_base + t, ML)], src) for k in range(P))
            assert (c.x[:, :c.xl.pre + c.n_time - ML] == pk.NAN32).all() and (c.x[:, c.xl.pre + c.n_time:] == pk.NAN32).all()
    drops = 0
    for ML in pk.GATHER_ML:
        for c in pk.gather_cases(ML, 32):
            e, esc, dropped = c.image()
            drops += dropped
            assert esc == 0 and (e[:, :c.guard] == SENT32).all(), "the guard in front of row -Lp"
            assert dropped == (0 if c.Lp >= ML else sum(1 for s in range(c.ns) if c.appended(s) == c.n))
            assert (e != SENT32).sum() == (c.ns * ML - dropped) * c.R
            assert (c.ring[1] == pk.NAN32).all() and (c.ring[0, c.ns:] == pk.NAN32).all()
    assert drops > 0

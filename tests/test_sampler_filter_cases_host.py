"""The cases of the sampling-filter tests (tests/sampler_filter_cases.py), checked without a GPU: every expectation is draw64_filtered's; for u < 1 it
is a kept class; families f-j and the greedy rows have no undecided row, family k at most 1 %; the level rows sit on every seam with dropped classes
between kept ones; with the filter off draw64_filtered IS sampler_cases.draw64; and the cases tell the four mutants from the contract."""
import numpy as np
import pytest

import sampler_cases as sc
import sampler_filter_cases as fc

IDS = ["%s-%s-C%d" % c for c in fc.case_ids()]


def test_case_list():
    assert len(fc.case_ids()) == len(fc.FAMILIES) * (1 + 3)
    assert fc.K_FILTERS == ((0, .9), (0, .5), (40, .95), (5, 0.), (0, .999), (0, 1e-3)) and fc.BAND == 1e-6 and fc.UNDECIDED_CAP == 0.01


def test_filter64_by_hand():
    x = np.array([0., -1., 0., -2., -1., -50.], np.float32)
    e1, e2 = np.exp(-1.), np.exp(-2.)
    assert fc.filter64(x, 0, 0.)[0].all() and fc.filter64(x, 6, 1.)[0].all() and fc.filter64(x, 9, 0.)[0].all()
    assert fc.filter64(x, 1, 0.)[0].tolist() == [True, False, True, False, False, False]          # the tie at the threshold stays
    assert fc.filter64(x, 3, 0.)[0].tolist() == [True, True, True, False, True, False]            # ... inside the second level too
    T = 2 + 2 * e1 + e2 + np.exp(-50.)
    below, above = 2 / T - 0.01, 2 / T + 0.01
    assert fc.filter64(x, 0, below)[0].tolist() == [True, False, True, False, False, False]       # G = 2 for the second level: 2 / T >= top_p
    assert fc.filter64(x, 0, above)[0].tolist() == [True, True, True, False, True, False]
    assert fc.filter64(x, 0, 1e-6)[0].tolist() == [True, False, True, False, False, False]        # the maximum always stays
    # top_p sees the survivors' total: with top_k = 4 the third level is gone and 2 / (2 + 2 e1) is what counts
    mid = 0.5 * (2 / T + 2 / (2 + 2 * e1))
    assert fc.filter64(x, 4, mid)[0].tolist() == [True, False, True, False, False, False]
    assert fc.filter64(x, 0, mid)[0].tolist() == [True, True, True, False, True, False]
    keep, decided = fc.filter64(x, 0, np.float32(2 / T))
    assert not decided                                                                            # on the boundary: inside the band


def test_off_is_draw64():
    fam = sc.family("a", "one_wave", 256)
    for part in fam.parts:
        for i in range(0, part.n, 17):
            for k, p in ((0, 0.), (256, 0.), (300, 1.), (0, 1.)):
                assert fc.draw64_filtered(part.logits[i], part.reg, part.temp[i], part.u[i], False, k, p) == part.expect[i]


@pytest.mark.parametrize("kernel,name,C", fc.case_ids(), ids=IDS)
def test_family(kernel, name, C):
    fam = fc.family(name, kernel, C)
    assert fam.n >= 30, "a family of %d rows" % fam.n
    undecided = 0
    for part in fam.parts:
        dec = part.decided()
        undecided += int((~dec).sum())
        for i in range(part.n):
            want = fc.draw64_filtered(part.logits[i], part.reg, part.temp[i], part.u[i], bool(part.greedy[i]), part.top_k, part.top_p)
            assert part.expect[i] == want, (name, part.kind[i], i, part.top_k, part.top_p)
            if part.greedy[i]:
                assert want == sc.draw64(part.logits[i], part.reg, part.temp[i], part.u[i], True)       # the filter is ignored
            elif part.u[i] < 1.0:
                assert part.keep[part.base[i], want], "the expectation of row %d is a dropped class" % i
            else:
                assert want == C - 1
        if not part.greedy.all():
            x = part.x.astype(np.float64)
            d = x - x.max(axis=1, keepdims=True)
            assert not ((d > -104) & (d <= -87)).any(), "a mass in the denormal range"
            assert part.keep[np.arange(len(part.x)), part.x.argmax(axis=1)].all(), "the maximum is always kept"
    if name in fc.BY_CONSTRUCTION:
        assert undecided == 0, "%d undecided rows in a family that has none by construction" % undecided
    else:
        assert undecided <= fc.UNDECIDED_CAP * fam.n, "%d of %d rows undecided" % (undecided, fam.n)
        assert fam.n >= 2000


@pytest.mark.parametrize("kernel,C", [(k, C) for k in fc.KERNELS for C in fc.class_counts(k)])
def test_levels_sit_on_the_seams(kernel, C):
    """family f: on both sides of every seam there is a row with a kept class, and a row with a dropped class of real mass next to a kept one"""
    fam = fc.family("f", kernel, C)
    kept_at, dropped_at = set(), set()
    for part in fam.parts:
        keep, x = part.keep[0], part.x[0]
        assert int(keep.sum()) == part.top_k and (x[keep] == 0).all()
        dropped = (~keep) & (x > -100)
        assert dropped.any()
        kept_at |= set(np.nonzero(keep)[0].tolist())
        dropped_at |= set(np.nonzero(dropped)[0].tolist())
    for b in sc.seams(kernel, C):
        assert {b - 1, b} <= kept_at and {b - 1, b} <= dropped_at, "seam %d" % b
    assert {0, C - 1} <= kept_at and {0, C - 1} <= dropped_at


def test_top_p_cuts_are_off_the_ratio():
    for kernel in fc.KERNELS:
        for C in fc.class_counts(kernel):
            fam = fc.family("h", kernel, C)
            n_order = 0
            for part in fam.parts:
                x = part.x[0]
                a, b = int((x == 0).sum()), int((x == fc.LOW).sum())
                if getattr(part, "order_row", False):
                    c = int((x == fc.LOWER).sum())
                    n_order += 1
                    assert fc.ratio(a, b, c) + 0.05 <= part.top_p <= fc.ratio(a, b) - 0.05 and part.top_k == a + b
                    assert int(part.keep[0].sum()) == a
                else:
                    assert abs(part.top_p - fc.ratio(a, b)) >= 0.05 - 1e-7
                    assert int(part.keep[0].sum()) == (a if part.top_p < fc.ratio(a, b) else a + b)
            assert n_order >= 3


# ---------------------------------------------------------------- mutants
def _differs(fam, **mutant):
    """rows of the family whose expectation a mutated filter would change (the mutant's draw through the same CDF code)"""
    n = 0
    for part in fam.parts:
        for b in range(len(part.x)):
            keep = fc.filter64(part.x[b], part.top_k, part.top_p, **mutant)[0]
            if np.array_equal(keep, part.keep[b]):
                continue
            rows = np.nonzero((part.base == b) & (part.u < 1.0))[0]
            if not keep.any():
                n += len(rows)
                continue
            cdf = fc.cdf64_filtered(part.x[b], keep)
            n += sum(sc.pick(cdf, part.u[i]) != part.expect[i] for i in rows)
    return n


@pytest.mark.parametrize("kernel,C", [(k, C) for k in fc.KERNELS for C in fc.class_counts(k)])
def test_the_cases_tell_the_mutants(kernel, C):
    g, h = fc.family("g", kernel, C), fc.family("h", kernel, C)
    assert _differs(g, k_strict=True) >= 10, "`>` for `>=` in top_k drops the ties at the threshold: family g"
    assert _differs(h, p_first=True) >= 3, "top_p before top_k: the three-level rows of family h"
    assert _differs(h, p_total_all=True) >= 3, "top_p over the unfiltered total: the three-level rows of family h"
    assert _differs(fc.family("k", kernel, C), p_total_all=True) >= 1
    assert _differs(fc.family("f", kernel, C)) == 0 and _differs(g) == 0 and _differs(h) == 0        # (the contract against itself)


def test_strict_comparison_in_top_p():
    """`<=` for `<` shows only where G_i == top_p * T exactly, and exp() never makes two levels commensurable: with a mass function that weighs both
    levels of a family-h row 1.0, G_B = a, T = a + b, and top_p = a / (a + b) for a == b is exactly 0.5"""
    flat = lambda d: np.where(d < -100, 0.0, 1.0)  # noqa: E731
    n = 0
    for part in fc.family("h", "one_wave", 256).parts:
        x = part.x[0]
        a, b = int((x == 0).sum()), int((x == fc.LOW).sum())
        if a != b or getattr(part, "order_row", False):
            continue
        n += 1
        contract = fc.filter64(x, 0, 0.5, mass=flat)[0]
        mutant = fc.filter64(x, 0, 0.5, mass=flat, p_inclusive=True)[0]
        assert int(contract.sum()) == a and int(mutant.sum()) == a + b
    assert n >= 2

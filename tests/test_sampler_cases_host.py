"""The cases of the sampler kernel tests (tests/sampler_cases.py), checked without a GPU: the caps of family a hold; the expectations are the
reference's (draw64 on every row, and the reference's float32 pipeline -- parity_common.softmax_cdf, searchsorted, clamp -- on every decided and every
exact row); the exact rows are exact (the float32 pipeline's CDF and the float64 one are the same bits, the sums of the float32 masses do not depend
on their order); and the data of families b and d can tell the wrong kernels: side='left', a scan whose lanes / chunks take their prefix one unit too
early, a missing clamp."""
import math

import numpy as np
import pytest

import sampler_cases as sc
from parity_common import softmax_cdf

IDS = ["%s-%s-C%d" % c for c in sc.case_ids()]


def _rows(fam):
    for part in fam.parts:
        for i in range(part.n):
            yield part, i


def _cdf_rows(fam):
    """(part, row, float64 CDF) of the sampled rows; the CDF of a logits row is computed once"""
    memo = {}
    for part, i in _rows(fam):
        if part.greedy[i]:
            continue
        key = (id(part), part.logits[i].tobytes(), float(part.temp[i]))
        if key not in memo:
            memo[key] = sc.cdf64(sc.x32(part.logits[i], part.reg, part.temp[i], False))
        yield part, i, memo[key]


def test_case_list():
    assert len(sc.case_ids()) == 5 * (1 + 4)
    assert sc.unit("generic", 100) == 7 and sc.unit("generic", 40) == 3 and sc.unit("generic", 256) == 16
    assert sc.seams("generic", 40)[-1] == 39 and len(sc.seams("generic", 40)) == 13          # groups 14 and 15 are empty
    assert sc.seams("generic", 100)[-1] == 98 and len(sc.seams("generic", 100)) == 14        # group 15 is empty


@pytest.mark.parametrize("kernel,name,C", sc.case_ids(), ids=IDS)
def test_family(kernel, name, C):
    fam = sc.family(name, kernel, C)
    assert 100 <= fam.n, "a family of %d rows" % fam.n
    n_random = undecided_random = 0
    for part, i in _rows(fam):
        assert part.expect[i] == sc.draw64(part.logits[i], part.reg, part.temp[i], part.u[i], bool(part.greedy[i])), (name, part.kind[i], i)
        if part.greedy[i]:
            x = sc.x32(part.logits[i], part.reg, part.temp[i], True)
            assert x[part.expect[i]] == x.max() and not (x[:part.expect[i]] == x.max()).any()
    for part, i, cdf in _cdf_rows(fam):
        x = sc.x32(part.logits[i], part.reg, part.temp[i], False).astype(np.float64)
        d = x - x.max()
        assert not ((d > -104) & (d <= -87)).any(), "a mass in the denormal range"
        decided = sc.margin(cdf, part.u[i]) > sc.BAND
        if name == "a":
            assert np.array_equal(cdf, part.cdf[part.base[i]])
            if part.kind[i] == "random":
                n_random += 1
                undecided_random += not decided
            else:
                assert decided, "constructed row %d (%s) is undecided" % (i, part.kind[i])
        if decided or fam.exact:      # the expectation is the reference's own
            ref = softmax_cdf(part.logits[i], part.temp[i], part.reg)
            assert sc.pick(ref, part.u[i]) == part.expect[i] == int(min(np.searchsorted(ref, part.u[i], "right"), C - 1)), (name, part.kind[i], i)
    if name == "a":
        assert n_random >= 200 and undecided_random <= 0.005 * n_random, "%d of %d random rows undecided" % (undecided_random, n_random)
        kinds = {k for part in fam.parts for k in part.kind}
        assert kinds == {"random", "mid", "below", "above"}
        assert {float(t) for part in fam.parts for t in part.temp} == {float(np.float32(t)) for t in (1.0, 0.8, 2.5, 0.05)}
        assert [part.reg is None for part in fam.parts] == [True, False]


def _masses32(part, i):
    x = sc.x32(part.logits[i], part.reg, part.temp[i], False)
    p = np.exp(x - x.max()).astype(np.float32)
    return (p * (np.float32(1) / p.sum(dtype=np.float32))).astype(np.float32)


@pytest.mark.parametrize("kernel,name,C", [c for c in sc.case_ids() if c[1] in "bcd"], ids=[i for i in IDS if i.split("-")[1] in "bcd"])
def test_exact_rows_are_exact(kernel, name, C):
    fam = sc.family(name, kernel, C)
    seen = set()
    for part, i, cdf in _cdf_rows(fam):
        p = _masses32(part, i).astype(np.float64)
        key = p.tobytes()
        if key not in seen:     # every prefix sum of the float32 masses is exact in float64: the same in any order
            seen.add(key)
            fwd = np.cumsum(p)
            assert all(fwd[j] == math.fsum(p[:j + 1]) for j in range(C))
            assert fwd[-1] == np.cumsum(p[::-1])[-1] == math.fsum(p)
            u = sc.unit(kernel, C)
            by_unit = sum(float(np.cumsum(p[lo:lo + u])[-1]) for lo in range(0, C, u))
            assert by_unit == fwd[-1]
        ref = softmax_cdf(part.logits[i], part.temp[i], part.reg)
        if part.kind[i] == "mid":        # decided by a hundred times the band, which itself bounds what float32 masses move a CDF value
            assert sc.margin(cdf, part.u[i]) > 100 * sc.BAND and np.abs(ref - cdf).max() < sc.BAND
        else:                            # u may lie ON a CDF value: that value is the same number in float32 masses and in float64
            assert np.array_equal(ref, cdf), (name, part.kind[i], i)
            if part.kind[i] in ("on", "shared"):
                assert part.u[i] == 0.0 or (cdf == part.u[i]).any()
    if name == "b":
        us = {float(u) for part in fam.parts for u in part.u}
        assert {0.0, 1.0, sc.ONE_BELOW} <= us


@pytest.mark.parametrize("mutation", ["left", "shift", "noclamp"])
@pytest.mark.parametrize("kernel,name,C", [c for c in sc.case_ids() if c[1] in "bd"], ids=[i for i in IDS if i.split("-")[1] in "bd"])
def test_data_tells_wrong_kernels(kernel, name, C, mutation):
    fam = sc.family(name, kernel, C)
    wrong = 0
    for part, i in _rows(fam):
        x = sc.x32(part.logits[i], part.reg, part.temp[i], False)
        if mutation == "left":
            got = sc.pick(sc.cdf64(x), part.u[i], side="left")
        elif mutation == "shift":
            got = sc.pick(sc.cdf64(x, shift_unit=sc.unit(kernel, C)), part.u[i])
        else:
            got = sc.pick(sc.cdf64(x), part.u[i], clamp=False)
        wrong += got != part.expect[i]
    assert wrong >= 1, "no row of family %s tells %s" % (name, mutation)


def test_greedy_family_has_its_cases():
    for kernel in sc.KERNELS:
        for C in sc.class_counts(kernel):
            fam = sc.family("e", kernel, C)
            kinds = {k for part in fam.parts for k in part.kind}
            assert kinds == {"random", "tie", "equal", "zeros", "last", "first", "regtie", "undivided"}
            for part, i in _rows(fam):
                assert part.greedy[i] == 1
                x = part.logits[i]
                if part.kind[i] == "equal":
                    assert part.expect[i] == 0
                if part.kind[i] == "last":
                    assert part.expect[i] == C - 1
                if part.kind[i] == "zeros":
                    assert part.expect[i] == sc.seams(kernel, C)[0] - 1 and np.signbit(x[part.expect[i]]) != np.signbit(x[sc.seams(kernel, C)[-1]])
                if part.kind[i] == "regtie":     # the logits tie, x does not (or the tie stays and the first wins)
                    tied = np.nonzero(x == x.max())[0]
                    assert len(tied) == 2 and part.expect[i] in tied
                if part.kind[i] == "undivided":   # dividing would have tied the two and handed the draw to the earlier class
                    xd = sc.x32(x, part.reg, part.temp[i], False)
                    assert int(np.argmax(xd)) < part.expect[i] == int(np.argmax(x))
            temps = {float(t) for part in fam.parts for t in part.temp}
            assert 0.0 in temps and min(temps) < 0
            regtie = [int(part.expect[i]) != int(np.argmax(part.logits[i])) for part, i in _rows(fam) if part.kind[i] == "regtie"]
            assert any(regtie) and not all(regtie)

"""The cases of the log-probability / forced kernel tests (tests/logp_kernel_cases.py), checked without a GPU and without the code under test: family P's
masses are exactly 0 in fp32 and its expected bits are logp64's value to half an ulp; every forced class of M is on the side filter64 says, decided; U's
counts straddle its top_k values; S stays inside the 1 % cap of undecided rows; every family reads each element, lane and chunk; and the verdict the GPU
module uses (judge) tells three planted errors from the contract."""
import math

import numpy as np
import pytest

import logp_kernel_cases as kc
import logprob_cases as lc
import sampler_cases as sc
import sampler_filter_cases as fc

IDS = ["%s-%s-C%d" % c for c in kc.case_ids()]
KC = [(k, C) for k in kc.KERNELS for C in kc.class_counts(k)]
KC_IDS = ["%s-C%d" % c for c in KC]


def test_case_list():
    assert kc.case_ids() == [(k, f, C) for k in ("one_wave", "generic") for f in ("P", "M", "U", "S") for C in ((256,) if k == "one_wave" else (256, 128, 100, 40))]
    assert kc.UNDECIDED_CAP == 0.01 and kc.MODE_BITS == {"sampling": 1, "model": 2} and kc.MODES == ("sampling", "model")
    assert kc.a_of("one_wave", 256) == lc.a_of(3, 256) and kc.a_of("generic", 100) == lc.a_of(1, 100)


@pytest.mark.parametrize("kernel,name,C", kc.case_ids(), ids=IDS)
def test_expectations_are_logp64(kernel, name, C):
    """Base.logp is logp64 (a sample of every part's rows, the same float64 number), a part's arrays are its bases', and a launch stays small"""
    fam = kc.family(name, kernel, C)
    assert fam.n >= 100
    for part in fam.parts:
        assert 1 <= part.n <= 12000 and part.logits.shape == (part.n, C) and set(part.modes) <= set(kc.MODES)
        assert ((part.forced == kc.FREE) | ((part.forced >= 0) & (part.forced < C))).all()
        assert ((part.cls == part.forced) | (part.forced == kc.FREE)).all()
        for mode in part.modes:
            want, _, dec = part.expect(mode)
            for r in list(range(0, part.n, 97)) + [part.n - 1]:
                b = part.bases[part.base[r]]
                assert np.array_equal(part.logits[r], b.logits) and part.temp[r] == b.T and part.greedy[r] == b.greedy
                if part.cls[r] >= 0:
                    ref = lc.logp64(part.logits[r], part.reg, part.temp[r], bool(part.greedy[r]), part.top_k, part.top_p, part.cls[r], mode)
                    assert want[r] == ref or (math.isinf(ref) and want[r] == ref), (r, want[r], ref)
                assert dec[r] == (mode == "model" or lc.kept64(part.logits[r], part.reg, part.temp[r], bool(part.greedy[r]), part.top_k, part.top_p)[2])
        # no mass in the denormal range (sampler_cases' rule), on the rows that are sampled
        for b in part.bases:
            if not b.greedy:
                x = b.kept()[0].astype(np.float64)
                d = x - x.max()
                assert not ((d > -104) & (d <= -87)).any()


# ---------------------------------------------------------------- P
@pytest.mark.parametrize("kernel,C", KC, ids=KC_IDS)
def test_p_masses_are_zero_and_values_exact(kernel, C):
    fam = kc.family("P", kernel, C)
    sampling, model = fam.parts
    assert sampling.reg is None and sampling.modes == kc.MODES and model.reg is not None and model.modes == ("model",)
    maxima = set()
    for part in fam.parts:
        assert part.exact.all() and (part.forced >= 0).all() and part.top_k == 0 and part.top_p == 0.0
        for b in part.bases:
            for mode in part.modes:
                v, keep = b.view(mode)
                assert keep.all()
                d = (v - v.max()).astype(np.float32)                       # fp32 arithmetic, as the kernels form it
                j = int(v.argmax())
                assert d[j] == 0 and (np.delete(d, j) <= np.float32(sc.UNDERFLOW) - 1).all()
                with np.errstate(under="ignore"):
                    mass = np.exp(d)
                assert mass.dtype == np.float32 and mass[j] == 1 and np.count_nonzero(mass) == 1 and mass.sum(dtype=np.float32) == np.float32(1)
                assert len(set(d.tolist())) == C, "every class has a value of its own"
                if mode == "sampling":
                    assert np.array_equal(b.kept()[0].astype(np.float64) * float(b.T if not b.greedy else 1), b.logits.astype(np.float64)), "x / T is exact"
                    maxima.add(j)
        for mode in part.modes:
            want, ex, dec = part.expect(mode)
            assert dec.all() and np.isfinite(want).all()
            assert (np.abs(ex.astype(np.float64) - want) <= 0.5 * np.spacing(np.abs(ex)).astype(np.float64)).all(), "fl32(v_i - max v) is logp64's value to half an ulp"
        # every class is forced once per logits row and form
        for bi in range(len(part.bases)):
            assert sorted(part.forced[part.base == bi].tolist()) == list(range(C))
    assert maxima == set(kc.seam_classes(kernel, C))
    forms = {(float(b.T), b.greedy) for b in sampling.bases}
    assert forms == {(1.0, False), (0.5, False), (0.5, True)}
    assert {(b.T, b.greedy) for b in model.bases} == {(np.float32(kc.P_MODEL_T), False), (np.float32(kc.P_MODEL_T), True)} and kc.P_MODEL_T != 1


# ---------------------------------------------------------------- M
@pytest.mark.parametrize("kernel,C", KC, ids=KC_IDS)
def test_m_forced_classes_are_on_filter64s_side(kernel, C):
    fam = kc.family("M", kernel, C)
    assert {p.source for p in fam.parts} == set(kc.M_SOURCES)
    dropped_at, kept_at, clamp_dropped, clamp_kept = set(), set(), 0, 0
    n_k = n_p = n_both = 0
    for part in fam.parts:
        n_k += fc.top_k_on(part.top_k, C) and not fc.top_p_on(part.top_p)
        n_p += fc.top_p_on(part.top_p) and not fc.top_k_on(part.top_k, C)
        n_both += fc.top_k_on(part.top_k, C) and fc.top_p_on(part.top_p)
        sampled, greedy = part.bases
        x, keep, decided = sampled.kept()
        keep64, dec64 = fc.filter64(x, part.top_k, part.top_p)
        assert decided and dec64 and np.array_equal(keep, keep64) and not keep.all() and keep[x.argmax()]
        want, _, dec = part.expect("sampling")
        assert dec.all() and not part.exact.any()
        s = (part.greedy == 0) & (part.forced >= 0)
        assert sorted(part.forced[s].tolist()) == list(range(C)), "every class is forced"
        assert np.array_equal(np.isneginf(want[s]), ~keep[part.forced[s]]) and np.isfinite(want[s][keep[part.forced[s]]]).all()
        real = x > -100
        dropped_at |= set(np.nonzero(~keep & real)[0].tolist())
        kept_at |= set(np.nonzero(keep)[0].tolist())
        clamp = np.nonzero((part.u == 1.0) & (part.forced == kc.FREE))[0]
        assert len(clamp) == 1 and part.cls[clamp[0]] == C - 1 and np.isneginf(want[clamp[0]]) == (not keep[C - 1])
        clamp_dropped += not keep[C - 1]
        clamp_kept += bool(keep[C - 1])
        g = part.greedy != 0
        assert g.sum() >= 4 and np.isfinite(want[g]).all() and greedy.kept()[1].all(), "a greedy row ignores the filter"
        assert np.isfinite(part.expect("model")[0]).all(), "model mode: every class is finite"
    for b in sc.seams(kernel, C):
        assert {b - 1, b} <= kept_at and {b - 1, b} <= dropped_at, "seam %d" % b
    assert {0, C - 1} <= kept_at and {0, C - 1} <= dropped_at and clamp_dropped >= 3 and clamp_kept >= 3
    assert n_k >= 10 and n_p >= 10 and n_both >= 3


# ---------------------------------------------------------------- U
@pytest.mark.parametrize("kernel,C", KC, ids=KC_IDS)
def test_u_counts_straddle_k(kernel, C):
    fam = kc.family("U", kernel, C)
    assert len(fam.parts) == len(kc.u_filters(C)) * (len(sc.seams(kernel, C)) + 1)
    seen = {}
    under_at = set()
    for part in fam.parts:
        hi, lo = part.hi, part.lo
        assert len(hi) == 3 and len(lo) == 2 and not set(hi) & set(lo)
        under_at |= set(hi) | set(lo)
        k_on, p_on = fc.top_k_on(part.top_k, C), fc.top_p_on(part.top_p)
        for b in part.bases:
            x, keep, decided = b.kept()
            assert decided
            d = x.astype(np.float64) - float(x.max())
            under = d < sc.UNDERFLOW
            assert sorted(np.nonzero(under)[0].tolist()) == sorted(hi + lo) and (d[~under] >= -3).all()
            if b.greedy:
                assert keep.all()
                continue
            above_hi, above_lo = int((x > x[hi[0]]).sum()), int((x > x[lo[0]]).sum())
            assert (above_hi, above_lo) == (C - 5, C - 2) and len(set(x[hi].tolist())) == 1 and len(set(x[lo].tolist())) == 1
            # the contract's three statements about an underflowed class, against kept64
            want_hi = not p_on and (not k_on or above_hi < part.top_k)
            want_lo = not p_on and (not k_on or above_lo < part.top_k)
            assert keep[hi].tolist() == [want_hi] * 3 and keep[lo].tolist() == [want_lo] * 2
            seen[(part.top_k if k_on else 0, p_on)] = (want_hi, want_lo)
        want = part.expect("sampling")[0]
        rows = np.isin(part.forced, hi + lo) & (part.greedy == 0)
        assert {int(c) for c in part.forced[rows]} == set(hi + lo)
        keep_rows = np.array([part.bases[part.base[r]].kept()[1][part.forced[r]] for r in np.nonzero(rows)[0]])
        assert np.array_equal(np.isfinite(want[rows]), keep_rows) and np.array_equal(np.isneginf(want[rows]), ~keep_rows)
        assert (want[rows][keep_rows] < sc.UNDERFLOW).all(), "finite, and far below what log(mass) could give"
        assert np.isfinite(part.expect("model")[0]).all() and np.isfinite(want[part.greedy != 0]).all()
    # k on both sides of both counts, ties at the threshold staying; any top_p drops; every off spelling keeps
    assert seen[(0, False)] == (True, True) and seen[(0, True)] == (False, False)
    assert seen[(C - 5, False)] == (False, False) and seen[(C - 4, False)] == (True, False) and seen[(C - 3, False)] == (True, False)
    assert seen[(C - 2, False)] == (True, False) and seen[(C - 1, False)] == (True, True)
    assert seen[(C - 4, True)] == (False, False) and seen[(C - 1, True)] == (False, False)
    for b in sc.seams(kernel, C):
        assert {b - 1, b} <= under_at
    assert {0, C - 1} <= under_at


# ---------------------------------------------------------------- S
@pytest.mark.parametrize("kernel,C", KC, ids=KC_IDS)
def test_s_stays_inside_the_cap(kernel, C):
    fam = kc.family("S", kernel, C)
    assert len(fam.parts) == 2 * len(fc.K_FILTERS) and {(p.top_k, p.top_p) for p in fam.parts} == {(k if k < C else C // 2, float(np.float32(p))) for k, p in fc.K_FILTERS}
    undecided = 0
    for part in fam.parts:
        assert not part.exact.any()
        free = part.forced == kc.FREE
        assert free.sum() == part.n // 2 and (part.cls[free] == kc.FREE).all() and part.n >= 200
        undecided += int((~part.expect("sampling")[2]).sum())
        assert part.expect("model")[2].all()
    assert undecided <= kc.UNDECIDED_CAP * fam.n, "%d of %d rows undecided" % (undecided, fam.n)
    # (one logits row of sampler_cases' family a has a class within the band of top_p = 0.999 at C = 256 and one at C = 128 -- the kept sum, and with it
    # every value of the row, hangs on that class: all the row's rows are left out; nothing else is)
    assert undecided == {("generic", 256): 68, ("generic", 128): 58}.get((kernel, C), 0)


# ---------------------------------------------------------------- coverage
@pytest.mark.parametrize("kernel,name,C", kc.case_ids(), ids=IDS)
def test_every_element_lane_and_chunk_is_read(kernel, name, C):
    """by the class whose value a row reads back (the forced class, or the clamp's)"""
    fam = kc.family(name, kernel, C)
    read = np.unique(np.concatenate([p.cls[p.cls >= 0] for p in fam.parts]))
    assert set((read & 3).tolist()) == {0, 1, 2, 3}
    if kernel == "one_wave":
        assert set((read >> 2).tolist()) == set(range(64))
    chunk = sc.unit("generic", C)
    used = -(-C // chunk)
    assert set((read // chunk).tolist()) == set(range(used)), "every chunk that holds a class"
    assert used <= sc.GROUPS and (sc.GROUPS - used == 2) == (C == 40) and (sc.GROUPS - used == 1) == (C == 100)
    if name != "S":
        assert len(read) == C, "every class"


# ---------------------------------------------------------------- the verdict, and the planted errors
def _verdict(fam, kernel, plant=None, modes=kc.MODES):
    """(failing rows' messages, parts judged) of the family under the contract's own values (plant = None) or a planted error's"""
    fails = []
    for part in fam.parts:
        for mode in part.modes:
            if mode not in modes:
                continue
            if plant is None:
                want, ex, _ = part.expect(mode)
                idx, bits = part.cls.copy(), np.where(part.exact, ex, want.astype(np.float32)).astype(np.float32).view(np.uint32)
            else:
                idx, bits = kc.planted(part, mode, plant)
            assert (part.cls >= 0).all(), "P, M and U know the class of every row without a kernel"
            f, worst = kc.judge(part, mode, kc.a_of(kernel, fam.C), idx, bits)
            assert worst <= 1.0 or f
            fails += f
    return fails


@pytest.mark.parametrize("kernel,C", KC, ids=KC_IDS)
def test_the_verdict_passes_the_contract(kernel, C):
    for name in ("P", "M", "U"):
        assert not _verdict(kc.family(name, kernel, C), kernel)


@pytest.mark.parametrize("kernel,C", KC, ids=KC_IDS)
@pytest.mark.parametrize("plant", kc.PLANTS)
def test_the_cases_tell_the_planted_errors(plant, kernel, C):
    found = {name: len(_verdict(kc.family(name, kernel, C), kernel, plant)) for name in ("P", "M", "U")}
    assert sum(found.values()) >= 1, "no case of P, M or U fails for %s" % plant
    if plant in ("neighbour_element", "next_lane"):
        assert found["P"] >= 1, "family P has a value of its own for every class"
    else:
        assert found["U"] >= 1 and found["P"] >= 1, "a kept class of mass 0.0 is finite"
        assert not _verdict(kc.family("U", kernel, C), kernel, plant, modes=("model",)), "model mode has no membership"


def test_judge_sees_a_wrong_class_and_a_finite_value_for_a_dropped_one():
    part = kc.family("M", "one_wave", 256).parts[0]
    want, _, _ = part.expect("sampling")
    bits = want.astype(np.float32).view(np.uint32)
    f, worst = kc.judge(part, "sampling", lc.A_ONE_WAVE, part.cls, bits)
    assert not f and worst < 0.5          # (the fp32 rounding of the float64 value itself)
    r = int(np.nonzero(np.isneginf(want))[0][0])
    wrong = bits.copy()
    wrong[r] = np.float32(-200.0).view(np.uint32)
    assert len(kc.judge(part, "sampling", lc.A_ONE_WAVE, part.cls, wrong)[0]) == 1
    idx = part.cls.copy()
    idx[3] ^= 1
    assert len(kc.judge(part, "sampling", lc.A_ONE_WAVE, idx, bits)[0]) == 1
    r = int(np.nonzero(np.isfinite(want))[0][0])
    off = bits.copy()
    off[r] = np.float32(want[r] + 3 * lc.bound(want[r], 256, lc.A_ONE_WAVE)).view(np.uint32)
    f, worst = kc.judge(part, "sampling", lc.A_ONE_WAVE, part.cls, off)
    assert len(f) == 1 and worst > 2

"""-m gpu: the samplers' log-probability and forced forms at kernel level, one draw per workgroup on rows handed over bit for bit
(tests/kernels/wn_kernel_harness.hip includes csrc/wn_runtime.hip): wn_sample_1w_lp<true, true> of kernel variants 3 and 4 as their item loop calls it, and
wn_sample + the forced fork + wn_sample_logp of the generic kernel in wn_l0_input's order, against logprob_cases' float64 statement of the contract
(include/wn_abi.h: wn_set_logprob_output, wn_set_forced_samples).  The cases and the verdict (judge) are tests/logp_kernel_cases.py, checked without a GPU
in tests/test_logp_kernel_cases_host.py.

  * family P: the value of every forced class is fl32(v_i - max v), compared as RAW BITS (the kept sum is 1.0f and logf(1.0f) is +0.0f), in both modes
  * families M and U: a dropped class gives exactly -inf, a kept one -- also one whose mass underflowed -- a finite value within logprob_cases.bound
  * family S: spread rows under the six filters, free and forced, within the bound (a derived bound: nothing here is measured on the kernels)
  * every row returns the class it was forced to; wn_sample_1w_lp: all 64 lanes agree on index and value; wn_sample_logp: the 64 floats behind
    wn_smp_floats(C) keep their sentinel and out[at] is the only float of a guarded buffer that changes; a NULL pointer writes nothing
  * unarmed (r.logp == 0, nothing forced) the new wrappers return the indices of wn_sample_1w<true> / wn_sample on every row of sampler_cases' and
    sampler_filter_cases' families and leave the value's sentinel alone; armed with either mode and nothing forced, the same indices
  * at C = 256 the two samplers agree on the class and on -inf, and differ on a finite value by at most the sum of their bounds
One upload and one synchronisation per family and mode, one launch per part.  The record is printed at the end of the module (pytest -s)."""
import time
import types

import numpy as np
import pytest

import logp_kernel_cases as kc
import logprob_cases as lc
import sampler_cases as sc
import sampler_filter_cases as fc
from kernel_lib import _worst, assert_bits
from kernel_lib import kh  # noqa: F401  (the session fixture)
from kernel_lib import logp_launch as _launch
from kernel_lib import sampler_run as _run

pytestmark = pytest.mark.gpu
RECORD = {}
CASES = [(k, f, C, m) for k, f, C in kc.case_ids() for m in kc.MODES]
IDS = ["%s-%s-C%d-%s" % c for c in CASES]
_DONE = {}


@pytest.fixture(scope="module")
def kf(kh):
    """the shared harness's library (tests/kernel_lib.py), and this module's record at its end"""
    t0 = time.time()
    yield kh.dll
    print("\ntest_gpu_logp_kernels: %.1f s wall (with the harness's build / load only where this module is the first to ask for it); "
          "sampler / family / C / mode: rows, bit exact, -inf, bounded (worst err / bound), left out as undecided" % (time.time() - t0))
    for key in sorted(RECORD):
        r = RECORD[key]
        print("  %-8s %s C=%-3d %-8s rows %5d  exact %5d  -inf %5d  bounded %5d (%.3f)  undecided %3d" % (key + (r["rows"], r["exact"], r["inf"], r["bounded"], r["worst"], r["undecided"])))


def _parts(fam, mode):
    return [p for p in fam.parts if mode in p.modes]


def _run_lp(kf, kernel, fam, mode):
    """a family's parts of one mode through one sampler, once per process -> [(indices, value words)] per part"""
    key = (kernel, fam.kernel, fam.name, fam.C, mode)
    if key not in _DONE:
        _DONE[key] = _launch(kf, kernel, _parts(fam, mode), kc.MODE_BITS[mode])
    return _DONE[key]


def _check(kernel, fam, mode, got):
    rec = {"rows": 0, "exact": 0, "inf": 0, "bounded": 0, "worst": 0.0, "undecided": 0}
    failures = []
    A = kc.a_of(kernel, fam.C)
    for n, (part, (idx, bits)) in enumerate(zip(_parts(fam, mode), got)):
        f, worst = kc.judge(part, mode, A, idx, bits)
        failures += ["%s %s C=%d %s part %d (top_k %d, top_p %r): %s" % (kernel, fam.name, fam.C, mode, n, part.top_k, part.top_p, m) for m in f]
        dec = part.expect(mode)[2]
        inf = dec & (bits == kc.NEG_INF)
        rec["rows"] += part.n
        rec["undecided"] += int((~dec).sum())
        rec["exact"] += int((dec & part.exact & ~inf).sum())
        rec["inf"] += int(inf.sum())
        rec["bounded"] += int((dec & ~part.exact & ~inf).sum())
        rec["worst"] = max(rec["worst"], worst)
    if fam.kernel == kernel:
        RECORD[(kernel, fam.name, fam.C, mode)] = rec
    if fam.name != "P":
        _worst("logp %s (err / bound)" % fam.name, rec["worst"])
    assert not failures, "\n".join(failures[:12])
    return rec


@pytest.mark.parametrize("kernel,name,C,mode", CASES, ids=IDS)
def test_logp_family(kf, kernel, name, C, mode):
    fam = kc.family(name, kernel, C)
    rec = _check(kernel, fam, mode, _run_lp(kf, kernel, fam, mode))
    if name == "P":
        assert rec["exact"] == rec["rows"] == sum(p.n for p in _parts(fam, mode)), "every row of family P is compared bit for bit"
    elif mode == "model":
        assert rec["inf"] == 0 and rec["undecided"] == 0


# ---------------------------------------------------------------- E: equalities
def _unarmed(part, free=(-1,)):
    """a part of sampler_cases / sampler_filter_cases as the new wrappers take it: its own filter (none: off), nothing forced -- `free`: the entries that
    say so, in turn over the rows (anything outside [0, C) is a free position)"""
    forced = np.resize(np.array(free, dtype=np.int64), part.n).astype(np.int32)
    return types.SimpleNamespace(C=part.C, reg=part.reg, top_k=getattr(part, "top_k", 0), top_p=getattr(part, "top_p", 0.0), n=part.n, logits=part.logits,
                                 temp=part.temp, u=part.u, greedy=part.greedy, forced=forced)


OLD = [("sampler_cases",) + c for c in sc.case_ids()] + [("sampler_filter_cases",) + c for c in fc.case_ids()]


@pytest.mark.parametrize("table,kernel,name,C", OLD, ids=["%s-%s-%s-C%d" % c for c in OLD])
def test_unarmed_and_unforced_is_the_draw(kf, table, kernel, name, C):
    """r.logp == 0 and forced = -1: the indices of wn_sample_1w<true> / wn_sample on every row, and no value (the launch checks the sentinel); r.logp = 1 (the free
    entries spelt as -1, C, C + 7, -2, 2^30, INT32_MIN and 4096 in turn) or 2: the same indices"""
    if table == "sampler_cases":
        fam = sc.family(name, kernel, C)
        old = _run(kf, kernel, fam, filter_form=1, filt=(0, 0.0))
    else:
        fam = fc.family(name, kernel, C)
        old = _run(kf, kernel, fam)
    garbage = (-1, C, C + 7, -2, 1 << 30, -(1 << 31), 4096)      # every spelling of a free position, 256 and up also for the wrapper of wn_sample_1w_lp
    for logp_mode in (0, 1, 2):
        new = _launch(kf, kernel, [_unarmed(p, garbage if logp_mode == 1 else (-1,)) for p in fam.parts], logp_mode)
        for n, (want, (idx, bits)) in enumerate(zip(old, new)):
            assert_bits(idx.view(np.uint32), want.view(np.uint32), "%s %s %s C=%d part %d, r.logp = %d: the indices of the draw alone" % (table, kernel, name, C, n, logp_mode))
            if logp_mode:
                assert not (bits == np.uint32(0x7FC0DEAD)).any(), "r.logp = %d: a row without a value" % logp_mode


def _u_decided(part):
    """free rows whose uniform is farther than the band from every value of the filtered float64 CDF: there both samplers return the same class"""
    ok = np.ones(part.n, bool)
    cdfs = {}
    for r in np.nonzero(part.cls < 0)[0]:
        b = int(part.base[r])
        if b not in cdfs:
            x, keep, dec = part.bases[b].kept()
            cdfs[b] = fc.cdf64_filtered(x, keep) if dec else None
        ok[r] = cdfs[b] is not None and sc.margin(cdfs[b], part.u[r]) > sc.BAND
    return ok


@pytest.mark.parametrize("mode", kc.MODES)
@pytest.mark.parametrize("name", kc.FAMILIES)
def test_samplers_agree_at_256(kf, name, mode):
    """each sampler on the other's rows as well: the same class, -inf on the same rows, finite values within the sum of the two bounds"""
    for data in kc.KERNELS:
        fam = kc.family(name, data, 256)
        one, gen = _run_lp(kf, "one_wave", fam, mode), _run_lp(kf, "generic", fam, mode)
        _check("one_wave", fam, mode, one)
        _check("generic", fam, mode, gen)
        for part, (ia, ba), (ib, bb) in zip(_parts(fam, mode), one, gen):
            rows = part.expect(mode)[2] & _u_decided(part)
            assert_bits(ia[rows].view(np.uint32), ib[rows].view(np.uint32), "family %s (%s rows) %s: the two samplers' classes" % (name, data, mode))
            fa, fb = ba.view(np.float32).astype(np.float64), bb.view(np.float32).astype(np.float64)
            assert np.array_equal(ba[rows] == kc.NEG_INF, bb[rows] == kc.NEG_INF), "family %s (%s rows) %s: -inf on different rows" % (name, data, mode)
            fin = rows & (ba != kc.NEG_INF)
            assert np.isfinite(fa[fin]).all() and np.isfinite(fb[fin]).all()
            both = np.array([lc.bound(v, 256, lc.A_ONE_WAVE) + lc.bound(v, 256, lc.a_generic(256)) for v in fa[fin]])
            assert (np.abs(fa[fin] - fb[fin]) <= both).all(), "family %s (%s rows) %s: the two samplers' values" % (name, data, mode)
            if part.exact.all():
                assert_bits(ba, bb, "family %s (%s rows) %s: the two samplers' exact values" % (name, data, mode))


@pytest.mark.parametrize("C", kc.class_counts("generic"))
def test_null_pointer_writes_nothing(kf, C):
    """wn_logp_out's NULL (status words 6..7 zero): the launch checks that the whole guarded buffer keeps its sentinel; the classes are the armed launch's"""
    fam = kc.family("U", "generic", C)
    for mode in kc.MODES:
        armed = _run_lp(kf, "generic", fam, mode)
        for (ia, _), (ib, _) in zip(armed, _launch(kf, "generic", _parts(fam, mode), kc.MODE_BITS[mode], null_out=True)):
            assert_bits(ia.view(np.uint32), ib.view(np.uint32), "C=%d %s: the classes with and without an output" % (C, mode))

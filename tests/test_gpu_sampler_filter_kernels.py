"""-m gpu: the two samplers of the generation chain under the sampling filters (top-k, nucleus: include/wn_abi.h wn_set_sampling), one draw per
workgroup, on logits handed over bit for bit (tests/kernels/wn_kernel_harness.hip includes csrc/wn_runtime.hip: wn_sample_1w<true> of kernel
variants 3 and 4, wn_sample of the generic kernel), against the float64 statement of the contract (sampler_filter_cases.draw64_filtered).  The cases,
their reference and the decision rule are tests/sampler_filter_cases.py, checked on their own in tests/test_sampler_filter_cases_host.py.

  * families f-j and the greedy rows: the indices are BIT EQUAL to the expectation
  * family k: draw64_filtered's index on every decided row; on an undecided row a class that a membership inside the band keeps and whose CDF
    interval reaches within 1e-6 of the uniform
  * every index returned for u < 1 is a kept class
  * wn_sample_1w: all 64 lanes of a row return the same index;  wn_sample: the 64 floats behind wn_smp_floats(C) still hold their sentinel
  * at C = 256 the two samplers agree on every exact and every decided row of both samplers' families
  * wn_sample_1w<true> with the filter off is wn_sample_1w<false>, bit for bit, on sampler_cases' family a
One launch per part (the run carries one regulariser and one filter).  The record is printed at the end of the module (pytest -s)."""
import time

import numpy as np
import pytest

import sampler_cases as sc
import sampler_filter_cases as fc
from kernel_lib import assert_bits
from kernel_lib import kh  # noqa: F401  (the session fixture)
from kernel_lib import sampler_launch as _launch
from kernel_lib import sampler_run as _run

pytestmark = pytest.mark.gpu
RECORD = {}
IDS = ["%s-%s-C%d" % c for c in fc.case_ids()]


@pytest.fixture(scope="module")
def kf(kh):
    """the shared harness's library (tests/kernel_lib.py), and this module's record at its end"""
    t0 = time.time()
    yield kh.dll
    print("\ntest_gpu_sampler_filter_kernels: %.1f s wall (with the harness's build / load only where this module is the first to ask for it); "
          "sampler / family / C: rows, decided, undecided, disagreements with draw64_filtered on decided rows, on undecided rows" % (time.time() - t0))
    for key in sorted(RECORD):
        r = RECORD[key]
        print("  %-8s %s C=%-3d rows %5d  decided %5d  undecided %3d  disagreements %d / %d" % (key + (r["rows"], r["decided"], r["undecided"], r["differ"], r["differ_undecided"])))


def _check(kernel, fam, got):
    rec = {"rows": fam.n, "decided": 0, "undecided": 0, "differ": 0, "differ_undecided": 0}
    failures = []
    for part, idx in zip(fam.parts, got):
        assert ((idx >= 0) & (idx < fam.C)).all(), "an index outside the classes"
        dec = part.decided()
        bad = idx != part.expect
        rec["decided"] += int(dec.sum())
        rec["undecided"] += int((~dec).sum())
        rec["differ"] += int((bad & dec).sum())
        rec["differ_undecided"] += int((bad & ~dec).sum())
        sampled = (part.greedy == 0) & (part.u < 1.0)
        kept = part.keep[part.base, idx]
        for i in np.nonzero(bad & dec)[0][:4]:
            failures.append("%s %s C=%d (top_k %d, top_p %r) %s row %d: T %g u %r -> %d, draw64_filtered %d" % (
                kernel, fam.name, fam.C, part.top_k, part.top_p, part.kind[i], i, part.temp[i], part.u[i], idx[i], part.expect[i]))
        for i in np.nonzero(~dec)[0]:
            if not fc.allowed_filtered(part.x[part.base[i]], part.top_k, part.top_p, part.u[i], int(idx[i])):
                failures.append("%s %s C=%d undecided row %d: class %d is not allowed (u = %r, draw64_filtered %d)" % (kernel, fam.name, fam.C, i, idx[i], part.u[i], part.expect[i]))
        for i in np.nonzero(sampled & dec & ~kept)[0][:4]:
            failures.append("%s %s C=%d row %d: the dropped class %d was returned for u = %r" % (kernel, fam.name, fam.C, i, idx[i], part.u[i]))
    if fam.kernel == kernel:
        RECORD[(kernel, fam.name, fam.C)] = rec
    assert not failures, "\n".join(failures[:12])
    for part, idx in zip(fam.parts, got):
        dec = part.decided()
        assert_bits(idx[dec].view(np.uint32), part.expect[dec].view(np.uint32), "%s %s C=%d, decided rows" % (kernel, fam.name, fam.C))


def test_run_struct_grew_at_its_end(kf):
    assert kf.kf_run_bytes() == 128      # 120 bytes of the fields the kernels had + top_k, top_p


@pytest.mark.parametrize("kernel,name,C", fc.case_ids(), ids=IDS)
def test_sampler_filter(kf, kernel, name, C):
    fam = fc.family(name, kernel, C)
    _check(kernel, fam, _run(kf, kernel, fam))


@pytest.mark.parametrize("name", fc.FAMILIES)
def test_samplers_agree_at_256(kf, name):
    """each sampler on the other's rows as well: the same expectation, hence the same index, on every exact and every decided row"""
    for data in fc.KERNELS:
        fam = fc.family(name, data, 256)
        one, gen = _run(kf, "one_wave", fam), _run(kf, "generic", fam)
        _check("one_wave", fam, one)
        _check("generic", fam, gen)
        for part, a, b in zip(fam.parts, one, gen):
            keep = part.decided()
            assert_bits(a[keep].view(np.uint32), b[keep].view(np.uint32), "family %s (%s rows): the two samplers" % (name, data))


def test_filter_form_with_the_filter_off_is_the_product_form(kf):
    """wn_sample_1w<true> under (0, 0) and under the other off values against wn_sample_1w<false>: every row of sampler_cases' family a, decided or not"""
    fam = sc.family("a", "one_wave", 256)
    for part in fam.parts:
        product = _launch(kf, "one_wave", part, filter_form=0, filt=(0, 0.0))
        for filt in ((0, 0.0), (256, 1.0), (263, 0.0)):
            assert_bits(_launch(kf, "one_wave", part, filt=filt).view(np.uint32), product.view(np.uint32), "wn_sample_1w<true> with (%d, %g)" % filt)

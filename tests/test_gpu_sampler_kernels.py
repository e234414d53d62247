"""-m gpu: the two samplers of the generation chain, one draw per workgroup, on logits handed over bit for bit (tests/kernels/wn_kernel_harness.hip
includes csrc/wn_runtime.hip: wn_sample_1w of kernel variants 3 and 4, wn_sample with wn_smp_carve of the generic kernel), against the float64
statement of wavenet_model.py:280-294 (sampler_cases.draw64).  The cases, their references and the decision rule are tests/sampler_cases.py, checked
on their own in tests/test_sampler_cases_host.py; nothing goes through the persistent chain.

  * exact families (b ties, c one-hot by temperature, d zero-mass runs, e greedy): the indices are BIT EQUAL to the expectation
  * family a (spread): on a row whose uniform is farther than 1e-6 from every float64 CDF value the index is draw64's; on the others it is a class
    whose CDF interval reaches within 1e-6 of the uniform
  * wn_sample_1w: all 64 lanes of a row return the same index (each lane gathers its piece of the start_conv row with it)
  * wn_sample: the 64 floats behind the planner's sampler scratch (wn_smp_floats) still hold their sentinel, for every class count
  * the index outputs sit between sentinel guards that come back untouched (tests/kernel_lib.py: sampler_launch)
  * at C = 256 the two samplers agree on every decided and every exact row of both samplers' families
One launch per family and regulariser (the run carries one regulariser, or none).  The record -- rows, undecided rows, disagreements with draw64 and
their largest distance to a CDF boundary, per sampler and family -- is printed at the end of the module (pytest -s)."""
import time

import numpy as np
import pytest

import sampler_cases as sc
from kernel_lib import assert_bits, sampler_run
from kernel_lib import kh  # noqa: F401  (the session fixture)

pytestmark = pytest.mark.gpu
RECORD = {}


@pytest.fixture(scope="module")
def ks(kh):
    """the shared harness's library (tests/kernel_lib.py), and this module's record at its end"""
    t0 = time.time()
    yield kh.dll
    # the record (shown with pytest -s)
    print("\ntest_gpu_sampler_kernels: %.1f s wall (with the harness's build / load only where this module is the first to ask for it); "
          "sampler / family / C: rows, undecided, disagreements with draw64 (largest distance to a CDF boundary)" % (time.time() - t0))
    for key in sorted(RECORD):
        r = RECORD[key]
        print("  %-8s %s C=%-3d rows %5d  undecided %3d  disagreements %d (%.3g)" % (key + (r["rows"], r["undecided"], r["differ"], r["worst"])))


def _run(ks, kernel, fam):
    """no filter in these cases: wn_sample_1w<false>, the product form, and wn_sample with top_k = top_p = 0"""
    return sampler_run(ks, kernel, fam, filter_form=0, filt=(0, 0.0))


def _decided(part):
    """family a: (decided rows, distance of u to the nearest float64 CDF value)"""
    dist = np.abs(part.cdf[part.base] - part.u[:, None]).min(axis=1)
    return dist > sc.BAND, dist


def _check(kernel, fam, got):
    rec = {"rows": fam.n, "undecided": 0, "differ": 0, "worst": 0.0}
    for part, idx in zip(fam.parts, got):
        assert ((idx >= 0) & (idx < fam.C)).all(), "an index outside the classes"
        bad = idx != part.expect
        if fam.exact:
            dist = np.zeros(part.n)
        else:
            decided, dist = _decided(part)
            rec["undecided"] += int((~decided).sum())
        rec["differ"] += int(bad.sum())
        if bad.any():
            rec["worst"] = max(rec["worst"], float(dist[bad].max()))
            print("%s %s C=%d: %d row(s) differ from draw64, e.g. %s" % (kernel, fam.name, fam.C, int(bad.sum()), [
                (part.kind[i], float(part.temp[i]), part.u[i], int(idx[i]), int(part.expect[i]), float(dist[i])) for i in np.nonzero(bad)[0][:8]]))
    if fam.kernel == kernel:
        RECORD[(kernel, fam.name, fam.C)] = rec
    for part, idx in zip(fam.parts, got):
        if fam.exact:
            assert_bits(idx.view(np.uint32), part.expect.view(np.uint32), "%s %s C=%d" % (kernel, fam.name, fam.C))
        else:
            decided, dist = _decided(part)
            assert_bits(idx[decided].view(np.uint32), part.expect[decided].view(np.uint32), "%s a C=%d, decided rows" % (kernel, fam.C))
            for i in np.nonzero(~decided)[0]:
                assert sc.allowed_undecided(part.cdf[part.base[i]], part.u[i], int(idx[i])), \
                    "%s a C=%d row %d: class %d does not reach within %g of u = %r (draw64: %d)" % (kernel, fam.C, i, idx[i], sc.BAND, part.u[i], part.expect[i])


@pytest.mark.parametrize("kernel,name,C", sc.case_ids(), ids=["%s-%s-C%d" % c for c in sc.case_ids()])
def test_sampler(ks, kernel, name, C):
    fam = sc.family(name, kernel, C)
    _check(kernel, fam, _run(ks, kernel, fam))


@pytest.mark.parametrize("name", sc.FAMILIES)
def test_samplers_agree_at_256(ks, name):
    """each sampler on the other's rows as well: the same expectation, hence the same index, on every exact and every decided row"""
    for data in sc.KERNELS:
        fam = sc.family(name, data, 256)
        one, gen = _run(ks, "one_wave", fam), _run(ks, "generic", fam)
        _check("one_wave", fam, one)
        _check("generic", fam, gen)
        for part, a, b in zip(fam.parts, one, gen):
            keep = np.ones(part.n, bool) if fam.exact else _decided(part)[0]
            assert_bits(a[keep].view(np.uint32), b[keep].view(np.uint32), "family %s (%s rows): the two samplers" % (name, data))

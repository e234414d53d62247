"""-m gpu: the two samplers of the generation chain, one draw per workgroup, on logits handed over bit for bit (tests/kernels/wn_sampler_harness.hip
includes csrc/wn_runtime.hip: wn_sample_1w of kernel variants 3 and 4, wn_sample with wn_smp_carve of the generic kernel), against the float64
statement of wavenet_model.py:280-294 (sampler_cases.draw64).  The cases, their references and the decision rule are tests/sampler_cases.py, checked
on their own in tests/test_sampler_cases_host.py; nothing goes through the persistent chain.

  * exact families (b ties, c one-hot by temperature, d zero-mass runs, e greedy): the indices are BIT EQUAL to the expectation
  * family a (spread): on a row whose uniform is farther than 1e-6 from every float64 CDF value the index is draw64's; on the others it is a class
    whose CDF interval reaches within 1e-6 of the uniform
  * wn_sample_1w: all 64 lanes of a row return the same index (each lane gathers its piece of the start_conv row with it)
  * wn_sample: the 64 floats behind the planner's sampler scratch (wn_smp_floats) still hold their sentinel, for every class count
  * the index outputs sit between sentinel guards that come back untouched (tests/test_gpu_kernels.py)
  * at C = 256 the two samplers agree on every decided and every exact row of both samplers' families
One launch per family and regulariser (the run carries one regulariser, or none).  The record -- rows, undecided rows, disagreements with draw64 and
their largest distance to a CDF boundary, per sampler and family -- is printed at the end of the module (pytest -s)."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
import torch

import sampler_cases as sc
from test_gpu_kernels import SENT32, _stream, assert_bits, dev, host

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64
TAIL = 64                          # KS_TAIL of the harness
OTHER = np.uint32(0x7FC0BEEF)      # what the tail buffer holds before the launch (not the sentinel the kernel copies into it)
_P, _I = ctypes.c_void_p, ctypes.c_int
RECORD = {}
_DONE = {}


@pytest.fixture(scope="module")
def ks():
    """WN_SAMPLER_HARNESS=<path>: load a harness built elsewhere (a mutated copy of the samplers, for a mutation check) instead of building this one"""
    t0 = time.time()
    sys.path.insert(0, os.path.join(HERE, "kernels"))
    import build_sampler_harness
    dll = ctypes.CDLL(os.environ.get("WN_SAMPLER_HARNESS") or build_sampler_harness.build_harness())
    dll.ks_sample_1w.argtypes = [_P, _I, _P, _P, _P, _P, _P, _P]
    dll.ks_sample_generic.argtypes = [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P]
    dll.ks_sample_1w.restype = dll.ks_sample_generic.restype = dll.ks_smp_floats.restype = _I
    assert dll.ks_version() == 1, "stale harness (tests/kernels/build_sampler_harness.py --force)"

    yield dll
    # the record (shown with pytest -s)
    print("\ntest_gpu_sampler_kernels: %.1f s wall with the harness's build / load; sampler / family / C: rows, undecided, disagreements with draw64 (largest distance to a CDF boundary)"
          % (time.time() - t0))
    for key in sorted(RECORD):
        r = RECORD[key]
        print("  %-8s %s C=%-3d rows %5d  undecided %3d  disagreements %d (%.3g)" % (key + (r["rows"], r["undecided"], r["differ"], r["worst"])))


def _launch(ks, kernel, part):
    """-> the indices of the part's rows, after the checks that need no expectation: guards, uniform lanes, the scratch's tail"""
    n, C = part.n, part.C
    per = 64 if kernel == "one_wave" else 1
    logits, u, greedy, temp = dev(part.logits), dev(part.u), dev(part.greedy), dev(part.temp)
    reg = dev(part.reg) if part.reg is not None else None
    out0 = np.full(GUARD + n * per + GUARD, SENT32, np.uint32)
    out = dev(out0)
    o_ptr = out.data_ptr() + 4 * GUARD
    if kernel == "one_wave":
        assert C == 256
        rc = ks.ks_sample_1w(_stream(), n, logits.data_ptr(), reg.data_ptr() if reg is not None else None, u.data_ptr(), greedy.data_ptr(), temp.data_ptr(), o_ptr)
    else:
        tail0 = np.full(GUARD + n * TAIL + GUARD, OTHER, np.uint32)
        tail = dev(tail0)
        rc = ks.ks_sample_generic(_stream(), n, C, logits.data_ptr(), reg.data_ptr() if reg is not None else None, u.data_ptr(), greedy.data_ptr(), temp.data_ptr(),
                                  o_ptr, tail.data_ptr() + 4 * GUARD)
    assert rc == 0, "HIP error %d" % rc
    torch.cuda.synchronize()
    got = host(out, np.uint32)
    assert_bits(got[:GUARD], out0[:GUARD], "%s: guard in front of the indices" % kernel)
    assert_bits(got[-GUARD:], out0[-GUARD:], "%s: guard behind the indices" % kernel)
    idx = got[GUARD:-GUARD].view(np.int32).reshape(n, per)
    if kernel == "one_wave":
        assert_bits(idx, np.repeat(idx[:, :1], 64, axis=1), "one_wave: the lanes of a row disagree")
    else:
        t = host(tail, np.uint32)
        want = tail0.copy()
        want[GUARD:-GUARD] = SENT32
        assert_bits(t, want, "generic C=%d: the %d floats behind the sampler scratch of %d floats" % (C, TAIL, ks.ks_smp_floats(C)))
    return idx[:, 0].copy()


def _run(ks, kernel, fam):
    key = (kernel, fam.kernel, fam.name, fam.C)
    if key not in _DONE:
        _DONE[key] = [_launch(ks, kernel, part) for part in fam.parts]
    return _DONE[key]


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

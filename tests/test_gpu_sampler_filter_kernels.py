"""-m gpu: the two samplers of the generation chain under the sampling filters (top-k, nucleus: include/wn_abi.h wn_set_sampling), one draw per
workgroup, on logits handed over bit for bit (tests/kernels/wn_sampler_filter_harness.hip includes csrc/wn_runtime.hip: wn_sample_1w<true> of kernel
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
import ctypes
import os
import sys
import time

import numpy as np
import pytest
import torch

import sampler_cases as sc
import sampler_filter_cases as fc
from test_gpu_kernels import SENT32, _stream, assert_bits, dev, host

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64
TAIL = 64                          # KF_TAIL of the harness
OTHER = np.uint32(0x7FC0BEEF)
_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
RECORD = {}
_DONE = {}
IDS = ["%s-%s-C%d" % c for c in fc.case_ids()]


@pytest.fixture(scope="module")
def kf():
    t0 = time.time()
    sys.path.insert(0, os.path.join(HERE, "kernels"))
    import build_sampler_filter_harness
    dll = ctypes.CDLL(os.environ.get("WN_SAMPLER_FILTER_HARNESS") or build_sampler_filter_harness.build_harness())
    dll.kf_sample_1w.argtypes = [_P, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P]
    dll.kf_sample_generic.argtypes = [_P, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P]
    dll.kf_sample_1w.restype = dll.kf_sample_generic.restype = dll.kf_smp_floats.restype = dll.kf_run_bytes.restype = _I
    assert dll.kf_version() == 1, "stale harness (tests/kernels/build_sampler_filter_harness.py --force)"
    yield dll
    print("\ntest_gpu_sampler_filter_kernels: %.1f s wall with the harness's build / load; sampler / family / C: rows, decided, undecided, disagreements with "
          "draw64_filtered on decided rows, on undecided rows" % (time.time() - t0))
    for key in sorted(RECORD):
        r = RECORD[key]
        print("  %-8s %s C=%-3d rows %5d  decided %5d  undecided %3d  disagreements %d / %d" % (key + (r["rows"], r["decided"], r["undecided"], r["differ"], r["differ_undecided"])))


def _launch(kf, kernel, part, filter_form=1, filt=None):
    """-> the indices of the part's rows, after the checks that need no expectation: guards, uniform lanes, the scratch's tail"""
    n, C = part.n, part.C
    per = 64 if kernel == "one_wave" else 1
    logits, u, greedy, temp = dev(part.logits), dev(part.u), dev(part.greedy), dev(part.temp)
    reg = dev(part.reg) if part.reg is not None else None
    top_k, top_p = filt if filt is not None else (part.top_k, part.top_p)
    out0 = np.full(GUARD + n * per + GUARD, SENT32, np.uint32)
    out = dev(out0)
    o_ptr = out.data_ptr() + 4 * GUARD
    if kernel == "one_wave":
        assert C == 256
        rc = kf.kf_sample_1w(_stream(), filter_form, n, top_k, top_p, logits.data_ptr(), reg.data_ptr() if reg is not None else None, u.data_ptr(), greedy.data_ptr(),
                             temp.data_ptr(), o_ptr)
    else:
        tail0 = np.full(GUARD + n * TAIL + GUARD, OTHER, np.uint32)
        tail = dev(tail0)
        rc = kf.kf_sample_generic(_stream(), n, C, top_k, top_p, logits.data_ptr(), reg.data_ptr() if reg is not None else None, u.data_ptr(), greedy.data_ptr(),
                                  temp.data_ptr(), o_ptr, tail.data_ptr() + 4 * GUARD)
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
        assert_bits(t, want, "generic C=%d: the %d floats behind the sampler scratch of %d floats" % (C, TAIL, kf.kf_smp_floats(C)))
    return idx[:, 0].copy()


def _run(kf, kernel, fam):
    key = (kernel, fam.kernel, fam.name, fam.C)
    if key not in _DONE:
        _DONE[key] = [_launch(kf, kernel, part) for part in fam.parts]
    return _DONE[key]


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

"""-m gpu: the fused Adam step -- wn_opt_sumsq, wn_opt_adam (csrc/wn_optim.h) and their host side wn_adam_step (csrc/wn_optim.inl) -- called
directly with a hand-filled wn_adam_args on buffers the test owns, through the kernel harness library (tests/kernel_lib.py; WN_KERNEL_HARNESS loads
a mutated build), against the host restatement of tests/adam_cases.py (anchored to libm and torch's CPU optimiser in tests/test_adam_cases_host.py).

Every device operation of the step is a correctly rounded IEEE operation, so the expectation is a BIT PATTERN: families A, B, C and E compare bits,
and their one inequality is the derived bound on the reported norm of random gradients (C2).  Every tensor of a case (p, g, m, v), the norm scratch and
the norm output live in buffers of their own between sentinel guards, and after a call the WHOLE buffer is compared with "sentinels, then the
reference's values": one check for out-of-range writes, untouched tensors and the results.

  A  sizes 1 .. 12289 around the chunk (4096) and the float4 / scalar split, the four pointers independently 0 .. 3 elements off a 16-byte
     boundary, > 100 tensors in one call (batches of 48), entries without a gradient and of size 0 at the batch edges; once more through the
     product library
  B  a pairwise covering of beta1 (both lerp branches and their boundary), beta2, eps, weight decay, step (bias corrections) and lr
  C  clipping: exact norms (the scratch and the reported norm are exact; coef below, at and above 1), random gradients (norm within the derived
     bound, elements bit-equal given the reported norm), the NORM_ONLY / NORM_KEEP / NORM_GIVEN flags
  D  torch.optim.Adam and clip_grad_norm_ ON THE DEVICE as arbiter (the header's claim is about torch's device kernels): 0 differing elements
  E  the argument checks: WN_E_BADARG, a message, nothing touched
  F  FusedAdam at the same edges: misaligned parameter / gradient views, non-contiguous gradients, unequal step counts
The record (D's counts, the denormal tensor, C2's norm error) is printed at the end of the module (pytest -s)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import adam_cases as ac
from kernel_lib import SENT32, _pairwise, assert_bits, dev, host
from kernel_lib import kh  # noqa: F401  (the session fixture)
from mi355_wavenet import _abi

pytestmark = pytest.mark.gpu
RECORD = {}
G = ac.GUARD
FAMILY_B = ac.family_b(_pairwise)


@pytest.fixture(scope="module")
def step_fn(kh):
    """wn_adam_step of the harness library: (wn_adam_args or None) -> return code; and this module's record at its end"""
    t0 = time.time()

    def fn(a):
        return kh.rc("wn_adam_step", None if a is None else ctypes.byref(a))
    fn.last_error = kh.last_error
    yield fn
    print("\ntest_gpu_adam_kernels: %.1f s wall" % (time.time() - t0))
    for key in sorted(RECORD):
        print("  %s: %s" % (key, RECORD[key]))


# ---------------------------------------------------------------- buffers
class Buf:
    """`words` 32-bit words on the device between two guards of G sentinels (+ `off` more in front: the start sits `off` elements behind a 16-byte
    boundary); `h` is what the whole buffer must hold"""

    def __init__(self, words, off=0):
        words = np.ascontiguousarray(words)
        words = words.view(np.uint32) if words.dtype != np.uint32 else words
        self.n, self.lo = len(words), G + off
        self.h = np.full(self.lo + self.n + G, SENT32, np.uint32)
        self.h[self.lo:self.lo + self.n] = words
        self.d = dev(self.h)
        assert self.d.data_ptr() % 16 == 0
        self.ptr = self.d.data_ptr() + 4 * self.lo

    def vals(self):
        return self.h[self.lo:self.lo + self.n].view(np.float32)

    def set(self, vals):
        self.h[self.lo:self.lo + self.n] = ac.bits(vals)

    def got(self):
        return host(self.d, np.uint32)

    def got_vals(self):
        return self.got()[self.lo:self.lo + self.n].view(np.float32)

    def check(self, what):
        assert_bits(self.got(), self.h, what)


class Call:
    """the buffers of one argument array: per entry p, g (none without a gradient), m, v; the norm scratch (a double) and the norm output"""

    def __init__(self, entries):
        self.entries = entries
        self.bufs = []
        for t in entries:
            o = t.offs
            self.bufs.append((Buf(t.p, o[0]), Buf(t.g, o[1]) if t.g is not None and t.has_grad else None, Buf(t.m, o[2]), Buf(t.v, o[3])))
        self.scratch = Buf(np.full(2, SENT32, np.uint32))
        self.total = Buf(np.full(1, SENT32, np.uint32))

    def args(self, hp=ac.DEFAULTS, step=1, max_norm=0.0, flags=0):
        n = len(self.entries)
        tab = lambda k: (ctypes.c_void_p * n)(*[(b[k].ptr if b[k] is not None else None) for b in self.bufs])   # noqa: E731
        self.keep = [(ctypes.c_int64 * n)(*[t.size for t in self.entries]), tab(0), tab(1), tab(2), tab(3)]
        c = [ctypes.cast(x, ctypes.c_void_p) for x in self.keep]
        return _abi.wn_adam_args(n, torch.cuda.current_device(), c[0], c[1], c[2], c[3], c[4], hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"],
                                 float(max_norm), step, self.total.ptr, self.scratch.ptr, torch.cuda.current_stream().cuda_stream, flags)

    def run(self, fn, hp=ac.DEFAULTS, step=1, max_norm=0.0, flags=0):
        rc = fn(self.args(hp, step, max_norm, flags))
        torch.cuda.synchronize()
        assert rc == 0, "wn_adam_step: %d (%s)" % (rc, fn.last_error())

    def expect_step(self, hp, step, coef=1.0):
        """the reference's step on what the buffers must hold now (g * 1 is g, bit for bit: an unclipped gradient comes back as it was)"""
        for t, (p, g, m, v) in zip(self.entries, self.bufs):
            if t.stepped:
                pn, gw, mn, vn = ac.adam_reference(p.vals(), g.vals(), m.vals(), v.vals(), step=step, coef=coef, **hp)
                p.set(pn); g.set(gw); m.set(mn); v.set(vn)

    def expect_norm(self, sumsq=None, total=None):
        if sumsq is not None:
            self.scratch.h[G:G + 2] = np.array([sumsq], np.float64).view(np.uint32)
        if total is not None:
            self.total.set(np.array([total], np.float32))

    def set_scratch(self, value):
        self.expect_norm(sumsq=value)
        self.scratch.d.copy_(dev(self.scratch.h))
        torch.cuda.synchronize()

    def got_total(self):
        return self.total.got_vals()[0]

    def got_sumsq(self):
        return self.scratch.got()[G:G + 2].view(np.float64)[0]

    def check(self, what):
        for i, (t, b) in enumerate(zip(self.entries, self.bufs)):
            for name, x in zip("pgmv", b):
                if x is not None:
                    x.check("%s: entry %d (size %d, offsets %s%s) %s" % (what, i, t.size, t.offs, ", " + t.tag if t.tag else "", name))
        self.scratch.check(what + ": scratch")
        self.total.check(what + ": total_norm")

    def snapshot(self):
        return [x.got() for b in self.bufs for x in b if x is not None]


# ---------------------------------------------------------------- A: sizes, alignment and batching
# Which launcher path a workgroup takes (wn_opt_adam's `vec`, as kst_vec states it for the state kernels): the float4 path needs all four pointers
# on a 16-byte boundary AND a full chunk of 4096 -- so the all-aligned tensors of 4096, 8192 take it throughout, the all-aligned 4097, 8193, 12289
# take it on their full chunks and the scalar path on the tail, and every tensor with a non-zero offset on any of p, g, m, v, and every tensor below
# 4096, takes the scalar path only (ac.Tensor.vec_chunks; tests/test_adam_cases_host.py counts both).
_A_GOT = {}


def _family_a(fn, key):
    call = Call(ac.family_a(_pairwise))
    call.run(fn, ac.DEFAULTS, ac.A_STEP)
    _A_GOT[key] = call.snapshot()
    call.expect_step(ac.DEFAULTS, ac.A_STEP)
    call.check("A")      # (no clipping: scratch and total_norm keep their sentinels; the entries without a gradient / of size 0 are as they were)


def test_a_sizes_alignment_and_batching(step_fn):
    _family_a(step_fn, "harness")


def test_a_product_library_gives_the_harness_bits(step_fn):
    lib = _abi.load_product_library()

    def fn(a):
        return lib.dll.wn_adam_step(ctypes.byref(a))
    fn.last_error = lib.last_error
    _family_a(fn, "product")
    if "harness" not in _A_GOT:
        _family_a(step_fn, "harness")
    for i, (a, b) in enumerate(zip(_A_GOT["product"], _A_GOT["harness"])):
        assert_bits(a, b, "product library against harness, buffer %d" % i)


# ---------------------------------------------------------------- B: hyper-parameters
@pytest.mark.parametrize("case", range(len(FAMILY_B)), ids=lambda i: "b1=%.9g,b2=%g,eps=%g,wd=%g,step=%d,lr=%g" % (
    FAMILY_B[i][0]["beta1"], FAMILY_B[i][0]["beta2"], FAMILY_B[i][0]["eps"], FAMILY_B[i][0]["weight_decay"], FAMILY_B[i][1], FAMILY_B[i][0]["lr"]))
def test_b_hyper_parameters(step_fn, case):
    hp, step, t, _ = FAMILY_B[case]
    call = Call([t])
    call.run(step_fn, hp, step)
    call.expect_step(hp, step)
    call.check("B")


def test_b_the_lerp_branch_follows_the_fp32_weight():
    assert ac.lerp_hi(0.5) and not ac.lerp_hi(ac.B1_OTHER_BRANCH) and np.float32(1 - ac.B1_OTHER_BRANCH) >= np.float32(0.5) - np.float32(2.0 ** -25)
    assert np.float32(1 - 0.5) >= 0.5 and not np.float32(1 - ac.B1_OTHER_BRANCH) >= 0.5
    assert {c[0]["beta1"] for c in FAMILY_B} >= {0.5, ac.B1_BELOW_HALF, ac.B1_OTHER_BRANCH}


# ---------------------------------------------------------------- C1: clipping on an exact norm
def _c1_max_norm(kind, total):
    return {"clip": 0.25 * float(total), "loose": 8.0 * float(total), "c_is_1": ac.max_norm_with_c(total, 0), "c_below_1": ac.max_norm_with_c(total, -1),
            "c_above_1": ac.max_norm_with_c(total, 1)}[kind]


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("kind", ["clip", "loose", "c_is_1", "c_below_1", "c_above_1"])
def test_c1_exact_norm(step_fn, kind, wd):
    entries, sumsq = ac.family_c1()
    total = ac.norm32(sumsq)
    max_norm = _c1_max_norm(kind, total)
    coef = ac.clip_coef(total, max_norm)
    c = ac.raw_c(total, max_norm)
    assert {"clip": coef < 0.5, "loose": c > 2 and coef == 1, "c_is_1": c == 1 and coef == 1, "c_below_1": 1 - 2.0 ** -22 <= coef < 1,
            "c_above_1": c > 1 and coef == 1}[kind]
    hp = dict(ac.DEFAULTS, weight_decay=wd)
    call = Call(entries)
    g0 = [b[1].vals().copy() for b in call.bufs]
    call.run(step_fn, hp, 2, max_norm=max_norm)
    assert call.got_sumsq() == sumsq and ac.bits(call.got_total()) == ac.bits(total)
    call.expect_norm(sumsq, total)
    call.expect_step(hp, 2, coef)
    for g, b in zip(g0, call.bufs):     # the gradient written back is fl(g * coef): no weight decay in it
        assert np.array_equal(ac.bits(b[1].vals()), ac.bits(g * coef))
    call.check("C1 %s" % kind)


# ---------------------------------------------------------------- C2: clipping on random gradients
def test_c2_random_gradients(step_fn):
    """The reported norm against the fp64 norm: |total - norm64| <= 2^-20 * norm64 (ac.C2_NORM_REL: at most 25 fp32 roundings per term, recounted
    from wn_opt_sumsq, non-negative partial sums; half of 25 * 2^-24 for the root, half an ulp for the cast).  The elements: bit-equal to the
    reference on the reported norm, that one fp32 scalar now checked."""
    entries = ac.family_c2()
    norm64 = float(np.sqrt(ac.sumsq64(entries)))
    max_norm = 0.3 * norm64
    hp = dict(ac.DEFAULTS, weight_decay=0.01)
    call = Call(entries)
    call.run(step_fn, hp, 5, max_norm=max_norm)
    total = call.got_total()
    err = abs(float(total) - norm64) / norm64
    print("C2: reported norm %.9g, fp64 norm %.17g, relative error %.3g (bound %.3g)" % (total, norm64, err, ac.C2_NORM_REL))
    RECORD["C2 relative error of the reported norm (bound %.3g)" % ac.C2_NORM_REL] = "%.3g" % err
    assert err <= ac.C2_NORM_REL
    assert ac.bits(ac.norm32(call.got_sumsq())) == ac.bits(total)      # the reported norm is the root of the scratch value
    coef = ac.clip_coef(total, max_norm)
    assert coef < 1
    call.expect_norm(call.got_sumsq(), total)
    call.expect_step(hp, 5, coef)
    call.check("C2")


# ---------------------------------------------------------------- C3: the norm flags
def _groups():
    e1, s1 = ac.family_c1(seed=311, sizes=(4097, 100), offs=((0, 0, 0, 0), (1, 2, 3, 0)))
    e2, s2 = ac.family_c1(seed=312, sizes=(8192, 4095, 3), offs=((0, 0, 0, 0), (0, 3, 0, 0), (0, 0, 0, 0)))
    return Call(e1), s1, Call(e2), s2


def test_c3_norm_only_and_norm_keep_add_up_and_touch_nothing_else(step_fn):
    c1, s1, c2, s2 = _groups()
    c2.scratch = c1.scratch     # both groups' calls share one accumulator
    c1.run(step_fn, ac.DEFAULTS, 1, max_norm=1.0, flags=ac.NORM_ONLY)
    assert c1.got_sumsq() == s1
    c1.expect_norm(sumsq=s1)
    c1.check("NORM_ONLY")       # every p, g, m, v as it was; total_norm still holds its sentinel
    c2.run(step_fn, ac.DEFAULTS, 1, max_norm=1.0, flags=ac.NORM_ONLY | ac.NORM_KEEP)
    assert c2.got_sumsq() == s1 + s2
    c2.expect_norm(sumsq=s1 + s2)
    c2.check("NORM_ONLY | NORM_KEEP")
    c1.check("the first group after the second group's norm pass")
    # NORM_ONLY without NORM_KEEP starts from zero again, also with max_grad_norm = 0
    c2.run(step_fn, ac.DEFAULTS, 1, max_norm=0.0, flags=ac.NORM_ONLY)
    assert c2.got_sumsq() == s2
    c2.expect_norm(sumsq=s2)
    c2.check("NORM_ONLY, max_grad_norm 0")
    # the two-pass protocol: both groups step on the norm over both
    c1.run(step_fn, ac.DEFAULTS, 1, max_norm=1.0, flags=ac.NORM_ONLY)
    c2.run(step_fn, ac.DEFAULTS, 1, max_norm=1.0, flags=ac.NORM_ONLY | ac.NORM_KEEP)
    total = ac.norm32(s1 + s2)
    coef = ac.clip_coef(total, 1.0)
    assert coef < 1
    for c in (c1, c2):
        c.run(step_fn, ac.DEFAULTS, 1, max_norm=1.0, flags=ac.NORM_GIVEN)
        c.expect_norm(sumsq=s1 + s2, total=total)
        c.expect_step(ac.DEFAULTS, 1, coef)
        c.check("NORM_GIVEN on the norm of both groups")


def test_c3_norm_given_uses_the_scratch_value(step_fn):
    c1, s1, _, _ = _groups()
    assert s1 != 4.0
    c1.set_scratch(4.0)         # unrelated to the gradients: a norm pass would overwrite it
    c1.run(step_fn, ac.DEFAULTS, 1, max_norm=0.5, flags=ac.NORM_GIVEN)
    assert ac.bits(c1.got_total()) == ac.bits(np.float32(2.0)) and c1.got_sumsq() == 4.0
    c1.expect_norm(total=2.0)
    c1.expect_step(ac.DEFAULTS, 1, ac.clip_coef(np.float32(2.0), 0.5))
    c1.check("NORM_GIVEN")
    # max_grad_norm = 0: nothing is clipped, whatever the scratch says, and total_norm is left alone
    c2, _, _, _ = _groups()
    c2.set_scratch(4.0)
    c2.run(step_fn, ac.DEFAULTS, 1, max_norm=0.0, flags=ac.NORM_GIVEN)
    c2.expect_step(ac.DEFAULTS, 1)
    c2.check("NORM_GIVEN, max_grad_norm 0")


def test_c3_a_step_without_clipping_leaves_scratch_and_total_norm(step_fn):
    c1, _, _, _ = _groups()
    c1.set_scratch(123.5)
    c1.run(step_fn, ac.DEFAULTS, 1, max_norm=0.0)
    c1.expect_step(ac.DEFAULTS, 1)
    c1.check("no clipping")
    c1.run(step_fn, ac.DEFAULTS, 2, max_norm=-1.0)      # (a negative max_grad_norm is no clipping either)
    c1.expect_step(ac.DEFAULTS, 2)
    c1.check("negative max_grad_norm")


def test_c3_a_nan_norm_poisons_every_parameter_and_gradient(step_fn):
    c1, _, _, _ = _groups()
    c1.set_scratch(np.nan)
    c1.run(step_fn, ac.DEFAULTS, 1, max_norm=1.0, flags=ac.NORM_GIVEN)
    assert np.isnan(c1.got_total())
    for p, g, m, v in c1.bufs:
        for x in (p, g):
            assert np.isnan(x.got_vals()).all()
            x.set(x.got_vals())
        m.set(m.got_vals()); v.set(v.got_vals())
    c1.total.set(np.array([c1.got_total()], np.float32))
    c1.check("NaN norm: the guards")


# ---------------------------------------------------------------- D: torch on the device as arbiter
def _torch_adam(t, hp, step, foreach):
    """torch.optim.Adam's step number `step` on device copies of the entry -> p, exp_avg, exp_avg_sq"""
    p = torch.nn.Parameter(torch.from_numpy(t.p.copy()).cuda())
    p.grad = torch.from_numpy(t.g.copy()).cuda()
    opt = torch.optim.Adam([p], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=hp["weight_decay"], foreach=foreach)
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(t.m.copy()).cuda(), "exp_avg_sq": torch.from_numpy(t.v.copy()).cuda()}
    opt.step()
    st = opt.state[p]
    assert int(st["step"]) == step
    return [x.detach().cpu().numpy() for x in (p, st["exp_avg"], st["exp_avg_sq"])]


def _differing(a, b):
    a, b = ac.bits(a), ac.bits(b)
    return int((a != b).sum())


def _d_inputs():
    out = [("B/%d" % i, hp, step, t) for i, (hp, step, t, _) in enumerate(FAMILY_B)]
    aligned = [t for t in ac.family_a(_pairwise) if t.stepped and t.offs == (0, 0, 0, 0)]
    out += [("A/%d" % i, ac.DEFAULTS, ac.A_STEP, t) for i, t in enumerate(aligned)]
    return out


def _ulps(a, b):
    """the largest distance between finite elements, in units of the last place (the bit patterns as a signed-magnitude order)"""
    def order(x):
        i = ac.bits(x).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    fin = np.isfinite(a) & np.isfinite(b)
    return int(np.abs(order(a) - order(b))[fin].max()) if fin.any() else 0


# torch's two forms on the device disagree with each other in ONE operation, the division of sqrt(v) by the scalar sqrt(1 - beta2^t): the foreach
# form divides (_foreach_div_ with a scalar list), the single-tensor form's `tensor / python_scalar` multiplies by the fp32 rounding of the double
# reciprocal.  Both are fixed sequences (adam_reference(denom="div") and (denom="rcp") reproduce them with 0 differing elements), but they differ in p
# on 27120 of these 223516 elements, by up to 7739 units of the last place (where lr = 1 cancels p): one kernel cannot have both forms' bits.  The
# kernel has the foreach form's, torch's default for device parameters.  Measured on an MI355X with torch 2.10; both sides are deterministic.
D_SINGLE_TENSOR_P_DIFFER, D_SINGLE_TENSOR_P_ULPS = 27120, 7739


@pytest.mark.parametrize("foreach", [False, True])
def test_d_torch_adam_on_the_device(step_fn, foreach):
    """the elements of p, exp_avg and exp_avg_sq whose bits differ between wn_adam_step and torch.optim.Adam on the device, over family B's inputs
    and family A's aligned tensors.  foreach=True: 0.  foreach=False: 0 in exp_avg and exp_avg_sq; in p the count and the distance by which torch's
    two forms differ from each other, as upper bounds -- and torch's single-tensor result is, bit for bit, the reference with that one operation
    in its single-tensor form."""
    count = {"p": 0, "exp_avg": 0, "exp_avg_sq": 0, "elements": 0, "largest distance in p (ulps)": 0, "single-tensor reference against torch": 0}
    where = []
    for tag, hp, step, t in _d_inputs():
        call = Call([t])
        call.run(step_fn, hp, step)
        mine = [call.bufs[0][k].got_vals() for k in (0, 2, 3)]
        theirs = _torch_adam(t, hp, step, foreach)
        assert not any(np.isnan(x).any() for x in mine + theirs)
        d = [_differing(a, b) for a, b in zip(mine, theirs)]
        for k, x in zip(("p", "exp_avg", "exp_avg_sq"), d):
            count[k] += x
        count["elements"] += t.size
        count["largest distance in p (ulps)"] = max(count["largest distance in p (ulps)"], _ulps(mine[0], theirs[0]))
        if not foreach:
            ref = ac.adam_reference(t.p, t.g, t.m, t.v, step=step, denom="rcp", **hp)
            count["single-tensor reference against torch"] += sum(_differing(a, b) for a, b in zip(theirs, (ref[0], ref[2], ref[3])))
        if any(d):
            where.append((tag, hp, step, d))
    RECORD["D torch.optim.Adam(foreach=%s) on the device, differing elements" % foreach] = count
    if foreach:
        assert not where, "differing elements (p, exp_avg, exp_avg_sq) per case: %r" % where[:8]
    else:
        assert count["exp_avg"] == 0 and count["exp_avg_sq"] == 0 and count["single-tensor reference against torch"] == 0, count
        assert count["p"] <= D_SINGLE_TENSOR_P_DIFFER and count["largest distance in p (ulps)"] <= D_SINGLE_TENSOR_P_ULPS, count


@pytest.mark.parametrize("foreach", [False, True])
def test_d_denormals(step_fn, foreach):
    """a tensor whose g, m and v are fp32 denormals: wn_adam_step agrees with torch on the device (asserted); whether both agree with the IEEE
    reference (gradual underflow) is recorded, not asserted"""
    t = ac.denormal_tensor()
    call = Call([t])
    call.run(step_fn, ac.DEFAULTS, 800)
    mine = [call.bufs[0][k].got_vals() for k in (0, 2, 3)]
    theirs = _torch_adam(t, ac.DEFAULTS, 800, foreach)
    ref = ac.adam_reference(t.p, t.g, t.m, t.v, step=800, **ac.DEFAULTS)
    RECORD["D denormal tensor, foreach=%s: elements of (p, exp_avg, exp_avg_sq) differing from torch on the device / from the IEEE reference" % foreach] = (
        "%r / %r of %d" % ([_differing(a, b) for a, b in zip(mine, theirs)], [_differing(a, b) for a, b in zip(mine, (ref[0], ref[2], ref[3]))], t.size))
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), mine, theirs):
        assert _differing(a, b) == 0, name


def test_d_clip_grad_norm_on_the_device(step_fn):
    """the clipped gradients and the norm of torch.nn.utils.clip_grad_norm_ on the device, on gradients whose norm is exact (also as torch forms
    it, a norm of per-tensor norms: the tensors' sums of squares are 4, 4 and 1), at 40 max_norm values and the three around c = 1"""
    rs = np.random.RandomState(21)
    sums, total = (4.0, 4.0, 1.0), np.float32(3.0)
    entries = []
    for s in sums:
        n = int(s * 256)
        p, _, m, v = ac.values(rs, n, huge=False)
        entries.append(ac.Tensor(n, (0, 0, 0, 0), p, (rs.choice([-1.0, 1.0], n) * 2.0 ** -4).astype(np.float32), m, v))
    differ = 0
    for max_norm in [float(x) for x in rs.uniform(0.05, 3.5, 40)] + [ac.max_norm_with_c(total, w) for w in (-1, 0, 1)]:
        call = Call(entries)
        call.run(step_fn, ac.DEFAULTS, 1, max_norm=max_norm)
        ps = [torch.nn.Parameter(torch.zeros(t.size, device="cuda")) for t in entries]
        for q, t in zip(ps, entries):
            q.grad = torch.from_numpy(t.g.copy()).cuda()
        ret = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        assert ac.bits(ret.cpu().numpy()) == ac.bits(total) == ac.bits(call.got_total())
        for q, b in zip(ps, call.bufs):
            differ += _differing(q.grad.cpu().numpy(), b[1].got_vals())
    RECORD["D clip_grad_norm_ on the device, differing gradient elements"] = differ
    assert differ == 0


# ---------------------------------------------------------------- E: argument checks
def _bad_calls():
    def edit(**kw):
        def f(a, call):
            for k, v in kw.items():
                setattr(a, k, v)
            return a
        return f

    def no_exp_avg(a, call):
        tab = call.keep[3]
        tab[1] = None
        return a
    return [("NULL args", lambda a, call: None), ("NULL sizes", edit(sizes=None)), ("NULL params", edit(params=None)), ("NULL grads", edit(grads=None)),
            ("NULL exp_avg table", edit(exp_avg=None)), ("NULL exp_avg_sq table", edit(exp_avg_sq=None)), ("NULL scratch", edit(scratch=None)),
            ("negative n_tensors", edit(n_tensors=-1)), ("step 0", edit(step=0)), ("beta1 1", edit(beta1=1.0)), ("beta2 < 0", edit(beta2=-0.1)),
            ("beta1 NaN", edit(beta1=float("nan"))), ("eps < 0", edit(eps=-1e-8)), ("unknown flag", edit(flags=8)),
            ("NORM_ONLY | NORM_GIVEN", edit(flags=ac.NORM_ONLY | ac.NORM_GIVEN)), ("a gradient but no exp_avg", no_exp_avg)]


@pytest.mark.parametrize("what", [b[0] for b in _bad_calls()])
def test_e_bad_arguments_are_refused_and_touch_nothing(step_fn, what):
    entries, _ = ac.family_c1(seed=321, sizes=(100, 4097), offs=((0, 0, 0, 0), (0, 0, 0, 0)))
    call = Call(entries)
    call.set_scratch(7.25)
    device = torch.cuda.current_device()
    a = dict(_bad_calls())[what](call.args(ac.DEFAULTS, 1, max_norm=1.0), call)
    rc = step_fn(a)
    torch.cuda.synchronize()
    assert rc == _abi.WN_E_BADARG and step_fn.last_error()
    assert torch.cuda.current_device() == device
    call.check(what)


def test_e_nothing_to_do_is_no_error(step_fn):
    entries, _ = ac.family_c1(seed=322, sizes=(100, 4097), offs=((0, 0, 0, 0), (0, 0, 0, 0)))
    device = torch.cuda.current_device()
    call = Call(entries)
    a = call.args(ac.DEFAULTS, 1)
    a.n_tensors = 0
    assert step_fn(a) == 0
    a.n_tensors, a.sizes, a.params, a.grads, a.exp_avg, a.exp_avg_sq = 0, None, None, None, None, None    # (no tables are needed for no tensors)
    assert step_fn(a) == 0
    a = call.args(ac.DEFAULTS, 1)
    call.keep[2][0] = None
    call.keep[2][1] = None      # every gradient NULL
    assert step_fn(a) == 0
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == device
    call.check("nothing to do")


# ---------------------------------------------------------------- F: FusedAdam at the same edges
def _fused(params, **kw):
    from mi355_wavenet.optim import FusedAdam
    return FusedAdam(params, **kw)


def test_f_misaligned_parameter_and_gradient_views_step_to_the_aligned_bits():
    n = ac.CHUNK + 257
    rs = np.random.RandomState(31)
    p0, g0, _, _ = ac.values(rs, n)
    flat, gflat = torch.zeros(n + 8, device="cuda"), torch.zeros(n + 8, device="cuda")
    pv = flat[1:1 + n]
    pv.copy_(torch.from_numpy(p0))
    pv.requires_grad_(True)
    pa = torch.from_numpy(p0.copy()).cuda().requires_grad_(True)
    assert pv.data_ptr() % 16 == 4 and pa.data_ptr() % 16 == 0
    ov, oa = _fused([pv], weight_decay=0.01), _fused([pa], weight_decay=0.01)
    # step 1 without clipping; step 2 clipped, on gradients whose sum of squares is exact in whatever order it is formed (the misaligned view takes
    # the scalar path where the aligned copy takes the float4 path: another order of summation)
    exact = (rs.choice([-1.0, 1.0], n) * np.ldexp(1.0, -rs.randint(4, 10, n))).astype(np.float32)
    for k, g in enumerate((g0, exact)):
        gv = gflat[3:3 + n]
        gv.copy_(torch.from_numpy(g))
        assert gv.data_ptr() % 16 == 12 and gv.is_contiguous()
        pv.grad, pa.grad = gv, torch.from_numpy(g.copy()).cuda()
        ov.step(max_grad_norm=None if k == 0 else 1.0)
        oa.step(max_grad_norm=None if k == 0 else 1.0)
        for a, b, name in ((pv, pa, "p"), (pv.grad, pa.grad, "grad"), (ov.state[pv]["exp_avg"], oa.state[pa]["exp_avg"], "exp_avg"),
                           (ov.state[pv]["exp_avg_sq"], oa.state[pa]["exp_avg_sq"], "exp_avg_sq")):
            assert_bits(host(a.detach().contiguous(), np.uint32), host(b.detach(), np.uint32), "step %d: %s" % (k + 1, name))
    assert float(flat[0]) == 0 and float(flat[1 + n:].abs().sum()) == 0 and float(gflat[:3].abs().sum()) == 0 and float(gflat[3 + n:].abs().sum()) == 0


@pytest.mark.parametrize("clip", [False, True])
def test_f_a_non_contiguous_gradient(clip):
    """with clipping the clipped values are copied back into it; without, it is left bit-identical"""
    rs = np.random.RandomState(32)
    g0 = (rs.choice([-1.0, 1.0], (64, 70)) * np.ldexp(1.0, -rs.randint(4, 10, (64, 70)))).astype(np.float32)    # an exact sum of squares
    sumsq = float(np.sum(g0.astype(np.float64) ** 2))
    p = (rs.standard_normal((64, 70)) * 0.1).astype(np.float32)
    q = torch.from_numpy(p).cuda().requires_grad_(True)
    wide = torch.full((64, 140), 7.0, device="cuda")
    wide[:, ::2] = torch.from_numpy(g0).cuda()
    q.grad = wide[:, ::2]
    assert not q.grad.is_contiguous()
    opt = _fused([q])
    opt.step(max_grad_norm=1.0 if clip else None)
    total = ac.norm32(sumsq)
    coef = ac.clip_coef(total, 1.0) if clip else np.float32(1)
    assert coef < 1 or not clip
    if clip:
        assert ac.bits(opt.last_total_norm.cpu().numpy()) == ac.bits(total)
    want = np.full((64, 140), 7.0, np.float32)
    want[:, ::2] = g0 * coef
    assert_bits(host(wide, np.uint32), ac.bits(want), "the gradient's storage")
    pn, _, mn, vn = ac.adam_reference(p.ravel(), g0.ravel(), np.zeros(p.size, np.float32), np.zeros(p.size, np.float32), step=1, coef=coef, **ac.DEFAULTS)
    assert_bits(host(q.detach(), np.uint32).ravel(), ac.bits(pn), "p")
    assert_bits(host(opt.state[q]["exp_avg"], np.uint32).ravel(), ac.bits(mn), "exp_avg")
    assert_bits(host(opt.state[q]["exp_avg_sq"], np.uint32).ravel(), ac.bits(vn), "exp_avg_sq")


def test_f_parameters_with_different_step_counts_raise():
    a = torch.zeros(10, device="cuda", requires_grad=True)
    b = torch.zeros(10, device="cuda", requires_grad=True)
    opt = _fused([a, b])
    a.grad = torch.ones(10, device="cuda")
    opt.step()
    b.grad = torch.ones(10, device="cuda")
    with pytest.raises(RuntimeError, match="same number of steps"):
        opt.step()

"""-m gpu: the two kernels behind wn_state_save / wn_state_load (csrc/wn_state.inl: wn_state_gather, wn_state_scatter) alone, through the product's
launchers (tests/kernels/wn_kernel_harness.hip includes csrc/wn_runtime.hip), on made-up rings.  Every float of a ring is a bit pattern that encodes
(layer, stream, copy, slot, channel) -- the copies of a stream DIFFER, so a gather that read another copy than 0 would show -- and NaN sentinel bands
surround every buffer.  All comparisons are on the bits.

  * gather at queue time t: row j of layer l's block is slot (t + j) mod ML of copy 0, the caller's channels only; the rings keep their bits
  * scatter of that state at ANOTHER queue time into a range of streams: every copy of every stream of the range holds the state under the slot rule,
    padded channels are exactly +0.0, every other stream, and the guard bands, keep their bits (the other layers' blocks are the neighbours in memory)
  * gather back at that time from every stream of the range: the identity
Dilations 1, 2, 4 with k = 2 and 3; queue times 0, 1, ML-1, ML, 3 ML + 2 (ML of the largest ring); P = 1, 2, 4; streams 0, the middle, the last, a range
in between; R / R_own = 16/16, 32/24 (padded), 7/7 (scalar kernels), 128/128."""
import time

import numpy as np
import pytest
import torch

from kernel_lib import kh  # noqa: F401  (the session fixture)

pytestmark = pytest.mark.gpu
GUARD = 64
SENT = np.uint32(0x7FC0DEAD)
DIL = (1, 2, 4)
NS = 5
_T = {}


@pytest.fixture(scope="module")
def kst(kh):
    """the shared harness's library (tests/kernel_lib.py), and this module's record at its end"""
    t0 = time.time()
    yield kh.dll
    print("\ntest_gpu_state_kernels: %.1f s wall (with the harness's build / load only where this module is the first to ask for it); %d gathers, %d scatters, all bit equal"
          % (time.time() - t0, _T.get("g", 0), _T.get("s", 0)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


class Geo:
    def __init__(self, k, R, R_own, P):
        self.k, self.R, self.R_own, self.P = k, R, R_own, P
        self.ML = [(k - 1) * d + 1 for d in DIL]
        self.row_off = np.concatenate([[0], np.cumsum(self.ML)]).astype(np.int64)
        self.rows = int(self.row_off[-1])
        self.ring_off = np.concatenate([[0], np.cumsum([P * NS * ml * R for ml in self.ML])]).astype(np.int64)
        self.ring_floats = int(self.ring_off[-1])
        self.d_ring_off, self.d_row_off, self.d_dil = _dev(self.ring_off[:-1].copy()), _dev(self.row_off), _dev(np.asarray(DIL, np.int32))

    def rings(self, tag):
        """guarded ring buffer whose floats encode where they are (tag: the top bits, to tell two buffers apart; never a NaN, never zero)"""
        body = (np.arange(self.ring_floats, dtype=np.uint32) + np.uint32(1)) | np.uint32(tag)
        return np.concatenate([np.full(GUARD, SENT, np.uint32), body, np.full(GUARD, SENT, np.uint32)])

    def view(self, buf, l):
        """(P, NS, ML, R) view of layer l's rings inside a guarded host buffer"""
        a = buf[GUARD + int(self.ring_off[l]):GUARD + int(self.ring_off[l + 1])]
        return a.reshape(self.P, NS, self.ML[l], self.R)

    def args(self):
        return (self.d_ring_off.data_ptr(), self.d_row_off.data_ptr(), self.d_dil.data_ptr(), len(DIL), self.k, self.R, self.R_own, NS, self.P, self.rows)

    def expect_state(self, buf, t, s):
        return np.concatenate([self.view(buf, l)[0, s][(t + np.arange(ml)) % ml, :self.R_own].reshape(-1) for l, ml in enumerate(self.ML)])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gather(kst, g, d_rings, t, s, misalign=0):
    n = g.rows * g.R_own
    out0 = np.full(GUARD + n + GUARD, SENT, np.uint32)
    out = _dev(out0)
    rc = kst.kst_gather(_stream(), *g.args(), d_rings.data_ptr() + 4 * GUARD, t, s, out.data_ptr() + 4 * (GUARD + misalign))
    assert rc == 0, "HIP error %d" % rc
    got = _bits(out)
    lo = GUARD + misalign
    assert (got[:lo] == SENT).all() and (got[lo + n:] == SENT).all(), "gather wrote outside the state"
    _T["g"] = _T.get("g", 0) + 1
    return got[lo:lo + n].copy()


@pytest.mark.parametrize("P", [1, 2, 4])
@pytest.mark.parametrize("R,R_own", [(16, 16), (32, 24), (7, 7), (128, 128)])
@pytest.mark.parametrize("k", [2, 3])
def test_gather_scatter_identity_under_the_slot_rule(kst, k, R, R_own, P):
    g = Geo(k, R, R_own, P)
    ml = max(g.ML)
    times = [0, 1, ml - 1, ml, 3 * ml + 2]
    src0 = g.rings(0x10000000)
    d_src = _dev(src0)
    assert kst.kst_vec(R, R_own, d_src.data_ptr()) == (1 if R % 4 == 0 and R_own % 4 == 0 else 0)
    for ti, t in enumerate(times):
        t2 = times[(ti + 2) % len(times)]   # the queue time of the destination: another one
        for s, (s0, cnt) in zip((0, NS // 2, NS - 1, 1), ((0, 1), (NS // 2, 1), (NS - 1, 1), (1, 3))):
            state = _gather(kst, g, d_src, t, s)
            assert np.array_equal(state, g.expect_state(src0, t, s)), "gather t=%d stream %d" % (t, s)
            dst0 = g.rings(0x20000000)
            d_dst, d_state = _dev(dst0), _dev(state)
            rc = kst.kst_scatter(_stream(), *g.args(), d_dst.data_ptr() + 4 * GUARD, t2, s0, cnt, d_state.data_ptr())
            assert rc == 0, "HIP error %d" % rc
            _T["s"] = _T.get("s", 0) + 1
            got = _bits(d_dst)
            exp = dst0.copy()
            off = 0
            for l, m in enumerate(g.ML):
                blk = state[off:off + m * R_own].reshape(m, R_own)
                off += m * R_own
                v = g.view(exp, l)
                slots = (t2 + np.arange(m)) % m
                v[:, s0:s0 + cnt, slots, :R_own] = blk[None, None]
                v[:, s0:s0 + cnt, :, R_own:] = 0          # padded channels: exactly +0.0
            assert np.array_equal(got, exp), "scatter t2=%d streams [%d, %d): copies, padding, neighbours or guards differ" % (t2, s0, s0 + cnt)
            for sb in range(s0, s0 + cnt):
                assert np.array_equal(_gather(kst, g, d_dst, t2, sb), state), "round trip %d -> %d, stream %d" % (t, t2, sb)
    assert np.array_equal(_bits(d_src), src0), "the gathers changed their rings"


def test_a_state_that_is_not_16_byte_aligned_takes_the_scalar_kernels(kst):
    g = Geo(2, 16, 16, 2)
    src0 = g.rings(0x10000000)
    d_src = _dev(src0)
    assert kst.kst_vec(16, 16, d_src.data_ptr()) == 1 and kst.kst_vec(16, 16, d_src.data_ptr() + 4) == 0
    state = _gather(kst, g, d_src, 7, 3, misalign=1)
    assert np.array_equal(state, g.expect_state(src0, 7, 3))
    dst0 = g.rings(0x20000000)
    d_dst = _dev(dst0)
    d_state = _dev(np.concatenate([[SENT], state]).astype(np.uint32))
    assert kst.kst_scatter(_stream(), *g.args(), d_dst.data_ptr() + 4 * GUARD, 2, 1, 2, d_state.data_ptr() + 4) == 0
    assert np.array_equal(_gather(kst, g, d_dst, 2, 2), state)
    got = _bits(d_dst)
    assert (got[:GUARD] == SENT).all() and (got[-GUARD:] == SENT).all()
    assert np.array_equal(g.view(got, 1)[:, 0], g.view(dst0, 1)[:, 0]) and np.array_equal(g.view(got, 1)[:, 3], g.view(dst0, 1)[:, 3])

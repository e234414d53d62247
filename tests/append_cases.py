"""The append form of the batched priming pass restated in Python (csrc/wn_plan.h: wn_prime_plan_host with append, wn_ring_slot, wn_prime_hist_time),
the two invariants it must hold, and the cases of tests/test_append_host.py and tests/test_gpu_prime_append.py.  No torch, no engine.

The pass keeps the times [0, n) of the other forms; pass time t is the queue time t0 + t.  Stream s appends a_s = n_append[s] rows at [n - a_s, n).
Layer l's history gather copies the ring rows j = 1 .. ML (the layer's input at the queue times t0 - j, ring slot (t0 - j) mod ML) to the pass times
(n - a_s) - j, dropping what falls below -Lp; the fill takes all ML columns [n - ML, n) into the slots (t0 + t) mod ML; the products are the ragged
form's (or the rectangle's) over the same lengths."""
import numpy as np

import ragged_cases as rc

SPLIT_LENGTHS = rc.MINI3_LENGTHS


def split_cuts(lengths):
    """where row i is cut into the primed head and the appended tail: 0, 1, L - 1, L in turn, kept inside [0, L]"""
    return [min(max([0, 1, n - 1, n][i % 4], 0), n) for i, n in enumerate(lengths)]


def ring_slot(t, ML):
    """slot of time t, any sign: Python's % is the mathematical modulo for a positive ML"""
    return t % ML


def hist_time(n, n_append, j, Lp):
    """pass time of history row j (1 = the newest), or None: dropped below the workspace"""
    t = (n - n_append) - j
    return None if t < -Lp else t


def base_times(dil, k):
    """the queue times of the sweep: 0, 1, around the largest ring, and a large odd one"""
    ML = (k - 1) * max(dil) + 1
    return [0, 1, ML - 1, ML, ML + 1, 10 ** 6 + 3]


def append_plan(dil, k, R, D, n_append, ns, n, t0):
    """wn_prime_plan_host(append, t0) -> rc.pass_plan's dict with append, base_time and, per layer, fill_cols = hist_rows = ML"""
    p = rc.pass_plan(dil, k, R, D, n_append, ns, n)
    p.update(append=True, base_time=t0)
    for y in p["layer"]:
        y.update(fill_cols=y["ML"], hist_rows=y["ML"])
    return p


def check_append_plan(p, dil, k, n_append):
    """The two invariants, per stream: every row that a history gather, a product or a fill touches lies in [-Lp, n); and every row that a product or
    a fill READS was WRITTEN in this pass, into the buffer it is read from, as the input of the layer that reads it -- by the start gather, by that
    layer's history gather or by the products of the layer below.  owner[buffer][Lp + t] = the layer whose input the row at pass time t is (-1: not
    written in this pass), carried through the ping-pong: layer l + 2 finds layer l's rows in its buffer, and reading one of them is an error here.
    The only history row the clip may drop is j = ML of a stream that appends all n rows; nothing reads it.  Raises AssertionError."""
    n, ns, NL, k1, Lp = p["n"], p["ns"], len(dil), k - 1, p["Lp"]
    assert p["append"] and n >= 1 and Lp == k1 * max(dil)
    lengths = [n] * ns if p["rectangle"] else list(n_append)
    for s, a in enumerate(lengths):
        owner = [np.full(Lp + n, -1, np.int64), np.full(Lp + n, -1, np.int64)]

        def written(buf, lo, hi, layer, what):   # the pass times [lo, hi) of `buf` are read as layer `layer`'s input
            assert -Lp <= lo and hi <= n, (s, layer, what, "outside [-Lp, n)")
            assert (owner[buf][Lp + lo:Lp + hi] == layer).all(), (s, layer, what, "reads a row that this pass did not write as this layer's input")
        owner[0][Lp + n - a:Lp + n] = 0   # the start gather
        for l, y in enumerate(p["layer"]):
            buf, ML, d = l % 2, y["ML"], dil[l]
            assert ML == k1 * d + 1 and y["hist_rows"] == ML and y["fill_cols"] == ML
            for j in range(1, ML + 1):   # the history gather, ahead of the fill and the products
                t = hist_time(n, a, j, Lp)
                if t is None:
                    assert j == ML and a == n and ML == Lp + 1, (s, l, j, "the clip drops a row that is not the dead oldest one")
                    continue
                assert -Lp <= t < n - a, (s, l, j)
                owner[buf][Lp + t] = l
            written(buf, n - ML, n, l, "fill")
            if l == NL - 1:
                continue
            rows = y["rows"] if p["rectangle"] else p["ragged"]["rows"][1 + l][s]
            first = y["t0"] if p["rectangle"] else n - rows
            assert rows == min(p["need"][l + 1], a)
            for tap in range(k):   # tap k - 1 = x(t), which the residual product reads too
                back = (k1 - tap) * d
                if rows:
                    written(buf, first - back, first + rows - back, l, "tap %d" % tap)
            assert first >= n - a and first + rows == n
            owner[1 - buf][Lp + first:Lp + first + rows] = l + 1


def check_slots(ML, t0, n):
    """gather and fill agree with the canonical form: the slot the fill writes pass time t to is the slot of queue time t0 + t, all ML slots are
    written once, and a stream that appends nothing finds every row in the slot its old time has at the new queue time"""
    fill = [ring_slot(t0 + t, ML) for t in range(n - ML, n)]
    assert sorted(fill) == list(range(ML))
    for j in range(1, ML + 1):   # a_s = 0: history row j stands at pass time n - j
        assert ring_slot(t0 - j, ML) == (t0 - j) % ML >= 0
        assert fill[(n - j) - (n - ML)] == ring_slot(t0 + n - j, ML)
    for jj in range(ML):   # the canonical form at the new queue time T: row jj is time T - ML + jj, slot (T + jj) mod ML (wn_state.inl)
        T = t0 + n
        assert fill[jj] == (T + jj) % ML

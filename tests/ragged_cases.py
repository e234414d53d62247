"""The row plan of wn_prime_ragged restated in Python (csrc/wn_plan.h: wn_prime_ragged_plan_host), the properties it must have, and the length sets
of tests/test_ragged_host.py and tests/test_gpu_ragged_prime.py.  No torch, no engine.

Streams are right-aligned at the queue time n.  Stream s holds n_prime[s] samples at the times [n - n_prime[s], n).  Table 0 is the start_conv gather
(n_prime[s] rows), table 1 + l the products of layer l (l = 0 .. NL - 2): the trailing min(need[l + 1], n_prime[s]) rows, need[i] = the trailing
positions of layer i's input that the queues above can still see."""
import numpy as np


def dilations(layers, blocks):
    return [2 ** i for _ in range(blocks) for i in range(layers)]


def need_rows(dil, k):
    """need[0 .. NL]: wn_prime's q before its clamp to n"""
    k1, need = k - 1, [0] * (len(dil) + 1)
    for l in range(len(dil) - 1, -1, -1):
        v = need[l + 1] + k1 * dil[l] if need[l + 1] > 0 else 0
        need[l] = max(v, k1 * dil[l] + 1)
    return need


def plan(dil, k, n_prime, n=None):
    """-> dict(n, need, rows [NL][ns], start [NL][ns + 1], total [NL])"""
    n = max(n_prime) if n is None else n
    assert all(0 <= v <= n for v in n_prime)
    need = need_rows(dil, k)
    rows = [[min(v if t == 0 else need[t], v) for v in n_prime] for t in range(len(dil))]
    start = [[0] + list(np.cumsum(r, dtype=np.int64)) for r in rows]
    return dict(n=n, need=need, rows=rows, start=[[int(v) for v in s] for s in start], total=[int(s[-1]) for s in start])


def prime_rows(dil, k, n):
    """wn_prime's own rows per layer product (its q[l + 1], clamped to n) for streams of one length n"""
    k1, q = k - 1, [0] * (len(dil) + 1)
    for l in range(len(dil) - 1, -1, -1):
        v = q[l + 1] + k1 * dil[l] if q[l + 1] > 0 else 0
        q[l] = min(max(v, k1 * dil[l] + 1), n)
    return q


def find(start, m):
    """row m of a table -> (stream, first row of the stream, its row count): the LAST stream whose start is <= m"""
    s = max(i for i in range(len(start) - 1) if start[i] <= m)
    return s, start[s], start[s + 1] - start[s]


def check_plan(p, dil, k, n_prime):
    """The properties the kernels' addresses rest on; raises AssertionError."""
    n, ns, NL, k1 = p["n"], len(n_prime), len(dil), k - 1
    for t in range(NL):
        st = p["start"][t]
        assert len(st) == ns + 1 and st[0] == 0
        assert all(a <= b for a, b in zip(st, st[1:])), "starts decrease"
        assert st[-1] == p["total"][t] == sum(p["rows"][t]), "total is not the sum"
        assert st[-1] < 2 ** 31
        for s in range(ns):
            r = st[s + 1] - st[s]
            assert 0 <= r <= n_prime[s], "a stream computes a row before its start"
        seen = 0
        for m in range(st[-1]) if st[-1] <= 4096 else ():   # every row belongs to exactly one stream with rows, at a time inside the stream
            s, first, r = find(st, m)
            assert r > 0 and first <= m < first + r
            time = n - r + (m - first)
            assert n - n_prime[s] <= time < n
            seen += 1
        assert st[-1] > 4096 or seen == st[-1]
    for l in range(NL):   # what layer l's input offers (table l) against what reads it
        d = dil[l]
        for s in range(ns):
            have, begin = p["rows"][l][s], n - n_prime[s]   # layer l's input exists on [n - have, n); before `begin` everything is zero
            readers = [min(k1 * d + 1, n)]                  # the ring fill: the newest min(ML, n) columns
            if l < NL - 1:
                readers.append(p["rows"][l + 1][s] + k1 * d if p["rows"][l + 1][s] else 0)   # the products: rows, and k1 * d positions back
            for reach in readers:   # the times [n - reach, n) are read: computed, or before the stream's start (zero), never in between
                assert reach <= have or have == n_prime[s], (l, s, "reads a row inside the stream that was never computed")
                assert n - reach >= -k1 * max(dil), (l, s, "reads in front of the zero prefix")
            assert begin >= 0


# ---- the shapes and length sets
MINI3_DIL = dilations(3, 2)      # 6 layers, rings 2, 3, 5 (kernel_size 2): the GPU tests' MINI3
MINI3_LENGTHS = [0, 1, 2, 4, 5, 127, 128, 129, 300]


def host_sweep():
    """(k, layers, blocks, n_prime) for the CPU sweep: 0, 1, below / at / above every ring length, beyond the receptive field, duplicates, all
    equal, all zero, the longest stream first, last and in the middle"""
    out = []
    for k in (2, 3, 4):
        for layers, blocks in ((3, 2), (4, 1), (1, 1), (10, 1)):
            dil = dilations(layers, blocks)
            rings = sorted({(k - 1) * d + 1 for d in dil})
            rf = 1 + (k - 1) * sum(dil)
            edge = sorted({0, 1} | {v for ml in rings for v in (ml - 1, ml, ml + 1)} | {rf - 1, rf, rf + 1, rf + 130, 2 * rf + 257})
            out.append((k, layers, blocks, edge))
            out.append((k, layers, blocks, edge[::-1]))
            mid = edge[:len(edge) // 2] + [max(edge) + 3] + edge[len(edge) // 2:]
            out.append((k, layers, blocks, mid))
            out.append((k, layers, blocks, [7, 7, 0, 7, rf + 1, rf + 1, 0]))
            out.append((k, layers, blocks, [rf + 5] * 4))
            out.append((k, layers, blocks, [0, 0, 0]))
            out.append((k, layers, blocks, [3]))
            out.append((k, layers, blocks, [0, 0, 9]))
    return out

"""The pass plan of batched priming restated in Python (csrc/wn_plan.h: wn_prime_plan_host, and the ragged form's row plan in it,
wn_prime_ragged_plan_host), the properties it must have, and the length sets of tests/test_ragged_host.py and tests/test_gpu_ragged_prime.py.
No torch, no engine.

Streams are right-aligned at the queue time n.  Stream s holds n_prime[s] samples at the times [n - n_prime[s], n).  Table 0 is the start_conv gather
(n_prime[s] rows), table 1 + l the products of layer l (l = 0 .. NL - 2): the trailing min(need[l + 1], n_prime[s]) rows, need[i] = the trailing
positions of layer i's input that the queues above can still see.  Streams of one length n are the rectangle: no tables, min(need[l + 1], n) rows each."""
import numpy as np


def dilations(layers, blocks):
    return [2 ** i for _ in range(blocks) for i in range(layers)]


def need_rows(dil, k):
    """need[0 .. NL] (wn_prime_need): the layer's own queue, (k - 1) d + 1 columns, and (k - 1) d positions behind what the layer above needs"""
    k1, need = k - 1, [0] * (len(dil) + 1)
    for l in range(len(dil) - 1, -1, -1):
        need[l] = need[l + 1] + k1 * dil[l] if need[l + 1] > 0 else k1 * dil[l] + 1
    return need


def plan(dil, k, n_prime, n=None):
    """the ragged row plan -> dict(n, need, rows [NL][ns], start [NL][ns + 1], total [NL])"""
    n = max(n_prime) if n is None else n
    assert all(0 <= v <= n for v in n_prime)
    need = need_rows(dil, k)
    rows = [[min(v if t == 0 else need[t], v) for v in n_prime] for t in range(len(dil))]
    start = [[0] + list(np.cumsum(r, dtype=np.int64)) for r in rows]
    return dict(n=n, need=need, rows=rows, start=[[int(v) for v in s] for s in start], total=[int(s[-1]) for s in start])


def prime_rows(dil, k, n):
    """the rectangle's rows per layer product for streams of one length n: need, clamped to n"""
    return [min(v, n) for v in need_rows(dil, k)]


def pass_plan(dil, k, R, D, n_prime, ns, n):
    """wn_prime_plan_host (n_prime None: every stream has n) -> dict(ns, n, Lp, Lt, x_floats, z_floats, total_floats, rectangle, start_rows, need,
    layer [NL] of dict(ML, fill_cols, M, entries, rows, t0, z_rows), ragged: plan() or None)"""
    NL, k1 = len(dil), k - 1
    rectangle = n_prime is None or all(v == n for v in n_prime)
    ragged = None if rectangle else plan(dil, k, n_prime, n)
    assert ns * n < 2 ** 31 - 1
    need, Lp = need_rows(dil, k), k1 * max(dil)
    layer = []
    for l, d in enumerate(dil):
        y = dict(ML=k1 * d + 1, fill_cols=min(k1 * d + 1, n), M=0, entries=0, rows=0, t0=0, z_rows=0)
        if l < NL - 1 and rectangle:
            rows = min(need[l + 1], n)
            y.update(entries=ns, rows=rows, t0=n - rows, z_rows=rows)
        elif l < NL - 1:
            y.update(entries=1, rows=ragged["total"][1 + l], t0=0, z_rows=n)
        y["M"] = y["entries"] * y["rows"]
        layer.append(y)
    x_floats, z_floats = ns * (Lp + n) * R, ns * n * D
    return dict(ns=ns, n=n, Lp=Lp, Lt=Lp + n, x_floats=x_floats, z_floats=z_floats, total_floats=2 * x_floats + z_floats, rectangle=rectangle,
                start_rows=ns * n if rectangle else ragged["total"][0], need=need, layer=layer, ragged=ragged)


def check_pass_plan(p, dil, k, R, D):
    """What keeps the kernels inside the allocation: every row a product touches lies in [-Lp, n) of its stream, in a workspace of 2 x + z; raises
    AssertionError.  (The ragged tables' own properties: check_plan.)"""
    n, ns, NL, k1 = p["n"], p["ns"], len(dil), k - 1
    assert p["Lp"] == k1 * max(dil) and p["Lt"] == p["Lp"] + n
    assert p["total_floats"] == 2 * ns * p["Lt"] * R + ns * n * D and p["x_floats"] == ns * p["Lt"] * R and p["z_floats"] == ns * n * D
    assert 0 <= p["start_rows"] <= ns * n
    for l, y in enumerate(p["layer"]):
        assert y["ML"] == k1 * dil[l] + 1 and 0 <= y["fill_cols"] <= min(y["ML"], n), "the ring fill reads the times [n - fill_cols, n)"
        if l == NL - 1:
            assert y["M"] == 0, "the last layer's output is never consumed"
            continue
        assert y["M"] == y["entries"] * y["rows"] < 2 ** 31
        for s in range(ns):   # stream s: `count` rows from `first` on, counted from t0 of its batch entry (ragged: its time n - count, wn_ragged_find)
            count = y["rows"] if p["rectangle"] else p["ragged"]["rows"][1 + l][s]
            first = 0 if p["rectangle"] else n - count
            if count == 0:
                continue
            for tap in range(k):   # tap 0 = the oldest
                assert y["t0"] + first - (k1 - tap) * dil[l] >= -p["Lp"], (l, s, tap, "reads in front of the zero prefix")
            assert y["t0"] + first >= 0, (l, s, "writes into the zero prefix")
            assert y["t0"] + first + count - 1 < n, (l, s, "touches a row behind the stream")
            assert first + count - 1 < y["z_rows"] and y["entries"] * y["z_rows"] <= ns * n, (l, s, "z row outside z")
        assert p["rectangle"] or sum(p["ragged"]["rows"][1 + l]) == y["M"]


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

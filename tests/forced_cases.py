"""Forced samples (include/wn_abi.h: wn_set_forced_samples): the masks and the forced classes the tests use; numpy only, no GPU.
tests/test_forced_host.py checks the builders themselves, tests/test_gpu_forced.py runs whole jobs with them.

A mask is bool (n_streams, n): True = the position is forced.  forced_array(mask, values) is what the engine takes: values on the mask, FREE elsewhere.
  positions(n)        one row: position 0, a run of 5, every third position behind the run, the last position
  per_stream(ns, n)   rows that differ: row 0 all free (with a single stream: positions(n)), row 1 all forced, the others positions(n) shifted by the
                      row number and thinned differently -- no two rows are equal
  shifted_classes(plain, classes) = (plain + 128) % classes: never the class the unforced job emitted at that position (classes > 128), so the FIRST
                      forced position of a stream provably changes what the stream emits there and feeds the network afterwards
  ragged_prefix_lengths(ns) = 0, 5, 1, 7, 2, 6, 3, 4, 0, 5, ...: one stream without a prefix, no two neighbours alike"""
import numpy as np

FREE = -1
RUN = (7, 12)              # the run of 5: positions 7 .. 11
RAGGED = (0, 5, 1, 7, 2, 6, 3, 4)


def positions(n):
    assert n >= 16
    m = np.zeros(n, bool)
    m[0] = True
    m[RUN[0]:RUN[1]] = True
    m[RUN[1] + 3::3] = True
    m[n - 1] = True
    return m


def per_stream(ns, n):
    base = positions(n)
    if ns == 1:
        return base[None, :].copy()
    rows = []
    for s in range(ns):
        if s == 0:
            rows.append(np.zeros(n, bool))
        elif s == 1:
            rows.append(np.ones(n, bool))
        else:
            r = np.roll(base, s)
            r[s::s + 3] = False      # (thinned with a stride of its own: the rows stay different beyond the roll)
            r[s] = True
            rows.append(r)
    return np.stack(rows)


def shared(ns, n):
    return np.tile(positions(n), (ns, 1))


def forced_array(mask, values):
    values = np.broadcast_to(np.asarray(values), mask.shape)
    return np.where(mask, values, FREE).astype(np.int32)


def shifted_classes(plain_idx, classes):
    assert classes > 128
    return ((np.asarray(plain_idx).astype(np.int64) + 128) % classes).astype(np.int32)


def first_forced(mask_row):
    """the first forced position of a row, or None"""
    at = np.nonzero(mask_row)[0]
    return int(at[0]) if at.size else None


def ragged_prefix_lengths(ns):
    return [RAGGED[s % len(RAGGED)] for s in range(ns)]

"""CPU: batched priming onto a live state without a GPU.  The append form of the pass plan (csrc/wn_plan.h: wn_prime_plan_host with append, wn_ring_slot,
wn_prime_hist_time) compiled with g++ and held to its Python restatement (tests/append_cases.py) over the length sets of the ragged sweep times six
queue times, once more as a stand-alone program under AddressSanitizer / UBSan; the two invariants of the plan; the binding; and the facade's append=,
advance_state and prime_piece_samples on a fake engine."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import append_cases as ac
import ragged_cases as rc
import wavenet_model
from double_lib import double_backend, double_library
from facade_schedule_lib import FakeEngine
from mi355_wavenet import _abi, engine, synth
from test_generation_state_host import _some_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-wavenet_amd", "csrc")
TINY = synth.CONFIGS["tiny"]
NAME = "wn_prime_append"

HARNESS = r"""
#include "wn_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
// plan <kernel_size> <layers> <blocks> <R> <D> <ns> <n> <t0,t0,... ; -1: the form that is not the append form> [<length> x ns; none: NULL]
//   -> per t0: "pass Lp Lt x_floats z_floats total_floats rectangle start_rows append base_time", "need ...", one line per layer
//      "ML fill_cols M entries rows t0 z_rows hist_rows", then (ragged) the tables "<total> | start[0] .. start[ns]"; or "REFUSED why"
// slots <ML> <t>...            -> wn_ring_slot(t, ML) of every t
// hist <n> <n_append> <Lp> <j>... -> wn_prime_hist_time of every j ("-" for a dropped row)
int main(int argc, char** argv) {
    if (!strcmp(argv[1], "slots")) {
        for (int i = 3; i < argc; ++i) printf("%lld\n", wn_ring_slot(atoll(argv[i]), atoll(argv[2])));
        return 0;
    }
    if (!strcmp(argv[1], "hist")) {
        const long long n = atoll(argv[2]), a = atoll(argv[3]), Lp = atoll(argv[4]);
        for (int i = 5; i < argc; ++i) {
            const long long t = wn_prime_hist_time(n, a, atoll(argv[i]), Lp);
            if (t < -Lp) printf("-\n"); else printf("%lld\n", t);
        }
        return 0;
    }
    const int k = atoi(argv[2]), layers = atoi(argv[3]), blocks = atoi(argv[4]), R = atoi(argv[5]), D = atoi(argv[6]), ns = atoi(argv[7]);
    const long long n = atoll(argv[8]);
    std::vector<long long> times;
    for (char* tok = strtok(argv[9], ","); tok; tok = strtok(nullptr, ",")) times.push_back(atoll(tok));
    std::vector<int32_t> dil;
    for (int b = 0; b < blocks; ++b) for (int i = 0; i < layers; ++i) dil.push_back(1 << i);
    std::vector<int64_t> len;
    for (int i = 10; i < argc; ++i) len.push_back(atoll(argv[i]));
    if (!len.empty() && (int)len.size() != ns) { printf("USAGE\n"); return 1; }
    for (long long t0 : times) {
        WnPrimePlan p;
        const std::string why = t0 < 0 ? wn_prime_plan_host(dil.data(), (int)dil.size(), k, R, D, len.empty() ? nullptr : len.data(), ns, n, p)
                                       : wn_prime_plan_host(dil.data(), (int)dil.size(), k, R, D, len.empty() ? nullptr : len.data(), ns, n, p, true, t0);
        if (!why.empty()) { printf("REFUSED %s\n", why.c_str()); continue; }
        if (p.ns != ns || p.NL != (int)dil.size() || p.n != n || (int)p.layer.size() != p.NL) { printf("FIELDS\n"); return 1; }
        printf("pass %lld %lld %zu %zu %zu %d %lld %d %lld\nneed", p.Lp, p.Lt, p.x_floats, p.z_floats, p.total_floats, p.rectangle ? 1 : 0, p.start_rows, p.append ? 1 : 0,
               p.base_time);
        for (long long v : p.need) printf(" %lld", v);
        printf("\n");
        for (const WnPrimeLayer& y : p.layer) printf("%d %d %lld %lld %lld %lld %lld %d\n", y.ML, y.fill_cols, y.M, y.entries, y.rows, y.t0, y.z_rows, y.hist_rows);
        for (int t = 0; !p.rectangle && t < p.ragged.n_tables; ++t) {
            printf("%lld |", p.ragged.total[t]);
            for (int s = 0; s <= p.ragged.ns; ++s) printf(" %d", p.ragged.table(t)[s]);
            printf("\n");
        }
    }
    return 0;
}
"""

LAYER_KEYS = ("ML", "fill_cols", "M", "entries", "rows", "t0", "z_rows", "hist_rows")
HEAD_KEYS = ("Lp", "Lt", "x_floats", "z_floats", "total_floats", "rectangle", "start_rows", "append", "base_time")


def _build(tmp, flags, name):
    src = tmp / (name + ".cpp")
    src.write_text(HARNESS)
    exe = tmp / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("append"), [], "append_harness")


def _run_plan(exe, k, layers, blocks, R, D, ns, n, times, lengths=None):
    """-> one plan per queue time, in the form of ac.append_plan (ragged: its start and total), or the refusal line"""
    out = subprocess.check_output([exe, "plan"] + [str(v) for v in (k, layers, blocks, R, D, ns, n)] + [",".join(str(t) for t in times)]
                                  + [str(v) for v in lengths or ()]).decode().splitlines()
    plans, NL = [], layers * blocks
    while out:
        if out[0].startswith("REFUSED"):
            plans.append(out.pop(0))
            continue
        p = dict(zip(HEAD_KEYS, (int(v) for v in out[0].split()[1:])), ns=ns, n=n)
        p["rectangle"], p["append"] = bool(p["rectangle"]), bool(p["append"])
        p["need"] = [int(v) for v in out[1].split()[1:]]
        p["layer"] = [dict(zip(LAYER_KEYS, (int(v) for v in line.split()))) for line in out[2:2 + NL]]
        tables = out[2 + NL:2 + NL + (0 if p["rectangle"] else NL)]
        p["ragged"] = None if p["rectangle"] else dict(start=[[int(v) for v in line.split("|")[1].split()] for line in tables], total=[int(line.split("|")[0]) for line in tables])
        out = out[2 + NL + len(tables):]
        plans.append(p)
    assert len(plans) == len(times)
    return plans


def _hold_plan(exe, k, layers, blocks, R, D, ns, n, lengths=None):
    """the C++ plan at every queue time of the sweep against the restatement; the invariants once (they do not depend on the queue time)"""
    dil = rc.dilations(layers, blocks)
    times = ac.base_times(dil, k)
    case = (k, layers, blocks, R, D, ns, n, lengths)
    for t0, got in zip(times, _run_plan(exe, k, layers, blocks, R, D, ns, n, times, lengths)):
        want = ac.append_plan(dil, k, R, D, lengths, ns, n, t0)
        assert not isinstance(got, str), (case, t0, got)
        for key in got:
            if key != "ragged":
                assert got[key] == want[key], (case, t0, key)
        assert (got["ragged"] is None) == want["rectangle"], case
        if not want["rectangle"]:
            assert got["ragged"]["start"] == want["ragged"]["start"] and got["ragged"]["total"] == want["ragged"]["total"], case
    ac.check_append_plan(want, dil, k, lengths)
    rc.check_pass_plan(dict(want, layer=[dict(y, fill_cols=min(y["ML"], n)) for y in want["layer"]]), dil, k, R, D)   # the products' bounds: the ragged form's check
    return want


def _hold_sweep(exe):
    cases = [c for c in rc.host_sweep() if max(c[3]) > 0]   # (all lengths 0: the entry point returns before it plans)
    assert len(cases) >= 80
    for k, layers, blocks, lengths in cases:
        _hold_plan(exe, k, layers, blocks, 128, 128, len(lengths), max(lengths), lengths)
    for k in (2, 3, 4):   # the shared form: one stream's rectangle; a front member whose own streams are all shorter than the job's n, or append nothing
        for n in (1, 4 * (k - 1), 4 * (k - 1) + 1, 300):
            _hold_plan(exe, k, 3, 2, 32, 64, 1, n)
        _hold_plan(exe, k, 3, 2, 32, 64, 4, 300, [1, 4, 0, 9])
        _hold_plan(exe, k, 3, 2, 32, 64, 2, 5, [0, 0])


def test_append_plan_against_the_restatement(harness):
    _hold_sweep(harness)


def test_append_plan_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "append_harness_san")
    _hold_sweep(exe)
    _hold_slots(exe)
    assert "2^62" in _run_plan(exe, 2, 3, 2, 32, 32, 2, 8, [2 ** 62 - 8], [4, 8])[0]


def test_append_plan_in_numbers(harness):
    """MINI3 (rings 2, 3, 5, Lp 4): every ring is rewritten whole, the history is as long as the ring, the products and the workspace are the ragged form's"""
    p = _hold_plan(harness, 2, 3, 2, 128, 128, 9, 300, rc.MINI3_LENGTHS)
    assert [(y["fill_cols"], y["hist_rows"]) for y in p["layer"]] == [(2, 2), (3, 3), (5, 5), (2, 2), (3, 3), (5, 5)]
    assert p["total_floats"] == 2 * 9 * 304 * 128 + 9 * 300 * 128
    one = _hold_plan(harness, 2, 3, 2, 128, 128, 3, 1)   # n = 1 on every stream: the fill reads the times [1 - ML, 1), down to -Lp
    assert [y["fill_cols"] for y in one["layer"]] == [2, 3, 5, 2, 3, 5] and one["Lp"] == 4


def test_the_clip_drops_the_dead_oldest_row_only():
    """(n - a) - j < -Lp needs j = ML = Lp + 1 and a = n: the layer of the largest dilation, a stream that appends all n rows"""
    for Lp in (1, 4, 512):
        for n in (1, 2, Lp, Lp + 1, 3 * Lp):
            for a in (0, 1, n - 1, n):
                if not 0 <= a <= n:
                    continue
                dropped = [j for j in range(1, Lp + 2) if ac.hist_time(n, a, j, Lp) is None]
                assert dropped == ([Lp + 1] if a == n else []), (Lp, n, a)


def test_with_no_history_the_plan_is_the_ragged_plan(harness):
    """queue time 0: the same products, tables and workspace as wn_prime_ragged over the same lengths; only fill_cols and the history differ"""
    for k, layers, blocks, lengths in [c for c in rc.host_sweep() if max(c[3]) > 0][::3]:
        n, ns = max(lengths), len(lengths)
        app, rag = _run_plan(harness, k, layers, blocks, 128, 128, ns, n, [0, -1], lengths)
        assert app["append"] and not rag["append"] and rag["base_time"] == 0
        for key in ("Lp", "Lt", "x_floats", "z_floats", "total_floats", "rectangle", "start_rows", "need", "ragged"):
            assert app[key] == rag[key], (k, layers, blocks, lengths, key)
        for ya, yr in zip(app["layer"], rag["layer"]):
            assert {q: ya[q] for q in ("ML", "M", "entries", "rows", "t0", "z_rows")} == {q: yr[q] for q in ("ML", "M", "entries", "rows", "t0", "z_rows")}
            assert yr["hist_rows"] == 0 and yr["fill_cols"] == min(yr["ML"], n) and ya["fill_cols"] == ya["hist_rows"] == ya["ML"]


def _hold_slots(exe):
    for ML in (1, 2, 3, 5, 17, 1537):
        ts = [-3 * ML - 1, -ML - 1, -ML, -ML + 1, -2, -1, 0, 1, ML - 1, ML, ML + 1, 10 ** 6 + 3, -(10 ** 6) - 3, 2 ** 62 - 1, -(2 ** 62)]
        got = [int(v) for v in subprocess.check_output([exe, "slots", str(ML)] + [str(t) for t in ts]).decode().split()]
        assert got == [ac.ring_slot(t, ML) for t in ts] and all(0 <= v < ML for v in got), ML
    for n, a, Lp in ((1, 1, 4), (1, 0, 4), (300, 300, 4), (300, 5, 4), (7, 7, 512), (7, 6, 512)):
        js = list(range(1, Lp + 2))
        got = subprocess.check_output([exe, "hist", str(n), str(a), str(Lp)] + [str(j) for j in js]).decode().split()
        assert got == ["-" if ac.hist_time(n, a, j, Lp) is None else str(ac.hist_time(n, a, j, Lp)) for j in js]


def test_slot_arithmetic_at_negative_times(harness):
    _hold_slots(harness)
    for ML, t0, n in ((5, 0, 1), (5, 1, 2), (5, 4, 300), (5, 5, 3), (5, 6, 5), (17, 10 ** 6 + 3, 64), (2, 0, 1), (1, 7, 3), (3, 1, 1)):
        ac.check_slots(ML, t0, n)   # (queues younger than the ring: t0 + t < 0 for the oldest columns)


def test_plan_refusals(harness):
    assert "2^62" in _run_plan(harness, 2, 3, 2, 32, 32, 2, 8, [2 ** 62 - 8], [4, 8])[0]
    assert not isinstance(_run_plan(harness, 2, 3, 2, 32, 32, 2, 8, [2 ** 62 - 9], [4, 8])[0], str)
    assert _run_plan(harness, 2, 3, 2, 32, 32, 2, 2 ** 30, [5])[0] == "REFUSED too many rows"
    assert "2^31" in _run_plan(harness, 2, 3, 2, 32, 32, 3, 2 ** 30, [5], [2 ** 30, 2 ** 30, 5])[0]
    assert "outside" in _run_plan(harness, 2, 3, 2, 32, 32, 2, 8, [5], [4, 9])[0]


# ---------------------------------------------------------------- the binding
def test_the_entry_point_is_declared_bound_and_optional():
    hdr = open(os.path.join(ROOT, "include", "wn_abi.h")).read()
    assert re.search(r"\bint wn_prime_append\(wn_handle\* h, const int32_t\* samples, const int64_t\* n_append,\s+int64_t row_stride, int32_t shared, void\* hip_stream\);", hdr)
    assert "#define WN_ABI_VERSION 5" in hdr and _abi.ABI_VERSION == 5 and "2^62" in hdr
    assert NAME in _abi.EXPORTS and NAME in _abi.OPTIONAL_EXPORTS and NAME in _abi.LAZY_EXPORTS and len(_abi.Library._LAZY_ARGTYPES[NAME]) == 6
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = double_library()
    assert lib.missing == ("wn_score",) and not lib.has(NAME)
    assert NAME not in open(os.path.join(ROOT, "tests", "double", "wn_abi_double.cpp")).read()


def test_the_product_library_checks_its_arguments_before_any_hip_call():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
    import build
    lib = _abi.Library(build.build_hip())
    assert lib.has(NAME)
    buf = np.zeros(8, np.int32)
    n = (_abi.ctypes.c_int64 * 2)(1, 2)
    assert lib.dll.wn_prime_append(None, buf.ctypes.data, n, 4, 0, None) == _abi.WN_E_BADARG and "wn_prime_append: NULL argument" in lib.last_error()


def test_engine_prime_append_on_a_library_without_the_symbol():
    eng = engine.Engine(TINY, synth.init_weights(TINY, seed=1), n_streams=2, **double_backend())
    assert eng.prime_append([[1, 2, 3], [4]]) is False and eng.prime_append([[], []]) is False and eng.prime_append([1, 2, 3], shared=True) is False
    for bad, kw, what in (([[1, 2]], {}, "one row per stream"), ([[1], [2], [3]], {}, "one row per stream"), ([[1], [[2]]], {}, "1-D"), ([[1], [300]], {}, "classes"),
                          (np.zeros((2, 3), np.int64), {}, "list or tuple"), ([[1], [2]], {"shared": True}, "1-D"), ([1, 300], {"shared": True}, "classes")):
        with pytest.raises(ValueError, match=what):
            eng.prime_append(bad, **kw)
    eng.close()


# ---------------------------------------------------------------- the facade on a fake engine
class _Lib:
    path = "<fake>"
    missing = ()

    def has(self, name):
        return name not in self.missing


def _install(monkeypatch, missing=(), accept_append=True):
    """a tiny model whose engines record prime_host / prime_ragged / prime_shared / prime_append / state_load / generate and compute nothing"""
    log = []

    class Fake(FakeEngine):
        def __init__(self, cfg, weights, n_streams=1, device_index=0, **kw):
            super().__init__(cfg, weights, n_streams, device_index, **kw)
            self.lib = _Lib()
            self.lib.missing = tuple(missing)

        def state_load(self, state, stream_first=0, stream_count=None):
            log.append(["state_load", self.n_streams, int(stream_first), stream_count])

        def prime_ragged(self, prompts):
            log.append(["prime_ragged", [len(p) for p in prompts]])
            return bool(self.accept_prime)

        def prime_shared(self, row):
            log.append(["prime_shared", len(row)])
            return bool(self.accept_prime)

        def prime_append(self, prompts, shared=False):
            log.append(["prime_append", len(prompts) if shared else [len(p) for p in prompts], bool(shared)])
            return accept_append and NAME not in missing
    Fake.log, Fake.accept_prime = log, True
    monkeypatch.setattr(engine, "Engine", Fake)
    m = wavenet_model.WaveNetModel(output_length=8, **TINY)
    monkeypatch.setattr(m, "_stream_state", lambda eng, stream, last_index, evals: (stream, last_index, evals))
    return m, log


def test_append_argument_errors(monkeypatch):
    m = wavenet_model.WaveNetModel(output_length=4, **TINY)
    st = _some_state()
    for call in (lambda: m.generate_fast(4, append=[1, 2]), lambda: m.generate_fast(4, first_samples=[3], append=[1, 2]),
                 lambda: m.generate_fast_streams(4, [1.0], append=[1, 2]), lambda: m.score_continuation(np.zeros(4, np.int64), append=[1, 2])):
        with pytest.raises(ValueError, match="needs continue_from"):
            call()
    with pytest.raises(ValueError, match="first_samples must not be given"):   # the existing error stands
        m.generate_fast(4, first_samples=[3], continue_from=st, append=[1])
    for states, bad, what in ((st, [[1], [2]], "1-D"), (st, [1, 256], "classes"), (st, [-1], "classes"), (st, [1.5], "integers"), ([st, st], [[1]], "2 state"),
                              ([st, st], [1, 2], "1-D"), ([st, st], np.zeros((2, 3), np.int64), "a list of them"), ([st, st], [[1], [2], [3]], "3 sequence"),
                              ([st], [[1], [2]], "2 sequence")):
        with pytest.raises(ValueError, match=what):
            m.generate_fast(4, continue_from=states, append=bad)
    with pytest.raises(ValueError, match="ONE state"):
        m.generate_fast_streams(4, [1.0, 0.5], continue_from=[st, st], append=[1])
    with pytest.raises(ValueError, match="append is one 1-D sequence"):
        m.advance_state(st, None)
    assert m._wn_engine is None   # nothing was built on the way


def test_append_on_the_fake_engine(monkeypatch):
    """what the facade asks of the engine, the evals arithmetic, the shapes, the RNG's consumption"""
    m, log = _install(monkeypatch)
    one, two = _some_state(9), _some_state(4)
    np.random.seed(3)
    audio, state = m.generate_fast(5, continue_from=one, append=[7, 8, 9], return_state=True)
    drawn = np.random.random_sample()
    np.random.seed(3)
    np.random.random_sample((1, 5))
    assert np.random.random_sample() == drawn, "no uniform is consumed for appended samples"
    assert audio.shape == (5,) and state == (0, 0, 9 + 3 + 5)
    assert log == [["state_load", 1, 0, 1], ["prime_append", [3], False], ["generate", 5, 1, [1, 5], False, None, None]]   # rows [200, 7, 8]: then from 9
    del log[:]
    audio, states = m.generate_fast(5, continue_from=[one, two, one], append=[[7, 8, 9], [], torch.tensor([4])], return_state=True, temperature=0)
    assert audio.shape == (3, 5) and states == [(0, 0, 9 + 3 + 5), (1, 0, 4 + 0 + 5), (2, 0, 9 + 1 + 5)]
    assert log[:4] == [["state_load", 3, 0, 1], ["state_load", 3, 1, 1], ["state_load", 3, 2, 1], ["prime_append", [3, 0, 1], False]] and log[4][:3] == ["generate", 5, 1]
    del log[:]
    assert m.generate_fast(0, continue_from=one, append=[]).shape == (0,) and log == [["state_load", 1, 0, 1], ["prime_append", [0], False]]
    del log[:]
    assert m.advance_state(one, [1, 2]) == (0, 2, 9 + 2) and m.advance_state([one, two], [[1, 2], []]) == [(0, 2, 11), (1, 200, 4)]
    assert [e[0] for e in log] == ["state_load", "prime_append", "state_load", "state_load", "prime_append"]
    del log[:]
    rows = m.generate_fast_streams(4, [1.0, 0.0, 0.5], continue_from=one, append=[5, 6])
    assert rows.shape == (3, 4) and log[:2] == [["state_load", 3, 0, None], ["prime_append", 2, True]] and log[2][:3] == ["generate", 4, 1] and len(log) == 3
    del log[:]
    lp = m.score_continuation(np.arange(6), continue_from=one, append=[5, 6])
    assert lp.shape == (6,) and [e[0] for e in log] == ["state_load", "prime_append", "generate"] and log[2][5][:1] == [1]   # forced rows (1, 6)


def test_the_fallback_order(monkeypatch):
    """the batched pass is asked first; where it declines, one stream (or the shared row) goes through the chain on the job's engine, a list stream by
    stream through a one-stream engine: load, prime through the chain, save, load into the job's engine -- streams that append nothing are left alone"""
    m, log = _install(monkeypatch, accept_append=False)
    one = _some_state(9)
    m.generate_fast(5, continue_from=one, append=[7, 8, 9], temperature=0)
    assert log[:3] == [["state_load", 1, 0, 1], ["prime_append", [3], False], ["generate", 0, 4, None, False, None, None]] and log[3][:3] == ["generate", 5, 1]
    assert m._wn_last_prime_batched is False
    del log[:]
    m.generate_fast(5, continue_from=[one, one, one], append=[[7, 8], [], [4]], temperature=0)
    assert log[:4] == [["state_load", 3, 0, 1], ["state_load", 3, 1, 1], ["state_load", 3, 2, 1], ["prime_append", [2, 0, 1], False]]
    assert log[4:10] == [["state_load", 1, 0, None], ["generate", 0, 3, None, False, None, None], ["state_load", 3, 0, 1],
                         ["state_load", 1, 0, None], ["generate", 0, 2, None, False, None, None], ["state_load", 3, 2, 1]]
    assert log[10][:3] == ["generate", 5, 1] and len(log) == 11
    del log[:]
    m.generate_fast_streams(4, [1.0, 0.0], continue_from=one, append=[5, 6])
    assert log[:3] == [["state_load", 2, 0, None], ["prime_append", 2, True], ["generate", 0, 3, None, False, None, None]] and log[3][:3] == ["generate", 4, 1]
    del log[:]
    m2, log2 = _install(monkeypatch, missing=(NAME,))   # an older library: the same road
    m2.generate_fast(5, continue_from=one, append=[7, 8, 9], temperature=0)
    assert [e[0] for e in log2] == ["state_load", "prime_append", "generate", "generate"]


def test_prime_piece_samples_cuts(monkeypatch):
    m, log = _install(monkeypatch)
    prompts = [np.arange(n) % 256 for n in (9, 3, 6, 5, 1)]   # to prime: 8, 2, 5, 4, 0 samples
    m.generate_fast(2, first_samples=prompts, temperature=0)
    today = [list(e) for e in log]
    assert today[0] == ["prime_ragged", [8, 2, 5, 4, 0]] and [e[0] for e in today] == ["prime_ragged", "generate"]
    for p, want in ((4, [["prime_ragged", [4, 2, 4, 4, 0]], ["prime_append", [4, 0, 1, 0, 0], False]]),        # boundaries at p and p + 1, streams shorter than p
                    (3, [["prime_ragged", [3, 2, 3, 3, 0]], ["prime_append", [3, 0, 2, 1, 0], False], ["prime_append", [2, 0, 0, 0, 0], False]]),
                    (8, [["prime_ragged", [8, 2, 5, 4, 0]]]), (100, [["prime_ragged", [8, 2, 5, 4, 0]]])):
        del log[:]
        m.prime_piece_samples = p
        m.generate_fast(2, first_samples=prompts, temperature=0)
        assert log[:-1] == want and log[-1] == today[-1], p
    del log[:]
    m.prime_piece_samples = None
    m.generate_fast(2, first_samples=prompts, temperature=0)
    assert log == today, "None issues exactly today's calls"
    # the 2-D prompt and the shared prompt of generate_fast_streams: from Engine.PRIME_BATCH_MIN samples on, as today
    first = torch.zeros((2, 151), dtype=torch.int64)
    del log[:]
    m.generate_fast(2, first_samples=first, temperature=0)
    today = [list(e) for e in log]
    assert today[0] == ["prime_host", [2, 150]]
    m.prime_piece_samples = 64
    del log[:]
    m.generate_fast(2, first_samples=first, temperature=0)
    assert log[:-1] == [["prime_host", [2, 64]], ["prime_append", [64, 64], False], ["prime_append", [22, 22], False]] and log[-1] == today[-1]
    del log[:]
    m.generate_fast(2, first_samples=first[:, :40], temperature=0)   # below the threshold the chain primes, in one job
    assert log and all(e[0] == "generate" for e in log)
    del log[:]
    m.generate_fast_streams(2, [0.0, 0.0], first_samples=first[0])
    assert log[:3] == [["prime_shared", 64], ["prime_append", 64, True], ["prime_append", 22, True]] and log[3][:3] == ["generate", 2, 1] and len(log) == 4
    with pytest.raises(ValueError, match="prime_piece_samples"):
        m.prime_piece_samples = 0
        m.generate_fast(2, first_samples=first, temperature=0)
    m.prime_piece_samples = 64
    m2, log2 = _install(monkeypatch, missing=(NAME,))   # a library without the symbol: one pass, as today
    m2.prime_piece_samples = 64
    m2.generate_fast(2, first_samples=first, temperature=0)
    assert log2[0] == ["prime_host", [2, 150]]

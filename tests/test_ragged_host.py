"""CPU: batched priming without a GPU.  The row plan of wn_prime_ragged (csrc/wn_plan.h: wn_prime_ragged_plan_host) and the pass plan of all three
priming forms (wn_prime_plan_host) compiled with g++ and held to their Python restatement (tests/ragged_cases.py) over a sweep of length sets, once
more under AddressSanitizer / UBSan; the binding; and how the engine and the facade normalise a list of prompts (on the test double of the C ABI,
which has no wn_prime_ragged and stays as it is)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ragged_cases as rc
import wavenet_model
from double_lib import double_backend, double_library
from mi355_wavenet import _abi, engine, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-wavenet_amd", "csrc")
TINY = synth.CONFIGS["tiny"]

HARNESS = r"""
#include "wn_plan.h"
#include <cstdio>
#include <cstdlib>
// <kernel_size> <layers> <blocks> <n, or -1: the longest> <length>... -> "need ...", then one line per table: "<total> | start[0] .. start[ns]", or "REFUSED why"
int main(int argc, char** argv) {
    const int k = atoi(argv[1]), layers = atoi(argv[2]), blocks = atoi(argv[3]);
    long long n = atoll(argv[4]);
    std::vector<int32_t> dil;
    for (int b = 0; b < blocks; ++b) for (int i = 0; i < layers; ++i) dil.push_back(1 << i);
    std::vector<int64_t> len;
    for (int i = 5; i < argc; ++i) len.push_back(atoll(argv[i]));
    if (n < 0) { n = 0; for (int64_t v : len) n = v > n ? v : n; }
    WnRaggedPlan p;
    const std::string why = wn_prime_ragged_plan_host(dil.data(), (int)dil.size(), k, len.data(), (int)len.size(), n, p);
    if (!why.empty()) { printf("REFUSED %s\n", why.c_str()); return 0; }
    printf("need");
    for (long long v : p.need) printf(" %lld", v);
    printf("\n");
    for (int t = 0; t < p.n_tables; ++t) {
        printf("%lld |", p.total[t]);
        for (int s = 0; s <= p.ns; ++s) printf(" %d", p.table(t)[s]);
        printf("\n");
        for (int s = 0; s < p.ns; ++s)   // the accessors against the table
            if (p.rows(t, s) != p.table(t)[s + 1] - p.table(t)[s] || p.first_time(t, s) != p.n - p.rows(t, s)) { printf("ACCESSOR\n"); return 1; }
    }
    return 0;
}
"""

PASS_HARNESS = r"""
#include "wn_plan.h"
#include <cstdio>
#include <cstdlib>
// <kernel_size> <layers> <blocks> <R> <D> <ns> <n> [<length> x ns: the ragged form's argument; none: NULL] -> "pass Lp Lt x_floats z_floats total_floats
// rectangle start_rows", "need ...", one line per layer "ML fill_cols M entries rows t0 z_rows", then (ragged) the tables as above; or "REFUSED why"
int main(int argc, char** argv) {
    const int k = atoi(argv[1]), layers = atoi(argv[2]), blocks = atoi(argv[3]), R = atoi(argv[4]), D = atoi(argv[5]), ns = atoi(argv[6]);
    const long long n = atoll(argv[7]);
    std::vector<int32_t> dil;
    for (int b = 0; b < blocks; ++b) for (int i = 0; i < layers; ++i) dil.push_back(1 << i);
    std::vector<int64_t> len;
    for (int i = 8; i < argc; ++i) len.push_back(atoll(argv[i]));
    if (!len.empty() && (int)len.size() != ns) { printf("USAGE\n"); return 1; }
    WnPrimePlan p;
    const std::string why = wn_prime_plan_host(dil.data(), (int)dil.size(), k, R, D, len.empty() ? nullptr : len.data(), ns, n, p);
    if (!why.empty()) { printf("REFUSED %s\n", why.c_str()); return 0; }
    if (p.ns != ns || p.NL != (int)dil.size() || p.n != n || (int)p.layer.size() != p.NL) { printf("FIELDS\n"); return 1; }
    printf("pass %lld %lld %zu %zu %zu %d %lld\nneed", p.Lp, p.Lt, p.x_floats, p.z_floats, p.total_floats, p.rectangle ? 1 : 0, p.start_rows);
    for (long long v : p.need) printf(" %lld", v);
    printf("\n");
    for (const WnPrimeLayer& y : p.layer) printf("%d %d %lld %lld %lld %lld %lld\n", y.ML, y.fill_cols, y.M, y.entries, y.rows, y.t0, y.z_rows);
    for (int t = 0; !p.rectangle && t < p.ragged.n_tables; ++t) {
        printf("%lld |", p.ragged.total[t]);
        for (int s = 0; s <= p.ragged.ns; ++s) printf(" %d", p.ragged.table(t)[s]);
        printf("\n");
    }
    return 0;
}
"""


def _build(tmp, flags, name, source=HARNESS):
    src = tmp / (name + ".cpp")
    src.write_text(source)
    exe = tmp / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("ragged"), [], "ragged_harness")


def _run(exe, k, layers, blocks, lengths, n=-1):
    out = subprocess.check_output([exe, str(k), str(layers), str(blocks), str(n)] + [str(v) for v in lengths]).decode().splitlines()
    if out[0].startswith("REFUSED"):
        return out[0]
    need = [int(v) for v in out[0].split()[1:]]
    tables = [[int(v) for v in line.split("|")[1].split()] for line in out[1:]]
    totals = [int(line.split("|")[0]) for line in out[1:]]
    return need, tables, totals


def _hold_to_restatement(exe):
    cases = rc.host_sweep()
    assert len(cases) >= 90
    for k, layers, blocks, lengths in cases:
        dil = rc.dilations(layers, blocks)
        want = rc.plan(dil, k, lengths)
        need, tables, totals = _run(exe, k, layers, blocks, lengths)
        assert need == want["need"] and tables == want["start"] and totals == want["total"], (k, layers, blocks, lengths)
        rc.check_plan(want, dil, k, lengths)
        assert totals[0] == sum(lengths)
        if len(set(lengths)) == 1 and lengths[0] > 0:   # equal lengths: wn_prime's own rows, m -> (m / rows, n - rows + m % rows)
            q = rc.prime_rows(dil, k, lengths[0])
            for t in range(1, len(dil)):
                assert tables[t] == [s * q[t] for s in range(len(lengths) + 1)]
            assert tables[0] == [s * lengths[0] for s in range(len(lengths) + 1)]


def test_row_plan_against_the_restatement(harness):
    _hold_to_restatement(harness)


def test_row_plan_right_aligned_to_a_later_time(harness):
    """a member of a front whose own streams are all shorter than the job's n: same rows, later times"""
    dil = rc.dilations(3, 2)
    for lengths, n in (([1, 4, 0, 9], 300), ([0, 0], 5), ([7, 7], 8)):
        need, tables, totals = _run(harness, 2, 3, 2, lengths, n)
        want = rc.plan(dil, 2, lengths, n)
        assert tables == want["start"] == rc.plan(dil, 2, lengths)["start"]
        rc.check_plan(want, dil, 2, lengths)


def test_row_plan_refusals(harness):
    assert "outside" in _run(harness, 2, 3, 2, [4, -1])
    assert "outside" in _run(harness, 2, 3, 2, [4, 9], n=8)
    assert "2^31" in _run(harness, 2, 3, 2, [2 ** 30, 2 ** 30, 5])
    ok = _run(harness, 2, 3, 2, [2 ** 29, 2 ** 29, 5])   # 3 * 2^29 rows: below the bound
    assert ok[2][0] == 2 ** 30 + 5


def test_row_plan_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "ragged_harness_san")
    _hold_to_restatement(exe)
    assert "2^31" in _run(exe, 2, 3, 2, [2 ** 30, 2 ** 30, 5])


# ---------------------------------------------------------------- the pass plan of all three forms
LAYER_KEYS = ("ML", "fill_cols", "M", "entries", "rows", "t0", "z_rows")


@pytest.fixture(scope="module")
def pass_harness(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("prime_pass"), [], "pass_harness", PASS_HARNESS)


def _run_pass(exe, k, layers, blocks, R, D, ns, n, lengths=None):
    """-> the plan in the form of rc.pass_plan (ragged: its start and total), or the refusal line"""
    out = subprocess.check_output([exe] + [str(v) for v in (k, layers, blocks, R, D, ns, n)] + [str(v) for v in lengths or ()]).decode().splitlines()
    if out[0].startswith("REFUSED"):
        return out[0]
    head, NL = [int(v) for v in out[0].split()[1:]], layers * blocks
    p = dict(zip(("Lp", "Lt", "x_floats", "z_floats", "total_floats", "rectangle", "start_rows"), head), ns=ns, n=n)
    p["rectangle"] = bool(p["rectangle"])
    p["need"] = [int(v) for v in out[1].split()[1:]]
    p["layer"] = [dict(zip(LAYER_KEYS, (int(v) for v in line.split()))) for line in out[2:2 + NL]]
    tables = out[2 + NL:]
    assert len(tables) == (0 if p["rectangle"] else NL)
    p["ragged"] = None if p["rectangle"] else dict(start=[[int(v) for v in line.split("|")[1].split()] for line in tables], total=[int(line.split("|")[0]) for line in tables])
    return p


def _hold_pass(exe, k, layers, blocks, R, D, ns, n, lengths=None):
    dil = rc.dilations(layers, blocks)
    want, got = rc.pass_plan(dil, k, R, D, lengths, ns, n), _run_pass(exe, k, layers, blocks, R, D, ns, n, lengths)
    case = (k, layers, blocks, R, D, ns, n, lengths)
    assert not isinstance(got, str), (case, got)
    for key in got:
        if key != "ragged":
            assert got[key] == want[key], (case, key)
    assert (got["ragged"] is None) == (want["ragged"] is None) == want["rectangle"], case
    if not want["rectangle"]:
        assert got["ragged"]["start"] == want["ragged"]["start"] and got["ragged"]["total"] == want["ragged"]["total"], case
        rc.check_plan(want["ragged"], dil, k, lengths)
    rc.check_pass_plan(want, dil, k, R, D)
    return want


# (k, layers, blocks, ns, n, lengths): the shared form and wn_prime (no lengths) at n = 1 and below / at / above the largest ring (MINI3's: 5, 9, 13 for
# k = 2, 3, 4) and the receptive field; wn_prime_ragged with equal lengths, with a stream of every kind, and as a front member whose streams are all shorter
PASS_CASES = [(k, 3, 2, ns, n, None) for k in (2, 3, 4) for ns in (1, 3) for n in (1, 4 * (k - 1), 4 * (k - 1) + 1, 4 * (k - 1) + 2, 14 * (k - 1) + 1, 300)]
PASS_CASES += [(k, 3, 2, 3, n, [n] * 3) for k in (2, 3, 4) for n in (1, 4 * (k - 1) + 1, 300)]
PASS_CASES += [(k, 3, 2, len(rc.MINI3_LENGTHS), 300, rc.MINI3_LENGTHS) for k in (2, 3, 4)]
PASS_CASES += [(k, 3, 2, len(v), n, v) for k in (2, 3, 4) for v, n in (([1, 4, 0, 9], 300), ([0, 0], 5), ([7, 7], 8), ([0, 1], 1))]
PASS_CASES += [(2, 10, 5, 64, 5115, None), (2, 10, 5, 1, 5115, None), (2, 1, 1, 2, 7, None), (4, 1, 1, 2, 3, [3, 2])]


def _hold_pass_to_restatement(exe):
    for k, layers, blocks, ns, n, lengths in PASS_CASES:
        _hold_pass(exe, k, layers, blocks, 32, 64, ns, n, lengths)
    for k, layers, blocks, lengths in rc.host_sweep():   # every length set as the ragged form's argument, and its rectangle (every stream at the longest length)
        n = max(lengths)
        _hold_pass(exe, k, layers, blocks, 128, 128, len(lengths), n, lengths)
        _hold_pass(exe, k, layers, blocks, 128, 128, len(lengths), n)


def test_pass_plan_against_the_restatement(pass_harness):
    _hold_pass_to_restatement(pass_harness)


def test_pass_plan_in_numbers(pass_harness):
    """MINI3 (rings 2, 3, 5): the rectangle's trailing rows, the ragged form's (stream, time) maps, the same workspace"""
    rect = _hold_pass(pass_harness, 2, 3, 2, 128, 128, 9, 300)
    assert (rect["Lp"], rect["Lt"], rect["total_floats"]) == (4, 304, 2 * 9 * 304 * 128 + 9 * 300 * 128) and rect["need"] == [15, 14, 12, 8, 7, 5, 0]
    assert [(y["fill_cols"], y["entries"], y["rows"], y["t0"], y["z_rows"]) for y in rect["layer"]] == [
        (2, 9, 14, 286, 14), (3, 9, 12, 288, 12), (5, 9, 8, 292, 8), (2, 9, 7, 293, 7), (3, 9, 5, 295, 5), (5, 0, 0, 0, 0)]
    rag = _hold_pass(pass_harness, 2, 3, 2, 128, 128, 9, 300, rc.MINI3_LENGTHS)
    assert not rag["rectangle"] and rag["start_rows"] == sum(rc.MINI3_LENGTHS) and rag["total_floats"] == rect["total_floats"]
    assert [(y["entries"], y["rows"], y["t0"], y["z_rows"]) for y in rag["layer"][:2]] == [(1, 0 + 1 + 2 + 4 + 5 + 4 * 14, 0, 300), (1, 0 + 1 + 2 + 4 + 5 + 4 * 12, 0, 300)]
    assert [y["fill_cols"] for y in rag["layer"]] == [y["fill_cols"] for y in rect["layer"]]
    one = _hold_pass(pass_harness, 2, 3, 2, 128, 128, 3, 1)   # n = 1: one column per ring, one row per product, no tap inside the stream
    assert [(y["fill_cols"], y["rows"], y["t0"]) for y in one["layer"][:-1]] == [(1, 1, 0)] * 5
    equal = _hold_pass(pass_harness, 2, 3, 2, 128, 128, 9, 300, [300] * 9)   # equal lengths through wn_prime_ragged: the rectangle, no tables
    assert equal["rectangle"] and equal["layer"] == rect["layer"] and equal["ragged"] is None


def test_pass_plan_refusals(pass_harness):
    assert _run_pass(pass_harness, 2, 3, 2, 32, 32, 2, 2 ** 30) == "REFUSED too many rows"                       # the rectangle's text, as wn_prime gives it
    assert _run_pass(pass_harness, 2, 3, 2, 32, 32, 2, 2 ** 30, [2 ** 30] * 2) == "REFUSED too many rows"        # ... also through wn_prime_ragged
    assert "2^31" in _run_pass(pass_harness, 2, 3, 2, 32, 32, 3, 2 ** 30, [2 ** 30, 2 ** 30, 5])                 # the row plan's own
    assert "outside" in _run_pass(pass_harness, 2, 3, 2, 32, 32, 2, 8, [4, 9]) and "outside" in _run_pass(pass_harness, 2, 3, 2, 32, 32, 2, 8, [-1, 8])
    ok = _run_pass(pass_harness, 2, 3, 2, 32, 32, 3, 2 ** 29)   # 3 * 2^29 rows: below the bound
    assert ok["total_floats"] == 2 * 3 * (2 ** 29 + 4) * 32 + 3 * 2 ** 29 * 32


def test_pass_plan_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "pass_harness_san", PASS_HARNESS)
    _hold_pass_to_restatement(exe)
    assert _run_pass(exe, 2, 3, 2, 32, 32, 2, 2 ** 30) == "REFUSED too many rows" and "outside" in _run_pass(exe, 2, 3, 2, 32, 32, 2, 8, [4, 9])


def test_the_restatement_finds_rows_like_the_kernels():
    start = [0, 0, 3, 3, 3, 10, 10]
    assert [rc.find(start, m)[0] for m in range(10)] == [1, 1, 1, 4, 4, 4, 4, 4, 4, 4]
    p = rc.plan(rc.MINI3_DIL, 2, rc.MINI3_LENGTHS)
    assert p["n"] == 300 and p["total"][0] == sum(rc.MINI3_LENGTHS) and p["need"] == [15, 14, 12, 8, 7, 5, 0]   # need[0] = the receptive field
    rc.check_plan(p, rc.MINI3_DIL, 2, rc.MINI3_LENGTHS)


# ---------------------------------------------------------------- the binding
def test_the_entry_point_is_declared_bound_and_optional():
    hdr = open(os.path.join(ROOT, "include", "wn_abi.h")).read()
    assert re.search(r"\bint wn_prime_ragged\(wn_handle\* h, const int32_t\* first_samples, const int64_t\* n_prime, int64_t row_stride, void\* hip_stream\);", hdr)
    assert "#define WN_ABI_VERSION 5" in hdr and _abi.ABI_VERSION == 5
    n = "wn_prime_ragged"
    assert n in _abi.EXPORTS and n in _abi.OPTIONAL_EXPORTS and n in _abi.LAZY_EXPORTS and len(_abi.Library._LAZY_ARGTYPES[n]) == 5
    assert n in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = double_library()
    assert lib.missing == ("wn_score",) and not lib.has(n)
    assert n not in open(os.path.join(ROOT, "tests", "double", "wn_abi_double.cpp")).read()


def test_the_product_library_checks_its_arguments_before_any_hip_call():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
    import build
    lib = _abi.Library(build.build_hip())
    assert lib.has("wn_prime_ragged")
    buf = np.zeros(8, np.int32)
    n = (_abi.ctypes.c_int64 * 2)(1, 2)
    assert lib.dll.wn_prime_ragged(None, buf.ctypes.data, n, 4, None) == _abi.WN_E_BADARG and "wn_prime_ragged: NULL argument" in lib.last_error()


# ---------------------------------------------------------------- engine and facade normalisation
def test_what_counts_as_a_list_of_prompts():
    assert not engine.is_ragged_prompt(None) and not engine.is_ragged_prompt([]) and not engine.is_ragged_prompt([3, 4, 5])
    assert not engine.is_ragged_prompt(np.zeros((2, 3), np.int64)) and not engine.is_ragged_prompt(torch.zeros(2, 3, dtype=torch.long))
    assert not engine.is_ragged_prompt([np.int64(3), torch.tensor(4)])
    assert engine.is_ragged_prompt([[1, 2], [3]]) and engine.is_ragged_prompt(([1, 2], torch.tensor([3, 4, 5]))) and engine.is_ragged_prompt([np.arange(3)])
    rows, lengths = engine.ragged_rows([[1, 2], torch.tensor([3, 4, 5]), np.arange(1, dtype=np.int32)], 256)
    assert [r.tolist() for r in rows] == [[1, 2], [3, 4, 5], [0]] and lengths.tolist() == [2, 3, 1] and all(r.dtype == np.int64 for r in rows)
    assert engine.right_aligned(rows).tolist() == [[0, 1, 2], [3, 4, 5], [0, 0, 0]]
    for bad, what in (([[1, 2], [[3]]], "1-D"), ([[1, 2], 3], "1-D"), ([[1.5], [2]], "integers"), ([[1], [256]], "classes"), ([[1], [-1]], "classes"),
                      ([[1], []], "at least 1")):
        with pytest.raises(ValueError, match=what):
            engine.ragged_rows(bad, 256)
    assert engine.ragged_rows([[1], []], 256, min_length=0)[1].tolist() == [1, 0]


def test_engine_prime_ragged_on_a_library_without_the_symbol():
    eng = engine.Engine(TINY, synth.init_weights(TINY, seed=1), n_streams=2, **double_backend())
    assert eng.prime_ragged([[1, 2, 3], [4]]) is False and eng.prime_ragged([[], []]) is False
    for bad, what in (([[1, 2]], "one row per stream"), ([[1], [2], [3]], "one row per stream"), ([[1], [[2]]], "1-D"), ([[1], [300]], "classes"),
                      (np.zeros((2, 3), np.int64), "list or tuple")):
        with pytest.raises(ValueError, match=what):
            eng.prime_ragged(bad)
    eng.close()


def _double_model(monkeypatch):
    m = wavenet_model.WaveNetModel(output_length=4, **TINY)
    real = engine.Engine
    monkeypatch.setattr(engine, "Engine", lambda cfg, weights, n_streams=1, device_index=0, **kw: real(cfg, weights, n_streams=n_streams, device_index=device_index,
                                                                                                       **double_backend(), **kw))
    return m


def test_facade_normalisation_on_the_double(monkeypatch):
    """list versus array versus list of ints; the right-aligned matrix; the states' evals -- with the priming itself replaced (the double saves no state)"""
    m = _double_model(monkeypatch)
    seen = {}

    def fake_prime(eng, rows):
        seen["rows"] = [r.tolist() for r in rows]
        eng.reset()
        m._wn_last_prime_batched = False
        return engine.right_aligned(rows)
    monkeypatch.setattr(m, "_prime_ragged", fake_prime)
    monkeypatch.setattr(m, "_stream_state", lambda eng, stream, last_index, evals: (stream, last_index, evals))
    a = np.arange(12).reshape(2, 6) % 256
    # rows of one length: the 2-D call, which never asks for the ragged pass
    np.random.seed(3)
    as_list = m.generate_fast(5, first_samples=[a[0], torch.from_numpy(a[1])])
    np.random.seed(3)
    as_array = m.generate_fast(5, first_samples=torch.from_numpy(a))
    assert as_list.shape == (2, 5) and np.array_equal(as_list, as_array) and "rows" not in seen
    # a list of plain ints is the 1-D prompt
    np.random.seed(3)
    ints = m.generate_fast(5, first_samples=[1, 2, 3])
    np.random.seed(3)
    assert ints.shape == (5,) and np.array_equal(ints, m.generate_fast(5, first_samples=torch.tensor([1, 2, 3]))) and "rows" not in seen
    # unequal lengths: the job starts from the last column of the right-aligned matrix and draws (streams, n) uniforms
    np.random.seed(3)
    out, states = m.generate_fast(5, first_samples=[[9, 8, 7], (5,), torch.tensor([1, 2])], return_state=True)
    drawn = np.random.random_sample()
    assert seen["rows"] == [[9, 8, 7], [5], [1, 2]] and out.shape == (3, 5)
    assert [st[2] for st in states] == [2 + 5, 0 + 5, 1 + 5] and [st[0] for st in states] == [0, 1, 2]
    np.random.seed(3)
    np.random.random_sample((3, 5))
    assert np.random.random_sample() == drawn, "the RNG's consumption is not that of the 2-D call"
    # generate_fast_streams: one prompt per temperature, else a ValueError; a 1-D prompt stays shared
    seen.clear()
    rows = m.generate_fast_streams(4, [1.0, 0.0], first_samples=[[9, 8, 7], [5]])
    assert rows.shape == (2, 4) and seen["rows"] == [[9, 8, 7], [5]]
    with pytest.raises(ValueError, match="one per temperature"):
        m.generate_fast_streams(4, [1.0, 0.0, 0.5], first_samples=[[9, 8, 7], [5]])
    seen.clear()
    assert m.generate_fast_streams(4, [1.0, 0.0], first_samples=[9, 8, 7]).shape == (2, 4) and "rows" not in seen


def test_facade_argument_errors(monkeypatch):
    m = wavenet_model.WaveNetModel(output_length=4, **TINY)
    from test_generation_state_host import _some_state
    with pytest.raises(ValueError, match="first_samples must not be given"):
        m.generate_fast(4, first_samples=[[1, 2], [3]], continue_from=_some_state())
    for bad, what in (([[1, 2], [[3]]], "1-D"), ([[1, 2], []], "at least 1"), ([[1, 2], [999]], "classes"), ([[1, 2], 3], "1-D")):
        with pytest.raises(ValueError, match=what):
            m.generate_fast(4, first_samples=bad)
    with pytest.raises(ValueError, match="forced"):
        m.generate_fast(4, first_samples=[[1, 2], [3]], forced=np.zeros((3, 4), np.int64))
    with pytest.raises(ValueError, match="one row per prompt"):
        m.score_continuation(np.zeros((3, 4), np.int64), first_samples=[[1, 2], [3]])
    with pytest.raises(ValueError, match="one row per prompt"):
        m.score_continuation(np.zeros(4, np.int64), first_samples=[[1, 2], [3]])
    assert m._wn_engine is None   # nothing was built on the way

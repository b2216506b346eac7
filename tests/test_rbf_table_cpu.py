"""EquiMessage's rbf_proj as a table in u = exp(-d) (csrc/oard_rbf_table.h), the parts that need no GPU:

* the fill / check arithmetic the kernels share with this test through one header - tests/rbf_table/harness.cpp, a program of its own
  built here with g++ under the address and undefined-behaviour sanitizers: the midpoint criterion passes at the reference's betas
  and fails at betas x 16; the interval, fraction and factor of a row hold at the ends of the distance range;
* `FwdPlan::rbf_table` (csrc/oard_plan.h), from tests/rbf_table/plan_harness.cpp: true exactly for the layers whose table is good, in
  an inference call whose EquiMessage shape is the 8-wave streamed fp32 kernel, with the option on."""
import itertools
import math
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
E_W8, E_W4, E_SMALL, E_SMALL_SPLIT, E_B3, E_TRAIN, E_TRAIN_B3 = 2, 3, 4, 5, 6, 7, 8      # EquiShape (oard_plan.h)
RBT_N = 2048


def _build(tmp_path_factory, src):
    exe = str(tmp_path_factory.mktemp("rbf_table") / os.path.splitext(src)[0])
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(HERE, "rbf_table", src)], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build(tmp_path_factory, "harness.cpp")


@pytest.fixture(scope="module")
def plan_harness(tmp_path_factory):
    return _build(tmp_path_factory, "plan_harness.cpp")


def _run(exe, *args):
    res = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
    return res.stdout.split()


def test_midpoint_criterion_passes_at_the_reference_betas_and_fails_at_sixteen_times(harness):
    """2 049 points: 5.8e-8 of a channel's range at the reference's betas, 2.9e-6 with Gaussians four times narrower; the criterion is
    2e-7 (float32 resolution of the direct evaluation, as for the frame-scalar MLP's table)."""
    worst, ok, n = _run(harness, "check", 1, 48)
    print("betas x 1: worst midpoint deviation / range", worst)
    assert float(worst) <= 2e-7 and int(ok) == int(n) == 48
    worst, ok, n = _run(harness, "check", 16, 48)
    print("betas x 16: worst midpoint deviation / range", worst)
    assert float(worst) > 2e-7 and int(ok) < int(n)


def test_interval_fraction_and_factor_at_the_ends_of_the_range(harness):
    def locate(d, cutoff=10.0, mask=1.0):
        f = _run(harness, "locate", float(d).hex(), float(cutoff).hex(), mask)
        return int(f[0]), [float.fromhex(x) for x in f[1:]]
    # d = 0: u = 1 is the end of the LAST interval, fraction 1 - the value is the last point's: weights (0, 0, 1, 0) x envelope 1
    idx, (frac, factor, *w) = locate(0.0)
    assert idx == RBT_N - 1 and frac == 1.0 and factor == 1.0 and w == [0.0, 0.0, 1.0, 0.0]
    # one ulp under the cutoff: still inside - the envelope is the reference's own float64 expression (which rounds to 0 there: the
    # cosine of pi (1 - 1.8e-16) is -1 in float64) -, the interval that of u = exp(-10) * 2048 = 0.093; a little further inside it is positive
    d = math.nextafter(10.0, 0.0)
    idx, (frac, factor, *w) = locate(d)
    assert idx == 0 and factor == 0.5 * (math.cos(d * math.pi / 10.0) + 1.0) and 0.0 <= factor < 1e-12
    assert abs(frac - math.exp(-d) * RBT_N) <= 1e-15
    idx, (frac, factor, *w) = locate(10.0 - 1e-6)
    assert idx == 0 and 0.0 < factor < 1e-12 and all(abs(x) <= factor for x in w) and any(x != 0.0 for x in w)
    # from the cutoff on: factor 0, every weight exactly 0 (the edge's cr is 0 whatever the table holds); the interval stays legal
    for d in (10.0, 10.5, 1e3, 1e300):
        idx, (frac, factor, *w) = locate(d)
        assert 0 <= idx < RBT_N and factor == 0.0 and w == [0.0] * 4, d
    # a masked edge inside the cutoff
    idx, (frac, factor, *w) = locate(1.5, mask=0.0)
    assert 0 <= idx < RBT_N and factor == 0.0 and w == [0.0] * 4
    # every interval boundary from above and below lands in a legal interval with a fraction in [0, 1]
    for k in (1, 2, 1000, RBT_N - 1):
        for d in (math.nextafter(-math.log(k / RBT_N), 0.0), -math.log(k / RBT_N), math.nextafter(-math.log(k / RBT_N), 100.0)):
            idx, (frac, factor, *w) = locate(d)
            assert idx in (k - 1, k) and 0.0 <= frac <= 1.0, (k, d, idx, frac)


def test_value_through_the_row_record_matches_the_float64_sum(harness):
    """The edge kernel's arithmetic (four float32 FMAs on the stored entries with the row's float32 weights) against the float64 sum.
    Bound: the table's own midpoint deviation (<= 2e-7 of the range, checked above) + the rounding of four weights and three FMAs,
    each <= 2^-24 = 6e-8 of a term that is at most the range: 2e-7 + 7 x 6e-8 < 6.5e-7 of the channel's range."""
    for d in (0.3, 0.9, 1.1, 1.54, 2.0, 3.3, 4.75, 6.0, 8.5, 9.9):
        v, ref, rng = map(float, _run(harness, "eval", 1, float(d).hex()))
        print(f"d = {d}: table {v:.9e} float64 {ref:.9e} deviation / range {abs(v - ref) / rng:.2e}")
        assert abs(v - ref) <= 6.5e-7 * rng, (d, v, ref, rng)


def test_plan_takes_the_table_exactly_where_its_condition_holds(plan_harness):
    big, small, tiny = 97152, 600, 300                          # inner edges: throughput shape / demoted by the launch heuristics (latency kernel, its stage-split form)
    cases = []
    for (variant, auto), option, prec, train, A, good in itertools.product(
            [(2, 0), (2, 1), (1, 0), (4, 0)], (0, 1), (0, 2, 4), (0, 1), (big, small, tiny, 0), (0, 0b111111, 0b101010, 0b000001)):
        cases.append(dict(variant=variant, auto_small=4 * auto, auto_tiny=8 * auto, option=option, prec=prec, train=train, conc=4, npb=16,
                          A=A, E=3 * A, layers=6, good=good))
    text = "".join(" ".join(str(c[k]) for k in ("variant", "auto_small", "auto_tiny", "option", "prec", "train", "conc", "npb", "A", "E",
                                                 "layers", "good")) + "\n" for c in cases)
    res = subprocess.run([plan_harness], input=text, capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(cases)
    seen = set()
    n_true = 0
    for c, line in zip(cases, lines):
        f = [int(x) for x in line.split()]
        shape, table, wanted = f[0], f[1:17], f[17]
        seen.add(shape)
        eligible = (not c["train"]) and shape == E_W8 and c["option"] == 1 and c["A"] > 0
        assert wanted == int(eligible), (c, line)
        expect = [int(eligible and l < c["layers"] and (c["good"] >> l) & 1) for l in range(16)]
        assert table == expect, (c, line)
        n_true += sum(table)
        # the shape is what the case was built to reach: the table is never taken off the 8-wave streamed fp32 inference kernel
        if c["train"] or c["prec"] & 2 or c["variant"] != 2 or (c["auto_small"] and c["A"] in (small, tiny)):
            assert shape != E_W8 and not any(table), (c, line)
    assert {E_W8, E_W4, E_SMALL, E_SMALL_SPLIT, E_B3, E_TRAIN, E_TRAIN_B3} <= seen, seen
    assert n_true > 0

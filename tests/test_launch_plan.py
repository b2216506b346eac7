"""The forward's launch plan (csrc/oard_plan.h): one pure function decides every kernel shape of a call and sub-batch, and forward_impl
and its launchers only switch on the result.  tests/launch_plan/harness.cpp - a program of its own, built here with g++ under the address
and undefined-behaviour sanitizers and run as a child process - prints the plan of every case of a grid; this file restates the rules
independently and compares, then asserts the properties the kernels rely on from both sides (the edge kernel leaves something unwritten
and the node stage must not read it: `msum`, `l0_skip`; the list exists where it is walked: `use_al`).  No GPU."""
import itertools
import os
import subprocess

import pytest

from conftest import LIB_DEFAULTS, SUITE_OPTIONS

HERE = os.path.dirname(os.path.abspath(__file__))
OPTION_ORDER = ["gcl_variant", "equi_variant", "node_variant", "auto_small", "auto_tiny", "small_split", "gcl_persist", "gcl_grid",
                "gcl_skip", "equi_skip", "equi_l0_skip", "gcl_msum"]
# the library's defaults (oard_debug_option / INTEGRATION.md): what FwdOptions{} must hold
DEFAULTS = dict(gcl_variant=2, equi_variant=2, node_variant=1, auto_small=4, auto_tiny=8, small_split=128, gcl_persist=1, gcl_grid=0,
                gcl_skip=1, equi_skip=1, equi_l0_skip=1, gcl_msum=1)
PREC_GCL, PREC_EQUI, PREC_TRAIN = 1, 2, 4                                  # OARD_PREC_* (include/oard.h)
# enum values of oard_plan.h
G_INVALID, G_V0, G_PERSIST, G_RING3, G_W4, G_SMALL, G_B3, G_TRAIN_PERSIST, G_TRAIN_RING3, G_TRAIN_B3 = range(10)
E_INVALID, E_V0, E_W8, E_W4, E_SMALL, E_SMALL_SPLIT, E_B3, E_TRAIN, E_TRAIN_B3 = range(9)
N_V0, N_ROWS, N_LARGE = range(3)
CUS = 256


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(HERE, "launch_plan", "harness.cpp")], check=True)
    return exe


def run_plans(exe, cases):
    """cases: dicts(opt=, prec=, train=, conc=, npb=, A=, E=, CI=, CX=, layers=, scratch=) -> parsed plans, one per case."""
    text = "".join(" ".join(str(int(v)) for v in [*(c["opt"][k] for k in OPTION_ORDER), c["prec"], c["train"], c["conc"], c["npb"], CUS,
                                                  c["A"], c["E"], c["CI"], c["CX"], c["layers"], c["scratch"]]) + "\n" for c in cases)
    res = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(cases)
    plans = []
    for line in lines:
        f = [int(x) for x in line.split()]
        p = dict(zip(["msum", "l0_skip", "use_al", "fill_edges", "init_v1", "scalarize_tiles", "node", "equi"], f[:8]))
        pos, p["gcl"] = 8, []
        for _ in range(4):
            n = f[pos]
            p["gcl"].append([tuple(f[pos + 1 + 6 * i: pos + 7 + 6 * i]) for i in range(n)])      # (r0, r1, s1, s3, shape, grid)
            pos += 1 + 6 * n
        assert pos == len(f)
        plans.append(p)
    return plans


# ---- the rules, restated (from DESIGN.md section 5 and the option table of INTEGRATION.md, not from oard_plan.h) ----------------------------
def gcl_shape(c, n):
    o = c["opt"]
    if c["train"]:
        return G_TRAIN_B3 if c["prec"] & PREC_TRAIN else (G_TRAIN_PERSIST if o["gcl_persist"] else G_TRAIN_RING3)
    tiles = cdiv(n, 16) * c["conc"]
    kind = {2: "throughput", 3: "w4", 6: "latency", 0: "v0"}.get(o["gcl_variant"], "none")
    if kind == "throughput" and tiles <= 1024 * o["auto_small"]:
        kind = "w4"
    if kind in ("throughput", "w4") and tiles <= 512 * o["auto_tiny"]:
        kind = "latency"
    if kind == "throughput":
        if c["prec"] & PREC_GCL:
            return G_B3
        alone = c["conc"] == 1
        return G_PERSIST if o["gcl_persist"] >= 2 or (o["gcl_persist"] == 1 and alone) else G_RING3
    return {"w4": G_W4, "latency": G_SMALL, "v0": G_V0, "none": G_INVALID}[kind]


def gcl_grid(c, shape, n):
    if shape in (G_PERSIST, G_TRAIN_PERSIST):
        half_tiles = cdiv(cdiv(n, 16), 4)
        g = c["opt"]["gcl_grid"]
        if g > 0:
            want = g
        elif g < 0:
            want = cdiv(half_tiles, 2 * -g)
        else:
            want = max(1, CUS // 2) if c["conc"] > 1 else CUS
        return min(half_tiles, want)
    return cdiv(n, {G_SMALL: 16, G_W4: 64, G_V0: 64}.get(shape, 128))


def equi_shape(c):
    o = c["opt"]
    if c["train"]:
        return E_TRAIN_B3 if c["prec"] & PREC_TRAIN else E_TRAIN
    tiles = cdiv(c["A"], 16) * c["conc"]
    kind = {2: "w8", 1: "w4", 4: "latency", 0: "v0"}.get(o["equi_variant"], "none")
    if kind == "w8" and tiles <= 512 * o["auto_small"]:
        kind = "w4"
    if kind in ("w8", "w4") and tiles <= 512 * o["auto_tiny"]:
        kind = "latency"
    if kind == "w8":
        return E_B3 if c["prec"] & PREC_EQUI else E_W8
    if kind == "latency":
        return E_SMALL_SPLIT if c["scratch"] and tiles <= o["small_split"] else E_SMALL
    return {"w4": E_W4, "v0": E_V0, "none": E_INVALID}[kind]


def large_node_stage(c):
    o = c["opt"]
    return (c["train"] or (o["node_variant"] == 1 and o["equi_variant"] != 0)) and c["npb"] > 4


def msum_expected(c):
    """From the inputs alone: every launch the call would make over the column lists, layer by layer, takes the fp32 throughput shape.
    (Every option set of this grid has gcl_skip = 1.  With gcl_skip = 0 the two lists always run as one launch and the plan still judges
    them apart, as the library always has.)"""
    o = c["opt"]
    if c["train"] or not o["gcl_msum"] or c["E"] <= 0 or not large_node_stage(c):
        return False
    sizes = set()
    for l in range(c["layers"]):
        apart = o["gcl_skip"] and (l == 0 or l == c["layers"] - 1)
        sizes |= {c["CI"], c["CX"]} if apart else {c["CI"] + c["CX"]}
    return all(gcl_shape(c, n) in (G_PERSIST, G_RING3) for n in sizes if n > 0)


def expected(c):
    o, train = c["opt"], c["train"]
    v1 = train or (o["node_variant"] == 1 and o["equi_variant"] != 0)
    skip = bool(train or (o["gcl_skip"] and o["gcl_variant"] != 0))
    p = dict(msum=int(msum_expected(c)), fill_edges=int(not skip), init_v1=int(train or o["node_variant"] >= 1),
             scalarize_tiles=int(cdiv(c["A"], 64) * c["conc"] <= 2048), node=(N_V0 if not v1 else N_ROWS if c["npb"] <= 4 else N_LARGE),
             equi=equi_shape(c))
    p["use_al"] = int(not train and bool(o["equi_skip"]) and c["A"] > 0 and o["equi_variant"] != 0 and o["node_variant"] == 1)
    p["l0_skip"] = int(not train and bool(o["equi_l0_skip"]) and c["A"] > 0 and p["equi"] == E_W8 and large_node_stage(c))
    inner, total = (c["CI"], c["CI"] + c["CX"]) if p["msum"] else (c["A"], c["E"])
    p["gcl"] = []
    for kind in range(4):
        first, last = bool(kind & 1), bool(kind & 2)
        if skip and (first or last):
            ranges = [(0, inner, 1, 1), (inner, total, int(not first), int(not last))]
        else:
            ranges = [(0, total, 1, 1)]
        launches = []
        for r0, r1, s1, s3 in ranges:
            if r1 > r0:
                shape = gcl_shape(c, r1 - r0)
                launches.append((r0, r1, s1, s3, shape, gcl_grid(c, shape, r1 - r0)))
        p["gcl"].append(launches)
    return p


# ---- the grid ----------------------------------------------------------------------------------------------------------------------------
def option_sets():
    """(options, precision, train): the suite's and the library's options, each precision bit, the training-mode forward, gcl_persist 0 / 1 /
    2, gcl_grid 0 / 3 / -2."""
    plan_keys = set(OPTION_ORDER)
    out = []
    for base in (SUITE_OPTIONS, LIB_DEFAULTS):
        o = dict(DEFAULTS, **{k: v for k, v in base.items() if k in plan_keys})
        out += [(o, 0, 0), (o, PREC_GCL, 0), (o, PREC_EQUI, 0), (o, PREC_TRAIN, 0), (o, 0, 1), (o, PREC_TRAIN, 1), (o, PREC_GCL | PREC_EQUI, 1)]
        for persist, grid in itertools.product((0, 1, 2), (0, 3, -2)):
            out.append((dict(o, gcl_persist=persist, gcl_grid=grid), 0, 0))
        out += [(dict(o, gcl_persist=0), 0, 1), (dict(o, gcl_grid=3), 0, 1), (dict(o, gcl_grid=-2), 0, 1)]
        out += [(dict(o, gcl_variant=gv, equi_variant=ev), 0, 0) for gv, ev in ((3, 1), (6, 2), (6, 4))]      # the debug variants
    return out


def sizes_for(o, conc):
    """Row / column counts n such that cdiv(n, 16) * conc sits one below, on and one above every threshold the options set, plus 0, 1, 16, 17."""
    out = {0, 1, 16, 17}
    for threshold in (1024 * o["auto_small"], 512 * o["auto_small"], 512 * o["auto_tiny"], o["small_split"]):
        for target in (threshold - 1, threshold, threshold + 1):
            for tiles in {target // conc, cdiv(target, conc)}:
                if tiles > 0:
                    out |= {tiles * 16, tiles * 16 - 15}
    return sorted(out)


def grid_cases():
    cases = []
    for (o, prec, train), conc in itertools.product(option_sets(), (1, 2, 4)):
        if train and conc > 1:
            continue                                          # the training-mode forward is one sub-batch
        sizes = sizes_for(o, conc)
        big = sizes[-1] + 16 * 1024
        # (A, E, CI, CX): every size as the inner list beside a small, an equal and a large inter-object list; CI = 0 and CX = 0 on their own
        shapes = [(n, n + x, n, x) for n in sizes for x in (17, n, big)]
        # (one-atom objects have no inner edge: A = CI = 0; a single object has no inter-object one: CX = 0)
        shapes += [(0, n, 0, n) for n in sizes] + [(n, n, n, 0) for n in sizes] + [(big, 3 * big, big, 2 * big)]
        for i, (A, E, CI, CX) in enumerate(shapes):
            npb, layers = (1, 4, 5, 16)[i % 4], (1, 2, 5)[(i // 4) % 3]
            cases.append(dict(opt=o, prec=prec, train=train, conc=conc, npb=npb, A=A, E=E, CI=CI, CX=CX, layers=layers, scratch=int(i % 5 != 0)))
    # every (npb, num_layers) pair on the sizes around the thresholds
    sets = option_sets()
    picked = [s for s in sets if s[1] == 0 and s[0] in (sets[0][0], sets[len(sets) // 2][0])]        # both bases, inference and training
    for (o, prec, train), npb, layers in itertools.product(picked, (1, 4, 5, 16), (1, 2, 5)):
        for n in sizes_for(o, 1):
            cases.append(dict(opt=o, prec=prec, train=train, conc=1, npb=npb, A=n, E=3 * n, CI=n, CX=2 * n, layers=layers, scratch=1))
    return cases


@pytest.fixture(scope="module")
def planned(harness):
    cases = grid_cases()
    return cases, run_plans(harness, cases)


def test_library_defaults_and_the_unreachable_four_wave_shapes(harness):
    """FwdOptions{} holds the library's defaults.  A fact about them, recorded and not changed here: with auto_small = 4 and auto_tiny = 8
    both GCL thresholds are 4096 tiles (1024 x 4 = 512 x 8) and EquiMessage's are 2048 and 4096, so a launch small enough for the 4-wave
    shape is always small enough for the latency kernel - under the default options the 4-wave shapes of either edge kernel are
    unreachable, only debug options select them."""
    out = subprocess.run([harness, "defaults"], capture_output=True, text=True, check=True).stdout.split()
    assert dict(zip(OPTION_ORDER, map(int, out))) == DEFAULTS
    assert 1024 * DEFAULTS["auto_small"] == 512 * DEFAULTS["auto_tiny"] == 4096 and 512 * DEFAULTS["auto_small"] == 2048
    tiles = sorted(set(range(1, 200, 7)) | set(range(2040, 2056)) | set(range(4088, 4104)) | {1020, 1024, 1025, 3000, 5000, 9000})
    cases = [dict(opt=DEFAULTS, prec=0, train=0, conc=conc, npb=16, A=16 * t, E=48 * t, CI=16 * t, CX=32 * t, layers=3, scratch=1)
             for t in tiles for conc in (1, 2, 4)]
    plans = run_plans(harness, cases)
    shapes = {L[4] for p in plans for launches in p["gcl"] for L in launches}
    assert G_W4 not in shapes and {G_SMALL, G_PERSIST, G_RING3} <= shapes
    assert E_W4 not in {p["equi"] for p in plans} and {E_SMALL, E_SMALL_SPLIT, E_W8} <= {p["equi"] for p in plans}
    # ... and a debug option does select them
    w4 = run_plans(harness, [dict(c, opt=dict(DEFAULTS, auto_tiny=0)) for c in cases])
    assert G_W4 in {L[4] for p in w4 for launches in p["gcl"] for L in launches} and E_W4 in {p["equi"] for p in w4}


def test_plan_equals_the_restated_rules(planned):
    cases, plans = planned
    assert len(cases) > 5000
    for c, p in zip(cases, plans):
        assert p == expected(c), c
    # the grid reaches every product shape these option sets can select (not the 4-wave ones under the default thresholds: see the test above) and both answers of
    # every paired decision
    assert {L[4] for p in plans for launches in p["gcl"] for L in launches} >= set(range(G_PERSIST, G_TRAIN_B3 + 1)) - {G_W4}
    assert {p["equi"] for p in plans} >= set(range(E_W8, E_TRAIN_B3 + 1)) - {E_W4} and {p["node"] for p in plans} == {N_ROWS, N_LARGE}
    for key in ("msum", "l0_skip", "use_al", "scalarize_tiles"):
        assert {p[key] for p in plans} == {0, 1}, key


def layers_of(c, p):
    """The launches of every layer the call has."""
    return [p["gcl"][(1 if l == 0 else 0) | (2 if l == c["layers"] - 1 else 0)] for l in range(c["layers"])]


def test_paired_decisions_hold_from_both_sides(planned):
    """msum, l0_skip and use_al are true exactly where their condition holds - asserted false wherever it is false and true wherever it is
    true; the conditions are evaluated on the inputs (and, for msum, also on the launches the plan lists)."""
    cases, plans = planned
    for c, p in zip(cases, plans):
        o, train = c["opt"], c["train"]
        large = large_node_stage(c)
        assert (p["node"] == N_LARGE) == large
        cond = not train and bool(o["gcl_msum"]) and c["E"] > 0 and large
        assert bool(p["msum"]) == msum_expected(c), c
        every_launch_throughput = all(L[4] in (G_PERSIST, G_RING3) for launches in layers_of(c, p) for L in launches)
        if p["msum"]:
            assert cond and every_launch_throughput, c
        elif cond:       # refused by a launch shape: some launch over the column lists is not a throughput one
            assert not all(gcl_shape(c, n) in (G_PERSIST, G_RING3) for n in (c["CI"], c["CX"]) if n > 0), c
        w8 = equi_shape(c) == E_W8
        assert bool(p["l0_skip"]) == (not train and bool(o["equi_l0_skip"]) and c["A"] > 0 and w8 and large), c
        assert (p["equi"] == E_W8) == w8 and not (train and p["l0_skip"])
        assert bool(p["use_al"]) == (not train and bool(o["equi_skip"]) and c["A"] > 0 and o["equi_variant"] != 0 and o["node_variant"] == 1), c


def test_launches_tile_the_edges_and_grids_are_in_range(planned):
    cases, plans = planned
    for c, p in zip(cases, plans):
        inner, total = (c["CI"], c["CI"] + c["CX"]) if p["msum"] else (c["A"], c["E"])
        for kind, launches in enumerate(p["gcl"]):
            first, last = bool(kind & 1), bool(kind & 2)
            assert len(launches) <= 2
            at = 0
            for r0, r1, s1, s3, shape, grid in launches:
                assert r0 == at and r1 > r0, c                # no gap, no overlap, no empty launch
                at = r1
                inter_object = r0 >= inner
                assert s1 or (inter_object and first), c      # stages are skipped on inter-object ranges of the first / last layer only
                assert s3 or (inter_object and last), c
                assert not (r0 < inner < r1) or (s1 and s3)
                assert shape != G_INVALID and grid >= 1
                if shape in (G_PERSIST, G_TRAIN_PERSIST):
                    assert grid <= cdiv(cdiv(r1 - r0, 16), 4), c      # at most one workgroup per half-tile
            assert at == max(total, 0), c

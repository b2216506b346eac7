"""The two yardsticks of the order-matched RMSD against each other, on the host (tests/_match_cases.py; never loads the library):
the search is bounded below by the exact minimum and above by the same-order RMSD, and it finds the planted permutation (or a better
one) on EVERY planted case that tests/test_match_kernel.py runs on the GPU - a condition on those cases, not a measurement."""
import functools

import numpy as np
import pytest

import _match_cases as mc

SMALL = [(n, c) for n, c in mc.EXACT if n not in mc.NO_REFERENCE]
TIE = 1e-9            # relative: two float64 evaluations of the same permutation


@functools.lru_cache(maxsize=None)
def _case(kind):
    return mc.make_kind(kind)


@pytest.mark.parametrize("reflect", [False, True])
@pytest.mark.parametrize("kind", mc.KINDS)
def test_search_lies_between_exact_and_same_order(kind, reflect):
    case = _case(kind)
    worse = 0
    for g, name in enumerate(mc.NAMES):
        if name in mc.NO_REFERENCE:
            continue
        a, b, sp, _ = mc.segment(case, g)
        e, p, _ = mc.search(a, b, sp, reflect)
        scale = mc.rho(a, b)
        assert sorted(p) == list(range(len(a))) and (sp[p] == sp).all(), name
        assert e <= mc.same_order(a, b, reflect) * (1 + TIE) + 1e-12 * scale, name
        if (name, mc.SEGMENTS[g][1]) in SMALL:
            ex, _ = mc.brute(a, b, sp, reflect)
            assert e >= ex * (1 - TIE) - 1e-12 * scale, (name, e, ex)
            worse += e > ex * (1 + TIE) + 1e-12 * scale
    print(f"{kind} reflect={reflect}: the search is worse than the exact minimum in {worse} of {len(SMALL)} small segments")


# the mirror image is a planted copy only where reflection is allowed
@pytest.mark.parametrize("kind,reflect", [(k, r) for k in sorted(mc.PLANTED) for r in (False, True) if r or k != "mirror"])
def test_search_recovers_every_planted_case_of_the_gpu_test(kind, reflect):
    case = _case(kind)
    most = 0
    for g, name in enumerate(mc.NAMES):
        if name in mc.NO_REFERENCE:
            continue
        a, b, sp, planted = mc.segment(case, g)
        e, _, rounds = mc.search(a, b, sp, reflect)
        want = mc.planted_rmsd(a, b, planted, reflect)
        most = max(most, rounds)
        assert e <= want * (1 + TIE) + 1e-12 * mc.rho(a, b), (kind, name, e, want)
    assert most < mc.ROUNDS, most
    print(f"{kind} reflect={reflect}: most rounds of any run {most}")


def test_brute_is_the_minimum_over_hand_made_permutations():
    rng = np.random.default_rng(5)
    a, b, sp, planted = mc.make_segment("rigid_noise", (3, 2), rng)
    ex, p = mc.brute(a, b, sp, True)
    assert ex <= mc.planted_rmsd(a, b, planted, True) * (1 + TIE)
    assert abs(mc.same_order(a, b[p], True) - ex) <= 1e-12

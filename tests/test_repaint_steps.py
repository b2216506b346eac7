"""`schedule.repaint_steps`: the flat list of (s, jump target) that `DiffusionSampler.inpaint` walks equals the nested loop of the
reference (oa_reactdiff/diffusion/en_diffusion.py:788-853), restated here."""
import pytest

from oareactdiff_amd.schedule import get_repaint_schedule, repaint_steps

CASES = [(1, 1, 7), (2, 3, 12), (5, 5, 50), (3, 2, 1)]


def nested_loop(resamplings, jump_length, timesteps):
    """en_diffusion.py:788-853 without the arithmetic: which s is denoised, and where the state is re-noised to afterwards."""
    visited = []
    schedule = get_repaint_schedule(resamplings, jump_length, timesteps)
    s = timesteps - 1
    for i, n_denoise_steps in enumerate(schedule):
        for j in range(n_denoise_steps):
            target = None
            if j == n_denoise_steps - 1 and i < len(schedule) - 1:
                target = s + jump_length
            visited.append((s, target))
            if target is not None:
                s = target
            s -= 1
    return visited, s


@pytest.mark.parametrize("resamplings,jump_length,timesteps", CASES)
def test_flat_list_is_the_nested_loop(resamplings, jump_length, timesteps):
    want, s_end = nested_loop(resamplings, jump_length, timesteps)
    got = repaint_steps(resamplings, jump_length, timesteps)
    assert got == want
    assert isinstance(got, list) and all(isinstance(e, tuple) and len(e) == 2 for e in got)
    assert s_end == -1 and got[-1] == (0, None)                     # the loop ends on the step to s = 0, which never jumps
    assert got[0][0] == timesteps - 1
    assert all(0 <= s < timesteps and (j is None or (j == s + jump_length and j < timesteps)) for s, j in got)
    assert len(got) == sum(get_repaint_schedule(resamplings, jump_length, timesteps))
    # a pure function: the same list again, and the caller's copy is its own
    got.append(None)
    assert repaint_steps(resamplings, jump_length, timesteps) == want


def test_the_inpaint_test_case_has_21_steps():
    """(2, 3, 12): 21 entries - with the final x | z0 call the 22 network calls tests/test_sampler_loops.py counts."""
    steps = repaint_steps(2, 3, 12)
    assert len(steps) == 21
    assert sum(1 for _, j in steps if j is not None) == 3
    assert repaint_steps(3, 2, 1) == [(0, None)]

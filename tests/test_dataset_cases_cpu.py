"""The numpy emulation of `k_reaction_gather` (tests/_dataset_cases.py) against the reference's collate in every g12 fixture, without a
device: what the GPU tests then hold the kernel to bit for bit is itself held to the reference here."""
import numpy as np
import pytest

from _dataset_cases import CONFIGS, DatasetCase, check_against_reference, center_f64, emulate


@pytest.mark.parametrize("cfg", CONFIGS)
def test_emulation_matches_the_reference_collate(cfg):
    case = DatasetCase(cfg)
    store = case.store()
    assert len(store) == case.n_samples
    whole = np.arange(len(store))
    check_against_reference(case, store, emulate(store, whole), whole, "all")
    check_against_reference(case, store, emulate(store, case.sub_index), case.sub_index, "sub")


def test_fixtures_cover_the_edge_counts_and_switches():
    case = DatasetCase("reflect_append_multi")
    reps, _ = case.expected("all")
    assert sorted(set(reps[0]["size"].tolist())) == [1, 2, 7, 23, 63, 64, 65]
    assert reps[0]["charge"].shape[1] == 2 and len(reps[0]["size"]) == 14
    assert len(DatasetCase("swap_by_ind").expected("all")[0][0]["size"]) == 10
    assert len(DatasetCase("only_ts").expected("all")[0]) == 1
    assert set(DatasetCase("confidence").expected("all")[1]) == {"target", "rmsd", "condition"}


def test_one_atom_centres_to_exact_zero_and_sum_order_is_fixed():
    x = np.array([[5.1, -3.3, 1e6]], dtype=np.float32)
    assert np.all(center_f64(x) == 0.0)
    rng = np.random.default_rng(0)
    y = (3 * rng.standard_normal((130, 3)) + 5).astype(np.float32)
    a, b = center_f64(y), center_f64(y.copy())
    assert np.array_equal(a, b)
    exact = y.astype(np.float64) - y.astype(np.float64).mean(axis=0)
    assert np.all(np.abs(a - exact) <= 2.0 ** -24 * np.abs(exact) + 1e-12)

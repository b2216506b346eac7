"""`k_reaction_gather` through `ReactionStore.batch` / `DeviceLoader` on the device: against the reference's collate in every g12 fixture
(the bounds of tests/_dataset_cases.py), and bit for bit against the numpy emulation on a random store whose three objects have different
atom counts (1, 63, 64, 65, 130 among them)."""
import numpy as np
import pytest
import torch

from _dataset_cases import (CONFIGS, PROPS, RANDOM_COUNTS, RANDOM_SWITCHES, DatasetCase, assert_same, check_against_reference, emulate, random_raw,
                            to_numpy)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _random_store(name):
    from oareactdiff_amd.data import ReactionStore
    return ReactionStore(random_raw(), device=DEV, **RANDOM_SWITCHES[name])


@pytest.mark.parametrize("cfg", CONFIGS)
def test_batch_matches_the_reference_collate(cfg):
    case = DatasetCase(cfg)
    store = case.store(DEV)
    whole = np.arange(len(store))
    for tag, index in (("all", whole), ("sub", case.sub_index)):
        batch = store.batch(index.tolist() if tag == "all" else torch.from_numpy(index))
        reps, res = batch
        for k, r in enumerate(reps):                       # DDPMTrainer.to_device's layout: host copies beside the device tensors
            assert all(r[p].device == DEV for p in PROPS)
            assert r["size_host"].device.type == "cpu" and torch.equal(r["size_host"], r["size"].cpu())
            assert r["mask_host"].device.type == "cpu" and torch.equal(r["mask_host"], r["mask"].cpu())
        got = to_numpy(batch)
        check_against_reference(case, store, got, index, tag)
        assert_same(got, emulate(store, index), f"{cfg} {tag}")


@pytest.mark.parametrize("name", list(RANDOM_SWITCHES))
def test_random_store_is_bitwise_the_emulation(name):
    store = _random_store(name)
    n = len(store)
    rng = np.random.default_rng(5)
    whole = rng.permutation(n)
    assert_same(to_numpy(store.batch(whole)), emulate(store, whole), f"{name} whole")
    for v in (0, n - 1):                                   # B = 1
        assert_same(to_numpy(store.batch([v])), emulate(store, [v]), f"{name} single {v}")
    if store.swap and store.reflect:                       # one batch that mixes original, swapped, reflected and both
        q = store.n_sel
        mixed = [3 * q + 1, 1, q + 1, 2 * q + 1, 0, 4 * q - 1]
        f_bit, s_bit, _ = store.decode(mixed)
        assert {(int(a), int(b)) for a, b in zip(f_bit, s_bit)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert_same(to_numpy(store.batch(mixed)), emulate(store, mixed), f"{name} mixed")


def test_loader_first_nonzero_short_last_batch_and_forty_batches_back_to_back():
    from oareactdiff_amd.data import DeviceLoader
    from oareactdiff_amd.data import ReactionStore
    store = ReactionStore(random_raw(counts=np.tile(RANDOM_COUNTS, (6, 1))), device=DEV, **RANDOM_SWITCHES["swap_reflect"])
    assert len(store) == 232                               # 58 selected reactions x 2 x 2
    loader = DeviceLoader(store, batch_size=5, shuffle=True, seed=2)
    loader.set_epoch(1)
    plan = loader.epoch_plan()
    assert plan.batches[-1] == (230, 2) and len(plan.batches) == len(loader) == 47
    got = list(loader)                                     # one upload, then 47 launches with nothing in between
    torch.cuda.synchronize()
    want = [emulate(store, plan.indices[a: a + b]) for a, b in plan.batches]
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(to_numpy(g), w, f"batch {i}")
    dropped = DeviceLoader(store, batch_size=50, drop_last=True)
    assert [int(b[0][0]["size"].numel()) for b in dropped] == [50] * 4


def test_a_sample_has_the_same_bits_in_any_batch_and_epoch():
    from oareactdiff_amd.data import DeviceLoader
    store = _random_store("swap_reflect")
    v = 2 * store.n_sel + 4                                # a reflected sample of 130 / 64 / 63 atoms

    def rows(batch, b):
        reps, _ = to_numpy(batch)
        out = []
        for r in reps:
            a = int(r["size"][:b].sum())
            out.append({p: r[p][a: a + int(r["size"][b])] for p in ("pos", "one_hot", "charge")})
        return out
    first = rows(store.batch([v, 0, 1]), 0)
    later = rows(store.batch([7, 30, 12, v]), 3)
    for a, b in zip(first, later):
        for p in a:
            assert np.array_equal(a[p].view(np.uint8), b[p].view(np.uint8)), p
    loader = DeviceLoader(store, batch_size=6, shuffle=True, seed=9)
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        plan = loader.epoch_plan()
        at = int(np.nonzero(plan.indices == v)[0][0])
        i = at // 6
        batch = list(loader)[i]
        for a, b in zip(first, rows(batch, at - plan.batches[i][0])):
            for p in a:
                assert np.array_equal(a[p].view(np.uint8), b[p].view(np.uint8)), (epoch, p)


@pytest.mark.parametrize("name", ["swap_reflect", "confidence_swap", "append_multi_key"])
def test_no_poison_survives(name):
    """Outputs allocated with a poison fill: every element is written (0xA5 bytes are no value any output can take)."""
    store = _random_store(name)

    def poisoned(shape, dtype, device):
        t = torch.empty(shape, dtype=dtype, device=device)
        t.view(torch.uint8).fill_(0xA5)
        return t
    store.alloc = poisoned
    index = np.arange(len(store))[::-1].copy()
    batch = store.batch(index)
    got, want = to_numpy(batch), emulate(store, index)
    assert_same(got, want, name)
    poison64, poison32 = np.frombuffer(b"\xa5" * 8, dtype=np.int64)[0], np.frombuffer(b"\xa5" * 4, dtype=np.float32)[0]
    for r in got[0]:
        for p in PROPS:
            assert not np.any(r[p] == (poison32 if p == "pos" else poison64)), p
    for key, val in got[1].items():
        assert not np.any(val == (poison32 if val.dtype == np.float32 else poison64)), key

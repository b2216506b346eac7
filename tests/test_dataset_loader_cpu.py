"""`DeviceLoader.epoch_plan` and the host side of `ReactionStore` without a device: index streams, batch shapes, host layouts, index
decoding, constructor errors and the restricted unpickler."""
import os
import pickle

import numpy as np
import pytest
import torch
from torch.utils.data.distributed import DistributedSampler

from _dataset_cases import RANDOM_SWITCHES, DatasetCase, emulate, random_raw
from oareactdiff_amd.data import DeviceLoader, ReactionStore, load_raw


def _store(name="swap_reflect"):
    return ReactionStore(random_raw(), **RANDOM_SWITCHES[name])


@pytest.mark.parametrize("world_size", [1, 2, 8])
@pytest.mark.parametrize("shuffle", [False, True])
def test_index_stream_is_distributed_samplers(world_size, shuffle):
    store = _store()                                     # 8 selected x 2 x 2 = 32 samples; world size 8 divides, a 9-reaction one below pads
    odd = ReactionStore(random_raw(), swapping_react_prod=True, reflection=True, single_frag_only=False, only_ts=True)   # 40 samples
    for st in (store, odd, ReactionStore(random_raw(), single_frag_only=True)):      # 9 samples: padding by wrapping
        for epoch in (0, 3):
            streams = []
            for rank in range(world_size):
                sampler = DistributedSampler(range(len(st)), num_replicas=world_size, rank=rank, shuffle=shuffle, seed=11, drop_last=False)
                sampler.set_epoch(epoch)
                loader = DeviceLoader(st, batch_size=4, shuffle=shuffle, seed=11, rank=rank, world_size=world_size)
                plan = loader.epoch_plan(epoch)
                assert plan.indices.tolist() == list(sampler)
                loader.set_epoch(epoch)
                assert loader.epoch_plan().indices.tolist() == list(sampler)
                assert len(plan.batches) == len(loader)
                streams.append(plan)
            assert len({len(p.batches) for p in streams}) == 1                      # every rank takes the same number of steps
            assert len({tuple(p.batches) for p in streams}) == 1
            assert set(np.concatenate([p.indices for p in streams]).tolist()) == set(range(len(st)))


def test_last_short_batch_and_drop_last():
    store = _store("plain")                              # 9 samples
    assert len(store) == 9
    keep = DeviceLoader(store, batch_size=4)
    assert keep.epoch_plan(0).batches == [(0, 4), (4, 4), (8, 1)] and len(keep) == 3
    drop = DeviceLoader(store, batch_size=4, drop_last=True)
    assert drop.epoch_plan(0).batches == [(0, 4), (4, 4)] and len(drop) == 2
    exact = DeviceLoader(store, batch_size=3, drop_last=True)
    assert exact.epoch_plan(0).batches == [(0, 3), (3, 3), (6, 3)] and len(exact) == 3
    with pytest.raises(ValueError):
        DeviceLoader(store, batch_size=0)
    with pytest.raises(ValueError):
        DeviceLoader(store, batch_size=2, rank=2, world_size=2)


@pytest.mark.parametrize("name", list(RANDOM_SWITCHES))
def test_host_layout_matches_the_emulation(name):
    store = _store(name)
    loader = DeviceLoader(store, batch_size=5, shuffle=True, seed=3)
    plan = loader.epoch_plan(1)
    table = plan.table()
    assert table.shape == (1 + store.n_obj, plan.indices.size + 1) and table.dtype == np.int64
    assert np.array_equal(table[0, :-1], plan.indices)
    for i, (first, B) in enumerate(plan.batches):
        reps, _ = emulate(store, plan.indices[first: first + B])
        sizes, atoms = plan.size_host(i), plan.atoms(i)
        for k, r in enumerate(reps):
            assert sizes[k].dtype == torch.int64 and np.array_equal(sizes[k].numpy(), r["size"])
            assert atoms[k] == r["mask"].size
            assert np.array_equal(torch.repeat_interleave(torch.arange(B), sizes[k]).numpy(), r["mask"])
            assert np.array_equal(table[1 + k, first: first + B + 1] - table[1 + k, first], np.concatenate([[0], np.cumsum(r["size"])]))


def test_virtual_index_decoding_at_the_block_boundaries():
    store = _store("swap_reflect")
    n = store.n_sel
    assert n == 8 and len(store) == 4 * n and store.sel.tolist() == [0, 1, 2, 3, 4, 6, 8, 9]
    v = [0, n - 1, n, 2 * n - 1, 2 * n, 3 * n - 1, 3 * n, 4 * n - 1]
    f_bit, s_bit, r = store.decode(v)
    assert f_bit.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert s_bit.tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    assert r.tolist() == [0, 9, 0, 9, 0, 9, 0, 9]
    counts = store.counts_of(v)
    raw = random_raw()
    assert counts[0].tolist() == [raw["reactant" if s == 0 else "product"]["num_atoms"][rr] for s, rr in zip(s_bit, r)]
    assert counts[2].tolist() == [raw["product" if s == 0 else "reactant"]["num_atoms"][rr] for s, rr in zip(s_bit, r)]
    for bad in (-1, 4 * n):
        with pytest.raises(IndexError):
            store.decode([bad])


def test_constructor_errors():
    raw = random_raw()
    with pytest.raises(NotImplementedError):
        ReactionStore(raw, pad_fragments=1)
    with pytest.raises(ValueError, match="use_ind"):
        ReactionStore({k: v for k, v in raw.items() if k != "use_ind"}, use_by_ind=True)
    ReactionStore({k: v for k, v in raw.items() if k != "use_ind"}, use_by_ind=True, confidence_model=True)   # confidence forces it off
    bad = random_raw()
    bad["transition_state"]["charges"][2][0] = 16
    with pytest.raises(ValueError, match="atomic number 16"):
        ReactionStore(bad)
    bad["single_fragment"][2] = 0                        # an unselected reaction is never read, as in the reference
    ReactionStore(bad)
    with pytest.raises(ValueError, match="reads past"):
        ReactionStore(raw, confidence_model=True, reflection=True)
    with pytest.raises(ValueError):
        ReactionStore(raw, device="cpu")


def test_files_npz_and_restricted_pickle(tmp_path):
    case = DatasetCase("default")
    flat = {key: case.raw[key] for key in ("single_fragment", "use_ind", "target", "rmsd")}
    for name in ("reactant", "transition_state", "product"):
        for field, val in case.raw[name].items():
            flat[f"{name}.{field}"] = val
    np.savez(tmp_path / "d.npz", **flat)
    a, want = ReactionStore.from_file(str(tmp_path / "d.npz")), case.store()
    with open(tmp_path / "d.pkl", "wb") as f:
        pickle.dump({k: (dict(v) if isinstance(v, dict) else v.tolist()) for k, v in case.raw.items()}, f)
    b = ReactionStore.from_file(str(tmp_path / "d.pkl"))
    for st in (a, b):
        assert len(st) == len(want) and st.sel.tolist() == want.sel.tolist()
        for s in range(3):
            assert np.array_equal(st._pos[s], want._pos[s]) and np.array_equal(st._z[s], want._z[s])

    class Evil:
        def __reduce__(self):
            return (os.system, ("true",))
    with open(tmp_path / "evil.pkl", "wb") as f:
        pickle.dump({"reactant": Evil()}, f)
    with pytest.raises(pickle.UnpicklingError, match="system"):
        load_raw(str(tmp_path / "evil.pkl"))
    with pytest.raises(ValueError):
        load_raw(str(tmp_path / "d.txt"))

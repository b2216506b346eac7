"""Shared by the dataset tests: the g12 fixture reader, a numpy emulation of `k_reaction_gather`'s arithmetic (csrc/oard_dataset.h) and a
random-store maker whose atom counts differ between the three objects of a reaction."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = ("default", "swap_by_ind", "reflect_append_multi", "confidence", "only_ts", "zero_charge", "no_center")
OBJECTS = ("reactant", "transition_state", "product")
PROPS = ("size", "pos", "one_hot", "charge", "mask")
CLASS = {1: 0, 6: 1, 7: 2, 8: 3, 9: 4}
EPS32 = 2.0 ** -24


class DatasetCase:
    """One tests/golden/g12_dataset_<cfg>.npz: `raw` (the mapping `ReactionStore` takes), `switches`, and the reference's collate of the
    whole dataset (`expected("all")`) and of the subset `sub_index` (`expected("sub")`), dtypes as the reference produced them."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.z = np.load(os.path.join(GOLDEN, f"g12_dataset_{cfg}.npz"), allow_pickle=False)
        meta = json.loads(str(self.z["meta"]))
        self.switches, self.n_samples = meta["switches"], meta["n_samples"]
        self.raw = {key: self.z[f"raw.{key}"] for key in ("single_fragment", "use_ind", "target", "rmsd")}
        for name in OBJECTS:
            self.raw[name] = {f: self.z[f"raw.{name}.{f}"] for f in ("num_atoms", "charges", "positions")}
            self.raw[name]["charges"] = self.raw[name]["charges"].astype(np.int64)
        self.sub_index = self.z["sub.index"]

    def store(self, device=None):
        from oareactdiff_amd.data import ReactionStore
        return ReactionStore(self.raw, device=device, **self.switches)

    def expected(self, tag):
        """-> (per object {prop: array}, {condition / target / rmsd: array})"""
        out, res = {}, {}
        for key in self.z.files:
            if not key.startswith(tag + ".") or key.endswith(".dtype") or key == "sub.index":
                continue
            val = self.z[key].astype(str(self.z[key + ".dtype"]))
            name = key[len(tag) + 1:]
            if name[0].isdigit():
                k, prop = name.split(".", 1)
                out.setdefault(int(k), {})[prop] = val
            else:
                res[name] = val
        return [out[k] for k in sorted(out)], res

    def max_raw(self, store, indices):
        """Per object, per atom row of the batch: max |raw position| of that row's molecule (the scale of the derived bound)."""
        _, s_bit, r = store.decode(indices)
        rows = []
        for s in store.src_obj:
            per = []
            for sb, rr in zip(s_bit, r):
                src = 2 - s if sb else s
                a, b = store.offsets[src][rr], store.offsets[src][rr + 1]
                per.append(np.full(b - a, np.abs(store._pos[src][a:b]).max()))
            rows.append(np.concatenate(per))
        return rows


def wave_sum(partials):
    """wave_sum_f64: the xor butterfly over 64 lanes, d = 32 .. 1 (csrc/oard_kernels.h)."""
    v = np.asarray(partials, dtype=np.float64).copy()
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ d]
    assert np.all(v == v[0]) or np.isnan(v).any()
    return v[0]


def center_f64(x32):
    """The kernel's centring of one molecule [n, 3] float32: lane partials in ascending rows, butterfly, one division, one rounding."""
    n = x32.shape[0]
    out = np.empty_like(x32)
    for c in range(3):
        part = np.zeros(64, dtype=np.float64)
        for lane in range(min(n, 64)):
            acc = np.float64(0.0)
            for i in range(lane, n, 64):
                acc = acc + np.float64(x32[i, c])
            part[lane] = acc
        mean = wave_sum(part) / np.float64(n)
        out[:, c] = (x32[:, c].astype(np.float64) - mean).astype(np.float32)
    return out


def emulate(store, indices):
    """What `store.batch(indices)` must return, bit for bit, from the store's host arrays: (per object {prop: array}, res dict)."""
    idx = np.asarray(indices, dtype=np.int64)
    f_bit, s_bit, r = store.decode(idx)
    B = idx.size
    reps = []
    for k, s in enumerate(store.src_obj):
        size, pos, one_hot, charge, mask = [], [], [], [], []
        for b in range(B):
            src = 2 - s if s_bit[b] else s
            a, e = store.offsets[src][r[b]], store.offsets[src][r[b] + 1]
            x = store._pos[src][a:e].copy()
            z = store._z[src][a:e].astype(np.int64)
            if f_bit[b] and store.reflect_obj[k]:
                x[:, 2] = -x[:, 2]
            pos.append(center_f64(x) if store.center else x)
            oh = np.zeros((e - a, 5), dtype=np.int64)
            oh[np.arange(e - a), [CLASS[int(v)] for v in z]] = 1
            one_hot.append(oh)
            col = np.zeros_like(z) if store.zero_charge else z
            charge.append(np.stack([col, np.full_like(z, store.append_charge[k])], axis=1) if store.append_frag else col[:, None])
            mask.append(np.full(e - a, b, dtype=np.int64))
            size.append(e - a)
        reps.append({"size": np.asarray(size, dtype=np.int64), "pos": np.concatenate(pos), "one_hot": np.concatenate(one_hot),
                     "charge": np.concatenate(charge), "mask": np.concatenate(mask)})
    res = {"condition": np.zeros((B, 1), dtype=np.int64)}
    if store._target is not None:
        res["target"], res["rmsd"] = store._target[idx % store.n_raw], store._rmsd[idx % store.n_raw]
    if store._ediff is not None:
        res["ediff"] = np.where(s_bit == 1, store._ediff[1][r], store._ediff[0][r]).astype(np.float32)
    return reps, res


RANDOM_COUNTS = np.array([[1, 63, 64], [63, 1, 65], [64, 65, 130], [65, 130, 1], [130, 64, 63], [5, 17, 9], [23, 2, 40], [7, 7, 7],
                          [2, 128, 3], [129, 3, 66]], dtype=np.int64)


def random_raw(seed=7, counts=RANDOM_COUNTS):
    """A raw mapping whose three objects have DIFFERENT atom counts per reaction (1, 63, 64, 65, 130 among them), padded arrays for the
    reactant, lists for the transition state, concatenated arrays for the product; every extra column present."""
    rng = np.random.default_rng(seed)
    R = counts.shape[0]
    raw = {"single_fragment": np.array([1] * R), "use_ind": np.array([i for i in range(R) if i != 5]),
           "target": rng.integers(0, 2, R), "rmsd": rng.uniform(0.0, 2.0, R)}
    raw["single_fragment"][7] = 0
    for s, name in enumerate(OBJECTS):
        n = counts[:, s]
        zs = [rng.choice([1, 6, 7, 8, 9], m) for m in n]
        ps = [3.0 * rng.standard_normal((m, 3)) + 5.0 for m in n]
        alt = [p + 0.25 for p in ps]
        if s == 0:
            zpad, ppad, apad = np.zeros((R, n.max()), dtype=np.int64), np.zeros((R, n.max(), 3)), np.zeros((R, n.max(), 3))
            for i, m in enumerate(n):
                zpad[i, :m], ppad[i, :m], apad[i, :m] = zs[i], ps[i], alt[i]
            raw[name] = {"num_atoms": n, "charges": zpad, "positions": ppad, "alt_positions": apad}
        elif s == 1:
            raw[name] = {"num_atoms": list(n), "charges": zs, "positions": ps, "alt_positions": alt}
        else:
            raw[name] = {"num_atoms": n, "charges": np.concatenate(zs), "positions": np.concatenate(ps), "alt_positions": np.concatenate(alt)}
        raw[name]["ediff"] = rng.standard_normal(R)
    return raw


#: switch sets the random store is built with (the kernel's every flag on at least once)
RANDOM_SWITCHES = {
    "plain": {},
    "swap_reflect": {"swapping_react_prod": True, "reflection": True, "use_by_ind": True, "ediff": "reactant"},
    "append_multi_key": {"append_frag": True, "single_frag_only": False, "reflection": True, "position_key": "alt_positions"},
    "confidence_swap": {"confidence_model": True, "swapping_react_prod": True, "single_frag_only": False},
    "only_ts_raw": {"only_ts": True, "center": False, "zero_charge": True, "reflection": True},
}


def assert_same(got, want, what=""):
    """Bitwise equality of two batches given as (reps, res) of numpy arrays."""
    (g_reps, g_res), (w_reps, w_res) = got, want
    assert len(g_reps) == len(w_reps), what
    for k, (g, w) in enumerate(zip(g_reps, w_reps)):
        for prop in PROPS:
            assert g[prop].dtype == w[prop].dtype and g[prop].shape == w[prop].shape, (what, k, prop, g[prop].dtype, g[prop].shape, w[prop].shape)
            assert np.array_equal(g[prop].view(np.uint8), w[prop].view(np.uint8)), (what, k, prop)
    assert set(g_res) == set(w_res), what
    for key in w_res:
        assert g_res[key].dtype == w_res[key].dtype and g_res[key].shape == w_res[key].shape, (what, key)
        assert np.array_equal(g_res[key], w_res[key]), (what, key)


def to_numpy(batch):
    """A `store.batch` result -> (reps, res) of numpy arrays (device tensors copied to the host)."""
    reps, res = batch
    if not isinstance(res, dict):
        res = {"condition": res}
    return ([{p: r[p].detach().cpu().numpy() for p in PROPS} for r in reps], {k: v.detach().cpu().numpy() for k, v in res.items()})


def check_against_reference(case, store, got, indices, tag):
    """The issue's bounds for one batch `got` (numpy) against the reference's collate `tag`: integers equal; pos within
    (n + 2) * 2^-24 * max|raw pos of that molecule| of the reference (float32 summation of n terms plus two roundings) and within
    2^-24 * |exact| + 1e-12 of the float64 centring of the float32 raw (one rounding); a one-atom molecule centred is exactly 0."""
    ref_reps, ref_res = case.expected(tag)
    g_reps, g_res = got
    scale = case.max_raw(store, indices)
    f_bit, s_bit, r = store.decode(indices)
    assert len(g_reps) == len(ref_reps)
    for k, (g, w) in enumerate(zip(g_reps, ref_reps)):
        for prop in ("size", "one_hot", "charge", "mask"):
            assert g[prop].dtype == w[prop].dtype == np.int64 and g[prop].shape == w[prop].shape, (case.cfg, k, prop)
            assert np.array_equal(g[prop], w[prop]), (case.cfg, k, prop)
        assert g["pos"].dtype == w["pos"].dtype == np.float32 and g["pos"].shape == w["pos"].shape
        n_row = np.repeat(g["size"], g["size"]).astype(np.float64)
        if store.center:
            bound = (n_row + 2.0) * EPS32 * scale[k]
            assert np.all(np.abs(g["pos"].astype(np.float64) - w["pos"].astype(np.float64)) <= bound[:, None]), (case.cfg, k)
        else:
            assert np.array_equal(g["pos"], w["pos"]), (case.cfg, k)
        # exact: float64 centring of the float32 raw rows (pairwise float64 mean: its own error, ~n 2^-53, sits inside the 1e-12)
        start = 0
        s = store.src_obj[k]
        for b, n in enumerate(g["size"]):
            src = 2 - s if s_bit[b] else s
            a = store.offsets[src][r[b]]
            x = store._pos[src][a: a + n].astype(np.float64)
            if f_bit[b] and store.reflect_obj[k]:
                x[:, 2] = -x[:, 2]
            exact = x - x.mean(axis=0) if store.center else x
            err = np.abs(g["pos"][start: start + n].astype(np.float64) - exact)
            assert np.all(err <= EPS32 * np.abs(exact) + 1e-12), (case.cfg, k, b)
            if n == 1 and store.center:
                assert np.all(g["pos"][start] == 0.0)
            start += n
    for key in ref_res:
        assert g_res[key].dtype == ref_res[key].dtype and g_res[key].shape == ref_res[key].shape, (case.cfg, key, g_res[key].dtype, ref_res[key].dtype)
        assert np.array_equal(g_res[key], ref_res[key]), (case.cfg, key)
    assert set(g_res) == set(ref_res)

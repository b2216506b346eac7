"""The fused RePaint step (k_inpaint_step behind oard_inpaint_step / oard_inpaint_step_dev) alone, through the C ABI, against the
formulas of include/oard.h restated here in float64 plain torch.  The network never runs: the narrowest built width pair, one layer.

Layouts: different atom counts per object, an empty (sample, object) group with node_nfs 4 / 5 / 6, groups of 1024 / 1 / 129 atoms, and
B = 64 x 3 x 23 split into 1, 2, 3 and 4 sub-batches (one launch per sub-batch, one wavefront per group); and 1, 2, 4 and 8 objects per
reaction instead of three, where `fixed_mask` (one bit per object) runs over no bit, every single bit, all bits and, at eight, 0b10101010.

Gate of every output tensor (the rule of tests/test_sampler_step.py): err(x) = max|x - ref64| / max|ref64|; the same formulas in torch
float32 on the CPU give e32; required is err(kernel) <= max(4 e32, 2^-21).

Residual centre of mass: the kernel removes a group mean in float64 from float32 values and rounds each entry once, so what stays is at
most 2^-24 max|out| per entry; asserted is |mean_group(out_pos)| <= 2^-23 max|out_pos of the group| on every group that is projected
(not fixed, or any group on a jump step) - also when the operands share an offset of 60 with spread 1, where ONE float32-summed
projection leaves 3e-6 ... 1e-5 (DiffusionSampler._project_again)."""
import ctypes as C
import itertools

import pytest
import torch

from _cases import debug_options, rel
from oareactdiff_amd import _capi
from oareactdiff_amd.graph_tools import get_edges_index, get_mask_for_frag, get_n_frag_switch
from oareactdiff_amd.schedule import Schedule

pytestmark = pytest.mark.gpu

NARROW = dict(pos_require_grad=False, cutoff=5.0, num_layers=1, hidden_channels=32, num_radial=8, in_hidden_channels=8)
LAYOUTS = {
    "ragged": ([[7, 23, 12, 1, 16], [9, 20, 5, 3, 16], [4, 23, 12, 2, 30]], [9, 9, 9], 1),
    "wrapper": ([[2, 0], [2, 3], [1, 2]], [4, 5, 6], 3),              # object 0 is empty in sample 1
    "groups_1024_1_129": ([[1024], [1], [129]], [9, 9, 9], 1),        # the largest group, one atom, two passes of the 64 lanes + 1
    "b64": ([[23] * 64] * 3, [9, 9, 9], 1),
    "one_object": ([[8, 1, 17, 5]], [9], 1),
    "two_objects": ([[9, 0, 5], [12, 7, 5]], [7, 12], 0),             # object 0 is empty in sample 1; no conditions
    "four_objects": ([[2, 3, 6], [1, 4, 3], [3, 0, 5], [2, 2, 7]], [4, 19, 9, 6], 5, dict(NARROW, in_hidden_channels=16)),
    "eight_objects": ([[k + 1, 8 - k] for k in range(8)], [9] * 8, 1),                              # groups of 1 to 8 atoms
}
FLOOR = 2.0 ** -21
COM = 2.0 ** -23
POS = 3
GUARD = 3                       # NaN rows behind every output tensor
MASKS = (0, 0b101, 0b010, 0b111)
OPERANDS = ("z", "eh", "xfix", "nk", "ns", "nj")


def object_masks(n_obj):
    """No bit, every single bit, all bits; at eight objects also every other bit."""
    masks = [0] + [1 << k for k in range(n_obj)] + [(1 << n_obj) - 1]
    if n_obj == 8:
        masks.append(0b10101010)
    return tuple(dict.fromkeys(masks))


def coefficient_rows():
    """[a_s, sigma_s, alpha_ts, c_eps, sigma, jump, a_j, sigma_j] of real schedule steps, the jump flag left to the caller: the first
    sampling step and a middle one, each with a forward jump of 5 steps (the first step's from 994, the table ends at 1000)."""
    sch = Schedule("polynomial_2", 1000, 1e-5)
    rows = {}
    for name, s, j0 in (("first", 999, 994), ("middle", 500, 500)):
        a_s, sig_s = sch.alpha_sigma(s)
        co = sch.step(s)
        a_j, sig_j = sch.forward_jump(j0, j0 + 5)
        rows[name] = [a_s, sig_s, co.alpha_ts, co.c_eps, co.sigma, 0.0, a_j, sig_j]
    return rows


class Rig:
    """A narrow dynamics module and the topology handle of one layout."""

    def __init__(self, layout, dev):
        from oareactdiff_amd import EGNNDynamics
        frags, self.node_nfs, cnf = LAYOUTS[layout][:3]
        model_config = LAYOUTS[layout][3] if len(LAYOUTS[layout]) > 3 else NARROW
        self.dev = dev
        frag = [torch.tensor(f) for f in frags]
        self.masks = [get_mask_for_frag(f) for f in frag]
        cm = torch.cat(self.masks)
        self.n_groups = len(frags[0])
        self.n_obj = len(self.node_nfs)
        self.dyn = EGNNDynamics(model_config=dict(model_config),
                                fragment_names=["R", "TS", "P"] if self.n_obj == 3 else [f"o{k}" for k in range(self.n_obj)],
                                node_nfs=self.node_nfs, edge_nf=0, condition_nf=cnf, device=dev)
        keys = (get_edges_index(cm, remove_self_edge=True).to(dev), get_n_frag_switch(frag).to(dev), cm.to(dev))
        with torch.cuda.device(dev):
            self.stream = torch.cuda.current_stream(dev).cuda_stream
            self.topo = self.dyn._get_topology(self.dyn._config(), keys[0], keys[1], keys[2], self.stream)
        assert self.topo.handle is not None, "the layout must run on the production topology"
        self.cfg = self.dyn._config()

    def one_sub_batch(self):
        buf = torch.zeros(self.n_groups * self.n_obj + 1, dtype=torch.int32, device=self.dev)
        rc = _capi.lib().oard_topology_export(self.topo.handle, _capi.TOPO_GROUP_PTR, buf.data_ptr(), buf.numel(), self.stream)
        torch.cuda.synchronize()
        assert rc in (_capi.OARD_OK, _capi.OARD_EINVAL)
        return rc == _capi.OARD_OK

    def inputs(self, seed, offset):
        """Six operand sets of N(0,1) with `offset` on every position column, and h0 as small integers; on the CPU and on the device."""
        g = torch.Generator().manual_seed(seed)
        cpu = {}
        for name in OPERANDS:
            xs = [torch.randn(m.numel(), nf, generator=g) for m, nf in zip(self.masks, self.node_nfs)]
            for x in xs:
                x[:, :POS] += offset
            cpu[name] = xs
        cpu["h0"] = [torch.randint(0, 9, (m.numel(), nf - POS), generator=g).float() for m, nf in zip(self.masks, self.node_nfs)]
        dev = {k: [t.to(self.dev).contiguous() for t in v] for k, v in cpu.items()}
        return cpu, dev

    def arr(self, ts):
        return (C.c_void_p * self.n_obj)(*[t.data_ptr() for t in ts]) if ts is not None else None

    def launch(self, ops, fixed_mask, coef, zero_h, use_h0, entry, out=None, nj="given"):
        """One launch; returns (rc, outputs on the CPU without their guard rows).  Every output element starts as NaN."""
        bufs = [torch.full((m.numel() + GUARD, nf), float("nan"), device=self.dev) for m, nf in zip(self.masks, self.node_nfs)]
        outs = bufs if out is None else out
        L = _capi.lib()
        head = (C.byref(self.cfg), self.topo.handle, fixed_mask, self.arr(ops["z"]), self.arr(ops["eh"]), self.arr(ops["xfix"]),
                self.arr(ops["nk"]), self.arr(ops["ns"]), self.arr(ops["nj"]) if nj == "given" else None,
                self.arr(ops["h0"]) if use_h0 else None)
        with torch.cuda.device(self.dev):
            if entry == "raw":
                rc = L.oard_inpaint_step(*head, (C.c_float * 8)(*coef), zero_h, self.arr(outs), self.stream)
            else:
                cd = torch.tensor(coef, dtype=torch.float32, device=self.dev)
                rc = L.oard_inpaint_step_dev(*head, cd.data_ptr(), zero_h, self.arr(outs), self.stream)
        torch.cuda.synchronize()
        if rc != _capi.OARD_OK or out is not None:
            return rc, None
        got = []
        for b, m in zip(bufs, self.masks):
            b = b.cpu()
            assert bool(torch.isnan(b[m.numel():]).all()), "the step wrote behind an object's rows"
            got.append(b[: m.numel()])
        return rc, got


def group_mean(x, idx, n_groups):
    s = torch.zeros(n_groups, x.shape[1], dtype=x.dtype).index_add_(0, idx, x)
    cnt = torch.zeros(n_groups, dtype=x.dtype).index_add_(0, idx, torch.ones(idx.numel(), dtype=x.dtype)).clamp(min=1)
    return (s / cnt.unsqueeze(1))[idx]


def reference(ops, fixed_mask, coef, zero_h, use_h0, masks, n_groups, dtype):
    """The comment above oard_inpaint_step (include/oard.h), per object, in `dtype`; the scalars are the float32 values the kernel gets."""
    a_s, sig_s, a_ts, c_eps, sig, jump, a_j, sig_j = (torch.tensor(v, dtype=torch.float32).to(dtype) for v in coef)

    def eps(n, m):
        n = n.to(dtype)
        return torch.cat([n[:, :POS] - group_mean(n[:, :POS], m, n_groups), torch.zeros_like(n[:, POS:]) if zero_h else n[:, POS:]], dim=1)

    def project(y, m):
        return torch.cat([y[:, :POS] - group_mean(y[:, :POS], m, n_groups), y[:, POS:]], dim=1)
    outs = []
    for k, m in enumerate(masks):
        if (fixed_mask >> k) & 1:
            y = a_s * ops["xfix"][k].to(dtype) + sig_s * eps(ops["nk"][k], m)
        else:
            y = project(ops["z"][k].to(dtype) / a_ts - ops["eh"][k].to(dtype) * c_eps + sig * eps(ops["ns"][k], m), m)
        if use_h0:
            y = torch.cat([y[:, :POS], ops["h0"][k].to(dtype)], dim=1)
        if float(jump) != 0.0:
            y = project(a_j * y + sig_j * eps(ops["nj"][k], m), m)
        outs.append(y)
    return outs


def check_com(got, masks, n_groups, fixed_mask, jump, where):
    """|mean_group(out_pos)| <= 2^-23 max|out_pos of the group| on every projected group; returns the largest ratio seen."""
    worst = 0.0
    for k, m in enumerate(masks):
        if got[k].numel() == 0 or (((fixed_mask >> k) & 1) and not jump):
            continue
        p = got[k][:, :POS].double()
        cnt = torch.bincount(m, minlength=n_groups).clamp(min=1).double()
        mean = torch.zeros(n_groups, POS, dtype=torch.float64).index_add_(0, m, p) / cnt.unsqueeze(1)
        top = torch.zeros(n_groups, dtype=torch.float64).scatter_reduce_(0, m, p.abs().max(dim=1).values, reduce="amax")
        bad = mean.abs().max(dim=1).values > COM * top
        assert not bool(bad.any()), (f"{where} object {k}: group {int(bad.nonzero()[0])} keeps a mean of "
                                     f"{float(mean.abs().max(dim=1).values[bad][0]):.3e} against max|out| {float(top[bad][0]):.3e}")
        ok = top > 0
        if bool(ok.any()):
            worst = max(worst, float((mean.abs().max(dim=1).values[ok] / top[ok]).max()))
    return worst


def sweep(rig, title, offsets=(0.0, 60.0), coef_names=("first", "middle"), entries=("raw", "dev"), masks=MASKS):
    """fixed_mask x jump x zero_feature_noise x h0 given / None x coefficient rows x input sets.  Returns the raw entry's outputs."""
    kept, worst_err, worst_ratio, worst_com = [], 0.0, 0.0, {}
    ng = rig.n_groups
    rows = coefficient_rows()
    for offset in offsets:
        cpu, ops = rig.inputs(17 + int(offset), offset)
        before = {k: [t.clone() for t in v] for k, v in ops.items()}
        for cname, fixed_mask, jump, zero_h, use_h0 in itertools.product(coef_names, masks, (0, 1), (0, 1), (False, True)):
            coef = list(rows[cname])
            coef[5] = float(jump)
            where = f"{title} offset {offset} coefficients {cname} fixed {fixed_mask:0{rig.n_obj}b} jump {jump} zero_feature_noise {zero_h} h0 {use_h0}"
            rc, got = rig.launch(ops, fixed_mask, coef, zero_h, use_h0, "raw")
            assert rc == _capi.OARD_OK, where
            kept.append(got)
            if "dev" in entries:
                rc, same = rig.launch(ops, fixed_mask, coef, zero_h, use_h0, "dev")
                assert rc == _capi.OARD_OK, where
                assert all(torch.equal(a, b) for a, b in zip(got, same)), f"{where}: coefficients in device memory: other bits"
            for name in ops:
                assert all(torch.equal(a, b) for a, b in zip(ops[name], before[name])), f"{where}: the step changed operand {name}"
            r64 = reference(cpu, fixed_mask, coef, zero_h, use_h0, rig.masks, ng, torch.float64)
            r32 = reference(cpu, fixed_mask, coef, zero_h, use_h0, rig.masks, ng, torch.float32)
            for k in range(rig.n_obj):
                if got[k].numel() == 0:
                    continue
                assert bool(torch.isfinite(got[k]).all()), f"{where} object {k}: an element was not written"
                slices = [("tensor", slice(None)), ("positions", slice(0, POS))]
                if not use_h0 or jump:
                    slices.append(("features", slice(POS, None)))
                for name, sl in slices:
                    err, e32 = rel(got[k][:, sl], r64[k][:, sl]), rel(r32[k][:, sl], r64[k][:, sl])
                    worst_err = max(worst_err, err)
                    if e32 > 0:
                        worst_ratio = max(worst_ratio, err / e32)
                    assert err <= max(4 * e32, FLOOR), f"{where} object {k} {name}: kernel {err:.3e}, float32 formula {e32:.3e}"
                if use_h0 and not jump:
                    assert torch.equal(got[k][:, POS:], cpu["h0"][k]), f"{where} object {k}: features are not h0"
            worst_com[offset] = max(worst_com.get(offset, 0.0), check_com(got, rig.masks, ng, fixed_mask, jump, where))
    print(f"{title}: worst kernel err {worst_err:.2e}, worst err / e32 {worst_ratio:.2f}, largest |group mean| / max|out of the group| "
          + ", ".join(f"offset {o}: {v:.2e}" for o, v in worst_com.items()) + f" (bound {COM:.2e})")
    return kept


@pytest.mark.parametrize("layout", ["ragged", "wrapper", "groups_1024_1_129"])
def test_fused_step_matches_its_float64_formula(layout):
    sweep(Rig(layout, torch.device("cuda:0")), layout)


@pytest.mark.parametrize("layout", ["one_object", "two_objects", "four_objects", "eight_objects"])
def test_fused_step_with_other_object_counts(layout):
    rig = Rig(layout, torch.device("cuda:0"))
    masks = object_masks(rig.n_obj)
    assert len(masks) == {1: 2, 2: 4, 4: 6, 8: 11}[rig.n_obj]
    sweep(rig, layout, masks=masks)
    # a bit beyond the objects is refused, at every object count (at eight there is no such bit in the 8-bit mask: bit 8)
    _, ops = rig.inputs(3, 0.0)
    scratch = [torch.zeros_like(x) for x in ops["z"]]
    row = coefficient_rows()["middle"]
    for entry in ("raw", "dev"):
        assert rig.launch(ops, 1 << rig.n_obj, row, 0, False, entry, out=scratch)[0] == _capi.OARD_EINVAL


def test_sub_batches_give_identical_bits():
    """B = 64 x 3 x 23 under `parts` = 1, 2, 3 and the library's own split (4): a group's result is a property of the group alone."""
    dev = torch.device("cuda:0")
    with debug_options(parts=1):
        rig = Rig("b64", dev)
        assert rig.one_sub_batch()
        base = sweep(rig, "b64 parts=1")
    for parts in (2, 3, 0):
        with debug_options(parts=parts):
            rig = Rig("b64", dev)
            assert not rig.one_sub_batch(), "the topology was not split"
            got = sweep(rig, f"b64 parts={parts}", offsets=(60.0,), coef_names=("middle",), entries=("raw",))
        tail = base[-len(got):]                              # the sweep's last block: offset 60, the middle row
        assert len(got) == len(tail) == 32
        for a, b in zip(got, tail):
            assert all(torch.equal(x, y) for x, y in zip(a, b)), f"parts={parts} differs from parts=1"


def test_bad_arguments_are_refused():
    dev = torch.device("cuda:0")
    rig = Rig("ragged", dev)
    _, ops = rig.inputs(3, 0.0)
    row = coefficient_rows()["middle"]
    jump = list(row)
    jump[5] = 1.0
    scratch = [torch.zeros_like(x) for x in ops["z"]]
    assert rig.launch(ops, 0b010, row, 0, False, "raw", out=scratch)[0] == _capi.OARD_OK
    for entry in ("raw", "dev"):
        # out on z (object 0 is free under 0b010), on xfix (object 1 is fixed), on a noise operand
        for name in ("z", "xfix", "nk", "ns", "nj"):
            assert rig.launch(ops, 0b010, row, 0, False, entry, out=ops[name])[0] == _capi.OARD_EINVAL, (entry, name)
        assert rig.launch(ops, 0b1000, row, 0, False, entry, out=scratch)[0] == _capi.OARD_EINVAL       # a bit beyond the objects
    # no jump noise: fine for host scalars without a jump, refused with one, and always for the device row
    assert rig.launch(ops, 0b010, row, 0, False, "raw", out=scratch, nj=None)[0] == _capi.OARD_OK
    assert rig.launch(ops, 0b010, jump, 0, False, "raw", out=scratch, nj=None)[0] == _capi.OARD_EINVAL
    assert rig.launch(ops, 0b010, row, 0, False, "dev", out=scratch, nj=None)[0] == _capi.OARD_EINVAL
    # through the sampler's wrapper the code becomes an error
    from oareactdiff_amd import DiffusionSampler
    smp = DiffusionSampler(rig.dyn, "polynomial_2", 1000, 1e-5)
    with torch.cuda.device(dev), pytest.raises(_capi.OardError):
        smp._inpaint_step(rig.topo, 0b010, ops["z"], ops["eh"], ops["xfix"], ops["nk"], ops["ns"], None, None, jump, scratch, rig.stream)
    with torch.cuda.device(dev):
        smp._inpaint_step(rig.topo, 0b010, ops["z"], ops["eh"], ops["xfix"], ops["nk"], ops["ns"], ops["nj"], None, jump, scratch, rig.stream)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in scratch)


# MEASURED on an MI355X, over both input sets (offset 0 / 60), both coefficient rows, the four masks, jump off / on, zero_feature_noise
# 0 / 1, h0 given / None: worst kernel err, worst err / e32 (gate 4), largest |group mean| / max|out of the group| at offset 0 / 60
# (bound 1.19e-07):
#   ragged              2.55e-06   1.42   1.99e-08 / 2.14e-08
#   wrapper             2.77e-06   2.29   1.77e-08 / 1.81e-08
#   groups_1024_1_129   1.93e-06   1.74   4.57e-09 / 6.12e-09
#   b64 (any parts)     2.00e-06   1.54   1.47e-08 / 1.18e-08
# and over object_masks(n_obj) in place of the four masks:
#   one_object          2.04e-06   1.36   1.04e-08 / 1.86e-08
#   two_objects         2.99e-06   1.14   2.28e-08 / 2.21e-08
#   four_objects        5.61e-06   2.16   2.78e-08 / 2.45e-08
#   eight_objects       3.49e-06   2.08   2.65e-08 / 2.53e-08

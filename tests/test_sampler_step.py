"""The element-wise sampler kernel (k_sampler_step behind oard_sampler_step / oard_sampler_step_dev) and oard_nan_replace, every mode
against the formulas of include/oard.h restated here in float64 plain torch - on layouts the golden fixtures do not have: different
atom counts per object, an empty (sample, object) group, 1-atom / 129-atom / 1024-atom groups, and a B = 64 batch split into 1, 2, 3
and 4 sub-batches (the step launches once per sub-batch); and with 1, 2, 4 and 8 objects per reaction instead of three (the object
loop, the per-object pointer tables and the group table `n_groups = B x n_obj` at every count the library takes).

The gate of every output tensor: err(x) = max|x - ref64| / max|ref64|; the same formulas in torch float32 on the CPU give e32;
required is err(kernel) <= max(4 e32, 2^-21) - the factor covers the different summation order of the group means (the kernel sums a
group's rows one after the other), the floor the case where e32 happens to be a single rounding."""
import ctypes as C
from dataclasses import astuple

import pytest
import torch

from _cases import debug_options, rel
from oareactdiff_amd import _capi
from oareactdiff_amd.graph_tools import get_edges_index, get_mask_for_frag, get_n_frag_switch
from oareactdiff_amd.schedule import Schedule

pytestmark = pytest.mark.gpu

# the network is never run here: the narrowest built width pair, one layer
NARROW = dict(pos_require_grad=False, cutoff=5.0, num_layers=1, hidden_channels=32, num_radial=8, in_hidden_channels=8)
WIDE = dict(NARROW, in_hidden_channels=16)           # embedding 10 + t + 5 conditions: all 16 columns of h_in in use
#           atoms per sample of each object (R, TS, P)                          node_nfs   condition_nf  [model_config]
LAYOUTS = {
    "ragged": ([[7, 23, 12, 1, 16], [9, 20, 5, 3, 16], [4, 23, 12, 2, 30]], [9, 9, 9], 1),
    "wrapper": ([[2, 0], [2, 3], [1, 2]], [4, 5, 6], 3),              # golden g1_wrapper_small: object 0 is empty in sample 1
    "groups_1024_1_129": ([[1024], [1], [129]], [9, 9, 9], 1),        # OARD_MAX_GROUP, one atom, one more than a 128-thread block
    "b64": ([[23] * 64] * 3, [9, 9, 9], 1),                           # the benchmark's batch: 4 sub-batches by default
    "one_object": ([[8, 1, 17, 5]], [9], 1),                          # every edge is an inner edge
    "two_objects": ([[9, 0, 5], [12, 7, 5]], [7, 12], 0),             # object 0 is empty in sample 1; no conditions
    "four_objects": ([[2, 3, 6], [1, 4, 3], [3, 0, 5], [2, 2, 7]], [4, 19, 9, 6], 5, WIDE),       # feature widths 1 and 16 side by side
    "eight_objects": ([[k + 1, 8 - k] for k in range(8)], [9] * 8, 1),                              # groups of 1 to 8 atoms
}
MODES = {0: "ancestral step", 1: "final x|z0", 2: "initial noise", 3: "q(z_s|x)", 4: "forward jump"}
FLOOR = 2.0 ** -21
POS = 3


def _coefficients():
    """(a, b, c) of real schedule steps: the first sampling step (t = 1), a middle one, and the final x | z_0 triple.  Every mode is run
    with every triple - all three values differ and none is 0 or 1, so a mode that read the wrong scalar would show."""
    s = Schedule("polynomial_2", 1000, 1e-5)
    return {"first": astuple(s.step(999)), "middle": astuple(s.step(500)), "final": astuple(s.final())}


class Rig:
    """A narrow dynamics module, its two samplers (zero_feature_noise = 0 / 1) and the topology handle of one layout."""

    def __init__(self, layout, dev):
        from oareactdiff_amd import DiffusionSampler, EGNNDynamics
        frags, self.node_nfs, cnf = LAYOUTS[layout][:3]
        model_config = LAYOUTS[layout][3] if len(LAYOUTS[layout]) > 3 else NARROW
        n_obj = len(frags)
        self.dev = dev
        frag = [torch.tensor(f) for f in frags]
        self.masks = [get_mask_for_frag(f) for f in frag]
        cm = torch.cat(self.masks)
        self.n_groups = len(frags[0])
        self.dyn = EGNNDynamics(model_config=dict(model_config), fragment_names=["R", "TS", "P"] if n_obj == 3 else [f"o{k}" for k in range(n_obj)],
                                node_nfs=self.node_nfs, edge_nf=0, condition_nf=cnf, device=dev)
        self.smp = {z: DiffusionSampler(self.dyn, "polynomial_2", 1000, 1e-5, pos_only=bool(z)) for z in (0, 1)}
        self.keys = (get_edges_index(cm, remove_self_edge=True).to(dev), get_n_frag_switch(frag).to(dev), cm.to(dev))
        with torch.cuda.device(dev):
            self.stream = torch.cuda.current_stream(dev).cuda_stream
            self.topo = self.dyn._get_topology(self.dyn._config(), self.keys[0], self.keys[1], self.keys[2], self.stream)
        assert self.topo.handle is not None, "the layout must run on the production topology"

    def one_sub_batch(self):
        """True iff the topology holds ONE sub-batch: oard_topology_export serves only those."""
        buf = torch.zeros(self.n_groups * len(self.node_nfs) + 1, dtype=torch.int32, device=self.dev)
        rc = _capi.lib().oard_topology_export(self.topo.handle, _capi.TOPO_GROUP_PTR, buf.data_ptr(), buf.numel(), self.stream)
        torch.cuda.synchronize()
        assert rc in (_capi.OARD_OK, _capi.OARD_EINVAL)
        return rc == _capi.OARD_OK

    def inputs(self, seed, offset):
        """z, eps_hat, noise: N(0,1); h0: small integers.  `offset` is added to every position column (common to the group, so that the
        group-mean subtraction cancels it)."""
        g = torch.Generator().manual_seed(seed)
        sets = []
        for _ in range(3):
            xs = [torch.randn(m.numel(), nf, generator=g) for m, nf in zip(self.masks, self.node_nfs)]
            for x in xs:
                x[:, :POS] += offset
            sets.append(xs)
        h0 = [torch.randint(0, 9, (m.numel(), nf - POS), generator=g).float() for m, nf in zip(self.masks, self.node_nfs)]
        return sets[0], sets[1], sets[2], h0

    def run(self, mode, z, eh, noise, h0, abc, zero_h, entry):
        """One step.  `entry`: "host" / "dev" = the sampler's wrappers (`_step_kernel`, `_step_kernel_dev`: for modes 0 and 4 the kernel
        plus its second projection), "raw" / "raw_dev" = the C entries called directly (one launch of k_sampler_step).  Returns the
        outputs on the CPU; asserts that no input changed."""
        dev = self.dev
        up = lambda ts: [t.to(dev).contiguous() for t in ts] if ts is not None else None
        zd, ed, nd, hd = up(z if mode != 2 else None), up(eh if mode <= 1 else None), up(noise), up(h0)
        out = [torch.full(n.shape, float("nan"), device=dev) for n in nd]          # every element must be written
        smp = self.smp[zero_h]
        with torch.cuda.device(dev):
            coef = torch.tensor(abc, dtype=torch.float32, device=dev)
            if entry == "host":
                smp._step_kernel(self.topo, mode, zd, ed, nd, hd, abc[0], abc[1], abc[2], out, self.stream)
            elif entry == "dev":
                smp._step_kernel_dev(self.topo, mode, zd, ed, nd, hd, coef, out, self.stream)
            else:
                L, cfg = _capi.lib(), self.dyn._config()
                arr = lambda ts: (C.c_void_p * len(nd))(*[t.data_ptr() for t in ts]) if ts is not None else None
                if entry == "raw":
                    rc = L.oard_sampler_step(C.byref(cfg), self.topo.handle, mode, arr(zd), arr(ed), arr(nd), arr(hd), C.c_float(abc[0]),
                                             C.c_float(abc[1]), C.c_float(abc[2]), zero_h, arr(out), self.stream)
                else:
                    rc = L.oard_sampler_step_dev(C.byref(cfg), self.topo.handle, mode, arr(zd), arr(ed), arr(nd), arr(hd), coef.data_ptr(),
                                                 zero_h, arr(out), self.stream)
                assert rc == _capi.OARD_OK
        torch.cuda.synchronize()
        for given, on_dev in ((z, zd), (eh, ed), (noise, nd), (h0, hd)):
            if on_dev is not None:
                assert all(torch.equal(a, b.cpu()) for a, b in zip(given, on_dev)), "the step changed an input"
        return [o.cpu() for o in out]


def group_mean(x, idx, n_groups):
    s = torch.zeros(n_groups, x.shape[1], dtype=x.dtype).index_add_(0, idx, x)
    cnt = torch.zeros(n_groups, dtype=x.dtype).index_add_(0, idx, torch.ones(idx.numel(), dtype=x.dtype)).clamp(min=1)
    return (s / cnt.unsqueeze(1))[idx]


def reference(mode, z, eh, noise, h0, abc, zero_h, masks, n_groups, dtype, project=True):
    """The comment above oard_sampler_step (include/oard.h), per object, in `dtype`.  `project=False`: without the CoM projection of
    modes 0 and 4 (the values whose group mean the kernel has to find)."""
    a, b, c = (torch.tensor(v, dtype=torch.float32).to(dtype) for v in abc)          # the float32 scalars the kernel receives
    outs = []
    for k, m in enumerate(masks):
        r = noise[k].to(dtype)
        eps = torch.cat([r[:, :POS] - group_mean(r[:, :POS], m, n_groups),
                         torch.zeros_like(r[:, POS:]) if zero_h else r[:, POS:]], dim=1)
        zk, ek = z[k].to(dtype), eh[k].to(dtype)
        if mode == 0:
            o = zk / a - ek * b + c * eps
        elif mode == 1:
            o = a * (zk - b * ek) + c * eps
        elif mode == 2:
            o = eps
        else:
            o = a * zk + c * eps
        if mode in (0, 4) and project:
            o = torch.cat([o[:, :POS] - group_mean(o[:, :POS], m, n_groups), o[:, POS:]], dim=1)
        if h0 is not None:
            o = torch.cat([o[:, :POS], h0[k].to(dtype)], dim=1)
        outs.append(o)
    return outs


class Worst:
    """Per mode: the largest kernel error, the float32 formula's error beside it, and the largest ratio of the two."""

    def __init__(self):
        self.rows = {m: [0.0, 0.0, 0.0] for m in MODES}

    def add(self, mode, err, e32):
        row = self.rows[mode]
        if err > row[0]:
            row[0], row[1] = err, e32
        if e32 > 0:
            row[2] = max(row[2], err / e32)

    def report(self, title):
        for m, (err, e32, ratio) in self.rows.items():
            print(f"{title} mode {m} ({MODES[m]}): worst kernel err {err:.2e} (e32 beside it {e32:.2e}), worst err / e32 {ratio:.2f}")


def sweep(rig, title, entries=("host", "dev")):
    """All modes x h0 given / None x zero_feature_noise x three coefficient triples x two input sets.  Returns the host entry's outputs
    and, per input set, the largest |group mean| / max|out| of the position blocks that modes 0 and 4 project (with its case)."""
    worst, worst_raw, kept, com = Worst(), Worst(), [], {}
    ng = rig.n_groups
    for offset in (0.0, 50.0):
        z, eh, noise, h0v = rig.inputs(11 + int(offset), offset)
        for cname, abc in _coefficients().items():
            for mode in MODES:
                for h0 in (h0v, None):
                    for zero_h in (0, 1):
                        got = rig.run(mode, z, eh, noise, h0, abc, zero_h, "host")
                        kept.append(got)
                        if "dev" in entries:
                            same = rig.run(mode, z, eh, noise, h0, abc, zero_h, "dev")
                            assert all(torch.equal(a, b) for a, b in zip(got, same)), "coefficients in device memory: other bits"
                        r64 = reference(mode, z, eh, noise, h0, abc, zero_h, rig.masks, ng, torch.float64)
                        r32 = reference(mode, z, eh, noise, h0, abc, zero_h, rig.masks, ng, torch.float32)
                        where = f"{title} offset {offset} coefficients {cname} mode {mode} h0 {h0 is not None} zero_feature_noise {zero_h}"
                        for k, m in enumerate(rig.masks):
                            if got[k].numel() == 0:
                                continue
                            # the whole tensor, and its position block on its own (h0's integers would otherwise set the scale)
                            slices = [("tensor", slice(None)), ("positions", slice(0, POS))]
                            if h0 is None:                   # computed features at their own scale (with the offset max|ref| is ~50)
                                slices.append(("features", slice(POS, None)))
                            for name, sl in slices:
                                err, e32 = rel(got[k][:, sl], r64[k][:, sl]), rel(r32[k][:, sl], r64[k][:, sl])
                                worst.add(mode, err, e32)
                                # worst err / e32 measured on an MI355X: 1.51 (groups_1024_1_129, mode 0); per layout and mode: MEASURED below
                                assert err <= max(4 * e32, FLOOR), f"{where} object {k} {name}: kernel {err:.3e}, float32 formula {e32:.3e}"
                            if h0 is not None:
                                assert torch.equal(got[k][:, POS:], h0[k]), f"{where} object {k}: features are not h0"
                            if mode in (0, 4):
                                gm = float(group_mean(got[k][:, :POS].double(), m, ng).abs().max())
                                top = float(got[k][:, :POS].abs().max())
                                if top > 0 and gm / top >= com.get(offset, (-1.0, ""))[0]:
                                    com[offset] = (gm / top, f"{where} object {k}: group mean {gm:.3e}, max |out| {top:.3e}")
                        if mode in (0, 4) and "dev" in entries:
                            raw_step(rig, mode, z, eh, noise, h0, abc, zero_h, r64, r32, where, worst_raw)
    worst.report(title)
    if "dev" in entries:
        worst_raw.report(title + ", C entry alone,")
    for offset, (ratio, where) in com.items():
        print(f"{title} offset {offset}: largest group mean of a projected output {ratio:.2e} max|out| ({where})")
    return kept, com


def raw_step(rig, mode, z, eh, noise, h0, abc, zero_h, r64, r32, where, worst):
    """The C entries on their own (one launch of k_sampler_step, what a C caller gets): the same gate, host and device coefficients
    the same bits, and the group mean that ONE float32 projection can leave.  The kernel adds the n rows of a group up one after
    the other in float32: the sum is off by at most (n - 1) 2^-24 sum|u_i|, the mean it subtracts by n 2^-24 max|u| (u the
    un-projected values, the product with 1 / n included), and the subtraction rounds each output by 2^-24 |out|; so
    |group mean| <= n 2^-24 max|u| + 2^-23 max|out|.  (The wrappers' second projection brings it under 1e-6 max|out| whatever u is:
    test_projected_outputs_are_com_free.)"""
    ng = rig.n_groups
    got = rig.run(mode, z, eh, noise, h0, abc, zero_h, "raw")
    same = rig.run(mode, z, eh, noise, h0, abc, zero_h, "raw_dev")
    assert all(torch.equal(a, b) for a, b in zip(got, same)), f"{where}: C entries, coefficients in device memory: other bits"
    u64 = reference(mode, z, eh, noise, h0, abc, zero_h, rig.masks, ng, torch.float64, project=False)
    for k, m in enumerate(rig.masks):
        if got[k].numel() == 0:
            continue
        for name, sl in (("tensor", slice(None)), ("positions", slice(0, POS))):
            err, e32 = rel(got[k][:, sl], r64[k][:, sl]), rel(r32[k][:, sl], r64[k][:, sl])
            worst.add(mode, err, e32)
            assert err <= max(4 * e32, FLOOR), f"{where} object {k} {name}, C entry alone: kernel {err:.3e}, float32 formula {e32:.3e}"
        n_max = int(torch.bincount(m, minlength=ng).max())
        gm = float(group_mean(got[k][:, :POS].double(), m, ng).abs().max())
        bound = n_max * 2.0 ** -24 * float(u64[k][:, :POS].abs().max()) + 2.0 ** -23 * float(got[k][:, :POS].abs().max())
        assert gm <= bound, f"{where} object {k}, C entry alone: group mean {gm:.3e}, bound of one float32 projection {bound:.3e}"


_SWEEPS = {}


def _layout_sweep(layout):
    if layout not in _SWEEPS:
        _SWEEPS[layout] = sweep(Rig(layout, torch.device("cuda:0")), layout)
    return _SWEEPS[layout]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_mode_matches_its_float64_formula(layout):
    _layout_sweep(layout)


@pytest.mark.parametrize("offset", [0.0, 50.0])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_projected_outputs_are_com_free(layout, offset):
    """Modes 0 and 4 subtract the group mean of their position output: what is left is at most 1e-6 max|out|, also when the group's
    members share an offset far above their spread (MEASURED below)."""
    _, com = _layout_sweep(layout)
    ratio, where = com[offset]
    assert ratio <= 1e-6, where


def test_sub_batches_give_identical_bits():
    """B = 64 x 3 x 23 under `parts` = 1, 2, 3 and the library's own split (4): the step launches once per sub-batch and every row is
    computed from its own group alone, so the outputs are the same bits whatever the split."""
    dev = torch.device("cuda:0")
    with debug_options(parts=1):
        rig = Rig("b64", dev)
        assert rig.one_sub_batch()
        base, _ = sweep(rig, "b64 parts=1", entries=("host",))
    for parts in (2, 3, 0):
        with debug_options(parts=parts):
            rig = Rig("b64", dev)
            assert not rig.one_sub_batch(), "the topology was not split"
            got, _ = sweep(rig, f"b64 parts={parts}", entries=("host",))
        assert len(got) == len(base)
        for a, b in zip(got, base):
            assert all(torch.equal(x, y) for x, y in zip(a, b)), f"parts={parts} differs from parts=1"


def test_bad_arguments_are_refused():
    dev = torch.device("cuda:0")
    rig = Rig("ragged", dev)
    z, eh, noise, h0 = rig.inputs(3, 0.0)
    up = lambda ts: [t.to(dev) for t in ts]
    z, eh, noise = up(z), up(eh), up(noise)
    out = [torch.zeros_like(x) for x in noise]
    L = _capi.lib()
    cfg = rig.dyn._config()
    arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts]) if ts is not None else None
    coef = torch.ones(3, device=dev)

    def both(mode, zz, ee):
        rc = L.oard_sampler_step(C.byref(cfg), rig.topo.handle, mode, arr(zz), arr(ee), arr(noise), None, C.c_float(1.0), C.c_float(1.0),
                                 C.c_float(1.0), 0, arr(out), rig.stream)
        rcd = L.oard_sampler_step_dev(C.byref(cfg), rig.topo.handle, mode, arr(zz), arr(ee), arr(noise), None, coef.data_ptr(), 0, arr(out),
                                      rig.stream)
        return rc, rcd
    with torch.cuda.device(dev):
        assert both(5, z, eh) == (_capi.OARD_EINVAL, _capi.OARD_EINVAL)
        assert both(-1, z, eh) == (_capi.OARD_EINVAL, _capi.OARD_EINVAL)
        assert both(0, None, eh) == (_capi.OARD_EINVAL, _capi.OARD_EINVAL)
        assert both(1, z, None) == (_capi.OARD_EINVAL, _capi.OARD_EINVAL)
        assert both(0, z, eh) == (_capi.OARD_OK, _capi.OARD_OK)
        # ... and through the sampler's own wrappers, which turn the code into an error
        for mode, zz, ee in ((5, z, eh), (0, None, eh), (1, z, None)):
            with pytest.raises(_capi.OardError):
                rig.smp[0]._step_kernel(rig.topo, mode, zz, ee, noise, None, 1.0, 1.0, 1.0, out, rig.stream)
            with pytest.raises(_capi.OardError):
                rig.smp[0]._step_kernel_dev(rig.topo, mode, zz, ee, noise, None, coef, out, rig.stream)
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout", ["ragged", "wrapper", "groups_1024_1_129"])
def test_nan_replace_against_its_formula(layout):
    """oard_nan_replace: status 0 leaves every bit of the output; status != 0 replaces each velocity block by noise - group mean (same
    gate as the step) and leaves the feature columns."""
    check_nan_replace(layout)


def check_nan_replace(layout):
    """(shared with tests/test_object_counts.py, which runs it with one and with eight objects)"""
    dev = torch.device("cuda:0")
    rig = Rig(layout, dev)
    L = _capi.lib()
    cfg = rig.dyn._config()
    n_obj = len(rig.node_nfs)
    arr = lambda ts: (C.c_void_p * n_obj)(*[t.data_ptr() for t in ts])
    for offset in (0.0, 50.0):
        g = torch.Generator().manual_seed(29 + int(offset))
        before = [torch.randn(m.numel(), nf, generator=g) for m, nf in zip(rig.masks, rig.node_nfs)]
        noise = [torch.randn(m.numel(), POS, generator=g) + offset for m in rig.masks]
        nd = [x.to(dev) for x in noise]
        for flag in (0, 1, -7):
            out = [x.to(dev) for x in before]
            status = torch.tensor([flag, 0], dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                _capi.check(L.oard_nan_replace(C.byref(cfg), rig.topo.handle, status.data_ptr(), arr(nd), arr(out), rig.stream), "oard_nan_replace")
            torch.cuda.synchronize()
            assert all(torch.equal(a, b.cpu()) for a, b in zip(noise, nd))
            assert int(status[0].item()) == flag
            for k, m in enumerate(rig.masks):
                got = out[k].cpu()
                if flag == 0:
                    assert torch.equal(got, before[k])
                    continue
                assert torch.equal(got[:, POS:], before[k][:, POS:])
                r64 = noise[k].double() - group_mean(noise[k].double(), m, rig.n_groups)
                r32 = noise[k] - group_mean(noise[k], m, rig.n_groups)
                err, e32 = rel(got[:, :POS], r64), rel(r32, r64)
                print(f"nan_replace {layout} offset {offset} flag {flag} object {k}: kernel err {err:.2e}, e32 {e32:.2e}")
                assert err <= max(4 * e32, FLOOR)


# MEASURED on an MI355X (suite launch shapes and OARD_TEST_SHAPES=auto give the same figures: the step does not depend on them).
# Per layout and mode, over both input sets, the three coefficient triples, h0 given / None and zero_feature_noise 0 / 1:
# worst kernel err (e32 beside it), worst err / e32.  The large entries are the offset-50 set, where e32 is as large.
#                     mode 0                     mode 1                     mode 2                     mode 3                     mode 4
# ragged              2.02e-06 (3.47e-06) 1.48   2.02e-07 (2.13e-07) 1.26   2.39e-06 (2.39e-06) 1.20   1.66e-07 (1.66e-07) 1.10   1.63e-06 (3.56e-06) 1.00
# wrapper             4.32e-06 (7.08e-06) 1.19   9.36e-08 (9.36e-08) 1.00   3.29e-06 (3.29e-06) 1.00   9.58e-08 (8.82e-08) 1.09   2.97e-06 (3.95e-06) 1.00
# groups_1024_1_129   1.52e-06 (7.65e-06) 1.51   8.76e-07 (9.07e-07) 1.25   1.26e-05 (1.26e-05) 1.00   6.17e-07 (6.17e-07) 1.00   1.28e-06 (4.37e-06) 1.24
# b64 (any parts)     1.65e-06 (4.40e-06) 1.04   2.75e-07 (2.92e-07) 1.05   3.56e-06 (2.91e-06) 1.22   2.31e-07 (1.91e-07) 1.21   1.26e-06 (4.04e-06) 1.26
# Largest |group mean| / max|out| of a mode 0 / mode 4 position output (bound 1e-6), offset 0 / offset 50:
#   ragged 1.86e-08 / 1.22e-08   wrapper 2.18e-08 / 1.92e-08   groups_1024_1_129 5.98e-09 / 5.09e-09   b64 1.41e-08 / 1.07e-08
#   (one projection alone, as the kernel does it: offset 50 leaves 3.03e-06, 2.98e-06, 1.10e-05, 4.15e-06 - hence the second pass of
#   DiffusionSampler._project_again)
# one / two / four / eight objects: worst kernel err over the modes 3.32e-06 (mode 0, eight_objects), worst err / e32 2.39 (mode 4,
# two_objects; the C entry alone: 5.92e-06, 2.39); largest group mean 2.8e-08 max|out|.
# oard_nan_replace, object 0 (kernel err / e32): offset 0 ragged 3.97e-08 / 3.97e-08, wrapper 3.15e-08 / 3.15e-08, groups 2.37e-08 /
# 2.37e-08; offset 50 ragged 1.97e-06 / 2.11e-06, wrapper 2.96e-06 / 2.96e-06, groups 4.12e-06 / 4.12e-06.

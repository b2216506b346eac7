"""oareactdiff_amd.metrics with like atoms matched first: `matched_rmsd`, `batch_rmsd(match_order=True)` and
`DDPMTrainer.eval_inpaint_batch(match_order=True)`, on the sample layout the samplers return ([n, 9]: positions, one-hot, charge - the
species is the last column).  The kernel itself is tested through the C ABI in tests/test_match_kernel.py."""
import numpy as np
import pytest
import torch

import _kabsch_cases as kc
import _match_cases as mc

SIZES = [4, 7, 1, 5]
CHARGES = [[6, 1, 1, 1], [6, 6, 8, 1, 1, 1, 1], [8], [7, 1, 1, 6, 1]]
WIDTH = 9


def _dev():
    return torch.device("cuda:0")


def _lists(seed=0, noise=0.0):
    """Three objects of ragged molecules; the generated rows are the true ones moved rigidly (plus `noise`) and then SHUFFLED, each row
    keeping its feature columns: like atoms change places, and so do unlike ones.  -> xh, out (numpy [n, 9] per object)."""
    rng = np.random.default_rng(seed)
    n = sum(SIZES)
    p = kc.seg_ptr(SIZES)
    xh, out = [], []
    for k in range(3):
        x = np.zeros((n, WIDTH), np.float32)
        x[:, :3] = 1.5 * rng.standard_normal((n, 3))
        x[:, 8] = np.concatenate(CHARGES)
        x[np.arange(n), 3 + (x[:, 8].astype(int) % 5)] = 1.0
        y = x.copy()
        for g in range(len(SIZES)):
            s = slice(p[g], p[g + 1])
            moved = x[s].copy()
            moved[:, :3] = x[s, :3] @ kc.random_rotation(rng).T.astype(np.float32) + rng.standard_normal(3).astype(np.float32) \
                + noise * rng.standard_normal((SIZES[g], 3)).astype(np.float32)
            order = rng.permutation(SIZES[g])
            while SIZES[g] > 1 and (order == np.arange(SIZES[g])).all():          # never the order given
                order = rng.permutation(SIZES[g])
            y[s] = moved[order]
        xh.append(x)
        out.append(y)
    return xh, out


def _reference(x, y, reflect=True):
    """float64 per molecule: the exact minimum (these molecules have few permutations) after b's rows are brought to a's species order."""
    p = kc.seg_ptr(SIZES)
    r, rho = [], []
    for g in range(len(SIZES)):
        a, b = x[p[g]: p[g + 1]], y[p[g]: p[g + 1]]
        sa, sb = a[:, 8].astype(int), b[:, 8].astype(int)
        order = np.argsort(sb, kind="stable")[np.argsort(np.argsort(sa, kind="stable"), kind="stable")]      # b[order] has a's species row by row
        assert (sb[order] == sa).all()
        r.append(mc.brute(a[:, :3], b[order][:, :3], sa, reflect)[0])
        rho.append(mc.rho(a[:, :3], b[:, :3]))
    return np.array(r), np.array(rho)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", [0, 1, 2])
def test_batch_rmsd_with_matching_undoes_a_shuffle(idx):
    from oareactdiff_amd.metrics import batch_rmsd
    dev = _dev()
    xh, out = _lists()
    frag = [torch.tensor(SIZES, device=dev) for _ in range(3)]
    xh_d, out_d = [torch.from_numpy(x).to(dev) for x in xh], [torch.from_numpy(x).to(dev) for x in out]
    kw = {} if idx == 1 else {"idx": idx}
    same = batch_rmsd(frag, out_d, xh_d, cap=None, **kw)                       # the default: the order given
    assert torch.equal(same, batch_rmsd(frag, out_d, xh_d, cap=None, match_order=False, **kw))
    matched = batch_rmsd(frag, out_d, xh_d, cap=None, match_order=True, **kw)
    assert matched.shape == (len(SIZES),) and matched.is_cuda and matched.dtype == torch.float32
    r, rho = _reference(xh[idx], out[idx])
    for g, n in enumerate(SIZES):
        print(f"idx={idx} n={n}: matched {float(matched[g]):.3e} (reference {r[g]:.3e}), same order {float(same[g]):.3e}")
        assert abs(float(matched[g]) - r[g]) <= kc.gate(r[g], rho[g])
        assert float(matched[g]) <= 1e-5                                       # a rigid copy: float32 rounding of the inputs is all that is left
        assert n < 4 or float(same[g]) > 0.3                                    # ... which the order given does not see
    capped = batch_rmsd(frag, out_d, xh_d, match_order=True, **kw)
    assert torch.equal(capped, matched.clamp(max=1.0))


@pytest.mark.gpu
def test_matched_rmsd_outputs_views_and_sizes():
    from oareactdiff_amd.metrics import MATCH_EXACT, MATCH_SEARCH, MATCH_SPECIES, MATCH_TOO_LARGE, kabsch_rmsd, matched_rmsd
    dev = _dev()
    xh, out = _lists(seed=1, noise=0.05)
    a, b = torch.from_numpy(xh[1]).to(dev), torch.from_numpy(out[1]).to(dev)
    r, rho = _reference(xh[1], out[1])
    # strided [n, 3] views of the [n, 9] tensors, species as the float column, a host list of sizes; every optional output
    rm, perm, status, rot, al = matched_rmsd(a[:, :3], b[:, :3], SIZES, a[:, -1], b[:, -1], return_perm=True, return_status=True,
                                             return_rotation=True, return_aligned=True)
    assert torch.equal(rm, matched_rmsd(a, b, torch.tensor(SIZES, device=dev), a[:, -1].long(), b[:, -1].long()))
    for g in range(len(SIZES)):
        assert abs(float(rm[g]) - r[g]) <= kc.gate(r[g], rho[g])
    assert perm.dtype == torch.int64 and status.tolist() == [MATCH_EXACT] * len(SIZES) and rot.shape == (len(SIZES), 3, 3)
    assert torch.equal(b[perm][:, -1], a[:, -1])                               # b[perm] is b in a's row order
    again = kabsch_rmsd(a, b[perm], SIZES)
    p = kc.seg_ptr(SIZES)
    for g in range(len(SIZES)):
        assert abs(float(again[g]) - float(rm[g])) <= kc.gate(float(rm[g]), rho[g])
        back = float(torch.sqrt(((al[p[g]: p[g + 1]].double() - a[p[g]: p[g + 1], :3].double()) ** 2).sum(1).mean()))
        assert abs(back - float(rm[g])) <= 1e-6 * (np.abs(xh[1][:, :3]).max() + np.abs(out[1][:, :3]).max())
    # exact_limit = 0: the search, never below the minimum
    srch, st = matched_rmsd(a, b, SIZES, a[:, -1], b[:, -1], exact_limit=0, return_status=True)
    assert st.tolist() == [MATCH_SEARCH] * len(SIZES)
    assert all(float(srch[g]) >= r[g] - kc.gate(r[g], rho[g]) for g in range(len(SIZES)))
    # species_b = None: the rows of b carry a's species - here they do not lie in that order, so nothing is undone
    assert bool((matched_rmsd(a, b, SIZES, a[:, -1])[1] > rm[1]).item())
    # device sizes are not read back: an entry that a host list is refused for is clamped, the oversize segment shows in the status
    n = int(a.shape[0])
    big_a, big_b = torch.cat([a] * 32)[:, :3], torch.cat([b] * 32)[:, :3]          # 544 rows: 4 + 257, and 283 left for the last entry
    sp = torch.zeros(32 * n, device=dev)
    with pytest.raises(ValueError):
        matched_rmsd(big_a, big_b, [4, 257], sp)
    with pytest.raises(ValueError):
        matched_rmsd(big_a, big_b, [4, 7, 1, 5000], sp)
    res, st = matched_rmsd(big_a, big_b, torch.tensor([4, 257, 5000], device=dev), sp, cap=0.75, return_status=True)
    assert st.tolist() == [MATCH_EXACT, MATCH_TOO_LARGE, MATCH_TOO_LARGE] and res[1:].tolist() == [0.75, 0.75]
    bad = a[:, -1].clone()
    bad[0] = 9.0
    res, st = matched_rmsd(a, b, SIZES, bad, b[:, -1], return_status=True)
    assert st.tolist() == [MATCH_SPECIES, MATCH_EXACT, MATCH_EXACT, MATCH_EXACT] and bool(torch.isnan(res[0])) and torch.equal(res[1:], rm[1:])


@pytest.mark.gpu
def test_argument_errors():
    from oareactdiff_amd.metrics import matched_rmsd
    dev = _dev()
    xh, out = _lists()
    a, b = torch.from_numpy(xh[1]).to(dev), torch.from_numpy(out[1]).to(dev)
    sp = a[:, -1]
    for args, kw in (((a, b[:-1], SIZES, sp), {}), ((a, b, [4, 7, 1, 6], sp), {}), ((a, b, [4, -1], sp), {}), ((a, b, SIZES, sp[:-1]), {}),
                     ((a, b, SIZES, sp, sp[:-1]), {}), ((a, b, SIZES, sp), {"exact_limit": 10001}), ((a, b, SIZES, sp), {"exact_limit": -1}),
                     ((a, b, SIZES, sp), {"cap": 0.0}), ((a[:, :2], b, SIZES, sp), {})):
        with pytest.raises(ValueError):
            matched_rmsd(*args, **kw)


def test_cpu_tensors_raise():
    from oareactdiff_amd._capi import OardError
    from oareactdiff_amd.metrics import batch_rmsd, matched_rmsd
    xh, out = _lists()
    a, b = torch.from_numpy(xh[1]), torch.from_numpy(out[1])
    with pytest.raises(OardError):
        matched_rmsd(a, b, SIZES, a[:, -1])
    with pytest.raises(OardError):
        batch_rmsd([torch.tensor(SIZES)] * 3, [torch.from_numpy(x) for x in out], [torch.from_numpy(x) for x in xh], match_order=True)


def test_xyz_writer_takes_a_permutation(tmp_path):
    from oareactdiff_amd.sampling_tools import write_single_xyz, write_tmp_xyz
    xh, out = _lists()
    rows = torch.from_numpy(out[1][:4])
    perm = [2, 0, 3, 1]
    write_single_xyz(str(tmp_path / "plain.xyz"), 4, rows)
    write_single_xyz(str(tmp_path / "perm.xyz"), 4, rows, perm=perm)
    plain, moved = [(tmp_path / f).read_text().splitlines() for f in ("plain.xyz", "perm.xyz")]
    assert plain[:2] == moved[:2] == ["4", ""] and moved[2:] == [plain[2 + k] for k in perm]
    with pytest.raises(ValueError):
        write_single_xyz(str(tmp_path / "bad.xyz"), 4, rows, perm=[0, 0, 1, 2])
    # per object, with the indices `matched_rmsd(return_perm=True)` returns: every molecule's rows inside the molecule
    p = kc.seg_ptr(SIZES)
    whole = np.concatenate([p[g] + np.random.default_rng(g).permutation(SIZES[g]) for g in range(len(SIZES))])
    samples = [torch.from_numpy(o) for o in out]
    a = write_tmp_xyz([torch.tensor(SIZES)] * 3, samples, idx=(1,), localpath=str(tmp_path), prefix="a")
    b = write_tmp_xyz([torch.tensor(SIZES)] * 3, samples, idx=(1,), localpath=str(tmp_path), prefix="b", perm={1: torch.from_numpy(whole)})
    for g, (fa, fb) in enumerate(zip(a, b)):
        la, lb = open(fa).read().splitlines(), open(fb).read().splitlines()
        assert lb[2:] == [la[2 + int(k - p[g])] for k in whole[p[g]: p[g + 1]]]


@pytest.mark.gpu
def test_eval_inpaint_batch_with_matching_is_never_larger(monkeypatch):
    """The smallest fixture of tests/test_trainer_eval_inpaint.py, on a positions-only trainer (the generated structure keeps the true
    atom types, so there is something to match): the same samples (same noise), matched <= same order per reaction, the float64
    minimum over the permutations of like atoms within the kernel's gate, and no host read more than without matching."""
    import test_trainer_eval_inpaint as te
    from oareactdiff_amd.trainer import DDPMTrainer
    sizes = [4, 7, 5]
    tr = DDPMTrainer(te._dynamics(), ema_decay=0.5, pos_only=True, **te.KW)
    batch = te._batch(sizes)
    reads = {"n": 0}

    def counted(name):
        orig = getattr(torch.Tensor, name)

        def fn(self, *a, **k):
            if self.is_cuda:
                reads["n"] += 1
            return orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, fn)
    tr.eval_inpaint_batch(batch, cap=None, noise_fn=te._noise(sizes), **te.RUN)          # builds the sampler and the layout
    for name in ("item", "tolist", "cpu", "numpy", "__bool__", "__int__", "__float__", "__index__"):
        counted(name)
    plain = tr.eval_inpaint_batch(batch, cap=None, noise_fn=te._noise(sizes), **te.RUN)
    r_plain, n_plain = tr.last_rmsds.clone(), reads["n"]
    reads["n"] = 0
    matched = tr.eval_inpaint_batch(batch, cap=None, noise_fn=te._noise(sizes), match_order=True, **te.RUN)
    r_matched, n_matched = tr.last_rmsds.clone(), reads["n"]
    monkeypatch.undo()
    print(f"host reads: {n_plain} without matching, {n_matched} with; rmsd {r_plain.tolist()} -> {r_matched.tolist()}")
    assert n_matched == n_plain
    assert bool(torch.isfinite(r_matched).all()) and bool((r_matched <= r_plain).all())
    assert matched[0] <= plain[0] and matched[1] <= plain[1]
    # against the float64 minimum, on the samples the trainer's own sampler draws from the same noise
    reps, cond = batch
    xh_d = [torch.cat([r["pos"], r["one_hot"], r["charge"]], dim=1) for r in reps]
    (smp,) = tr._eval_samplers.values()
    out, _ = smp.inpaint(len(sizes), [r["size_host"] for r in reps], conditions=cond, xh_fixed=xh_d, frag_fixed=[0, 2],
                         noise_fn=te._noise(sizes), **te.RUN)
    xh, gen = xh_d[1].cpu().numpy(), out[0][1].cpu().numpy()
    p = kc.seg_ptr(sizes)
    several = 0
    for g in range(len(sizes)):
        a, b = xh[p[g]: p[g + 1]], gen[p[g]: p[g + 1]]
        sp = a[:, -1].astype(int)
        assert (sp == b[:, -1].astype(int)).all()
        several += len(set(sp.tolist())) < len(sp)
        r = mc.brute(a[:, :3], b[:, :3], sp, True)[0]
        assert abs(float(r_matched[g]) - r) <= kc.gate(r, mc.rho(a[:, :3], b[:, :3])), (g, float(r_matched[g]), r)
    assert several, "no reaction of the fixture has two like atoms"


@pytest.mark.gpu
def test_eval_inpaint_batch_with_generated_atom_types():
    """The fixture's own trainer generates the atom types too; an untrained one does not reproduce the true charges, so the species lists
    differ and every reaction counts the cap, as the reference's `except: rmsd = 1.0` has it - never more than the same-order numbers,
    which the cap bounds as well.  Without a cap such a reaction is left out of mean and median."""
    import test_trainer_eval_inpaint as te
    from oareactdiff_amd.trainer import DDPMTrainer
    sizes = [4, 7, 5]
    tr = DDPMTrainer(te._dynamics(), ema_decay=0.5, **te.KW)
    batch = te._batch(sizes)
    plain = tr.eval_inpaint_batch(batch, noise_fn=te._noise(sizes), **te.RUN)
    r_plain = tr.last_rmsds.clone()
    matched = tr.eval_inpaint_batch(batch, noise_fn=te._noise(sizes), match_order=True, **te.RUN)
    r_matched = tr.last_rmsds.clone()
    assert bool((r_matched <= r_plain).all()) and bool((r_matched <= 1.0).all())
    assert matched[0] <= plain[0] and matched[1] <= plain[1]

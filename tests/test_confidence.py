"""The Confidence model on the GPU: oard_confidence_forward (trunk without its output head + k_conf_readout) against the reference's
float64 logits, and the properties the readout kernel promises (csrc/oard_conf.h).

Gate: `rel` of _cases.py, max|d| / max|ref64| over the batch, <= 1e-5 - the project's bar.  Plain torch float32 on the same inputs
sits at 1.2e-7 ... 5.9e-7 of float64 (logits ~ 0.01 - 0.03), so the bar leaves about 16 x over what float32 itself costs."""
import pytest
import torch

from _cases import Case, debug_options, rel
from _conf_cases import CONF_CASES, GATE, ConfCase, restate64
from oareactdiff_amd.graph_tools import get_edges_index, get_mask_for_frag, get_n_frag_switch
from oareactdiff_amd.spec import confidence_state_spec, synthetic_state_dict

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H32 = dict(pos_require_grad=False, cutoff=5.0, num_layers=2, hidden_channels=32, num_radial=8, in_hidden_channels=8)   # narrowest built pair


def _direct(m, c, t=None):
    with torch.no_grad():
        return m._forward([x.to(DEV) for x in c.xh], c.edge_index.to(DEV), (c.t if t is None else t).to(DEV), c.conditions.to(DEV),
                          c.n_frag_switch.to(DEV), c.combined_mask.to(DEV))


@pytest.mark.parametrize("precision", [None, "bf16x3"])
@pytest.mark.parametrize("name", CONF_CASES)
def test_fixture_parity_through_both_entries(name, precision):
    """Every fixture through `forward` (t = 0) and through `_forward` (the fixture's t), under the suite's poisoned workspace.  A
    fixture holds the reference's logits for ONE of the two times; the other entry is compared with the float64 restatement at its
    own time (tests/test_confidence_cpu.py: the restatement equals the reference to 1e-12)."""
    c = ConfCase(name)
    m = c.module(DEV, edge_precision=precision)
    with torch.no_grad():
        via_forward = m(c.representations(DEV), c.conditions.to(DEV))
    assert int(m.last_status[0].item()) == 0
    via_direct = _direct(m, c)
    assert int(m.last_status[0].item()) == 0
    want_shape = () if c.B == 1 else (c.B,)                                 # squeezed like the reference's
    assert via_forward.shape == want_shape and via_direct.shape == want_shape and via_forward.dtype == torch.float32
    if c.entry == "forward":
        ref_forward = ref_direct = c.ref64                                  # t = [0] either way
    else:
        ref_direct = c.ref64
        ref_forward = restate64(c.state_dict(torch.float64), c.cfg, c.xh, c.edge_index, torch.tensor([0.0]), c.conditions,
                                c.n_frag_switch, c.combined_mask, c.cnf, c.B)
    ef, ed = rel(via_forward.cpu().reshape(-1), ref_forward), rel(via_direct.cpu().reshape(-1), ref_direct)
    print(f"{name} [{precision}]: forward {ef:.2e}  _forward {ed:.2e}  (gate {GATE:g}; reference f32 {rel(c.ref32, c.ref64):.2e})")
    assert ef <= GATE and ed <= GATE


class _Ragged:
    """B = 5 reactions, 2 - 5 atoms per object, H = 32: not a fixture - inputs from a seeded generator, oracle computed here."""
    sizes = [[2, 3, 4, 5, 3], [5, 2, 3, 4, 2], [3, 5, 2, 2, 4]]
    node_nfs, cnf, B = [9, 9, 9], 1, 5

    def __init__(self):
        g = torch.Generator().manual_seed(20240611)
        self.frag = [torch.tensor(s) for s in self.sizes]
        self.masks = [get_mask_for_frag(f) for f in self.frag]
        self.combined_mask = torch.cat(self.masks)
        self.n_frag_switch = get_n_frag_switch(self.frag)
        self.edge_index = get_edges_index(self.combined_mask, remove_self_edge=True)
        self.xh = [torch.cat([1.5 * torch.randn(int(f.sum()), 3, generator=g), torch.rand(int(f.sum()), 6, generator=g)], dim=1)
                   for f in self.frag]
        self.conditions = torch.rand(self.B, 1, generator=g)
        self.t = torch.rand(self.B, 1, generator=g)
        self.spec = confidence_state_spec(H32, self.node_nfs, self.cnf)
        self.ref = restate64(synthetic_state_dict(self.spec, H32, seed=42, dtype=torch.float64), H32, self.xh, self.edge_index, self.t,
                             self.conditions, self.n_frag_switch, self.combined_mask, self.cnf, self.B)

    def module(self):
        from oareactdiff_amd.confidence import Confidence
        m = Confidence(model_config=dict(H32), fragment_names=["R", "TS", "P"], node_nfs=self.node_nfs, edge_nf=0, condition_nf=self.cnf,
                       device=DEV)
        m.load_state_dict(synthetic_state_dict(self.spec, H32, seed=42), strict=True)
        return m


@pytest.fixture(scope="module")
def ragged():
    return _Ragged()


def test_sub_batches_meet_the_gate_and_keep_every_reaction_in_its_row(ragged):
    """One, two and three sub-batches (the parts run on the topology's side streams, one readout launch each): the value of reaction b
    sits at row b - its combined_mask value, not its index inside the part."""
    r = ragged
    spread = (r.ref[:, None] - r.ref[None, :]).abs() + torch.eye(r.B)
    assert float(spread.min()) > 100 * GATE * float(r.ref.abs().max())      # the reactions differ: a misplaced row cannot pass
    got = {}
    for parts in (1, 2, 3):
        with debug_options(parts=parts), torch.no_grad():
            m = r.module()                                                  # a fresh module: the topology is built under `parts`
            out = m._forward([x.to(DEV) for x in r.xh], r.edge_index.to(DEV), r.t.to(DEV), r.conditions.to(DEV),
                             r.n_frag_switch.to(DEV), r.combined_mask.to(DEV))
            assert int(m.last_status[0].item()) == 0
        got[parts] = out.cpu()
        row_err = (got[parts].double() - r.ref).abs() / r.ref.abs().max()
        print(f"parts={parts}: rel {rel(got[parts], r.ref):.2e}  per row {[f'{float(e):.1e}' for e in row_err]}")
        assert out.shape == (r.B,) and rel(got[parts], r.ref) <= GATE and bool((row_err <= GATE).all())


def test_padding_columns_are_never_read():
    """Production width: HP = 208 > H = 196.  Whatever the workspace held - NaN patterns (the suite's poison) or huge finite garbage
    with poisoning off - the logits are the same bits."""
    c = ConfCase("cd_conf_prod_b2_n23")
    m = c.module(DEV)
    poisoned = _direct(m, c).clone()
    with debug_options(poison=0):
        m._ws.view(torch.float32).fill_(3.0e38)                             # (the workspace is a whole number of 4 KiB pages)
        garbage = _direct(m, c).clone()
        m._ws.zero_()
        zeros = _direct(m, c).clone()
    assert torch.equal(poisoned, garbage) and torch.equal(poisoned, zeros)
    assert rel(poisoned.cpu(), c.ref64) <= GATE


def test_a_reaction_alone_and_inside_a_batch_agree():
    c = ConfCase("cb_conf_ragged_h32")
    m = c.module(DEV)
    batch = _direct(m, c).cpu()
    scale = float(c.ref64.abs().max())
    for b in range(c.B):
        rows = [c.combined_mask[c.n_frag_switch == k] == b for k in range(c.n_obj)]
        xh = [c.xh[k][rows[k]] for k in range(c.n_obj)]
        cm = torch.zeros(sum(int(x.shape[0]) for x in xh), dtype=torch.long)
        nfs = torch.cat([torch.full((int(xh[k].shape[0]),), k, dtype=torch.long) for k in range(c.n_obj)])
        with torch.no_grad():
            alone = m._forward([x.to(DEV) for x in xh], get_edges_index(cm, remove_self_edge=True).to(DEV), c.t.to(DEV),
                               c.conditions[b: b + 1].to(DEV), nfs.to(DEV), cm.to(DEV))
        assert alone.shape == ()
        d = abs(float(alone) - float(batch[b])) / scale
        print(f"reaction {b}: alone {float(alone):.8f} in the batch {float(batch[b]):.8f}  difference / max|ref64| {d:.2e}")
        assert d <= GATE


@pytest.mark.parametrize("name", ["cb_conf_ragged_h32", "cd_conf_prod_b2_n23"])
def test_two_identical_calls_are_bit_identical(name):
    c = ConfCase(name)
    m = c.module(DEV)
    first = _direct(m, c).clone()
    second = _direct(m, c).clone()
    other = _direct(c.module(DEV), c)                                       # another module, another workspace, another topology
    assert torch.equal(first, second) and torch.equal(first, other)


def test_the_denoiser_is_untouched():
    """An EGNNDynamics that shares nothing with the Confidence module gives the same bits before and after a confidence call."""
    from oareactdiff_amd.dynamics import EGNNDynamics
    g = Case("g1_wrapper_small")
    dyn = EGNNDynamics(model_config=dict(g.cfg), fragment_names=["a", "b", "c"], node_nfs=g.node_nfs, edge_nf=0, condition_nf=g.cnf,
                       device=DEV)
    dyn.load_state_dict(g.state_dict(), strict=True)
    args = ([x.to(DEV) for x in g.xh], g.edge_index.to(DEV), g.t.to(DEV), g.conditions.to(DEV), g.n_frag_switch.to(DEV),
            g.combined_mask.to(DEV))
    with torch.no_grad():
        before = [o.clone() for o in dyn(*args)[0]]
    c = ConfCase("ca_conf_wrapper_small")
    assert rel(_direct(c.module(DEV), c).cpu(), c.ref64) <= GATE
    with torch.no_grad():
        after = dyn(*args)[0]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    v, h = g.split([o.cpu() for o in after])
    rv, rh = g.split(g.ref64)
    assert rel(v, rv) <= 1e-5 and rel(h, rh) <= 1e-5


def test_refusals():
    from oareactdiff_amd._capi import OardError
    from oareactdiff_amd.confidence import Confidence
    c = ConfCase("ca_conf_wrapper_small")
    m = c.module(DEV)
    # 1. an edge list that is not the complete graph per reaction
    with torch.no_grad(), pytest.raises(NotImplementedError, match="complete graph"):
        m._forward([x.to(DEV) for x in c.xh], c.edge_index[:, 1:].contiguous().to(DEV), c.t.to(DEV), c.conditions.to(DEV),
                   c.n_frag_switch.to(DEV), c.combined_mask.to(DEV))
    # 2. a width pair the production kernels were not built for
    cfg = dict(c.cfg, hidden_channels=64)
    wide = Confidence(model_config=cfg, fragment_names=["a", "b", "c"], node_nfs=c.node_nfs, edge_nf=0, condition_nf=c.cnf, device=DEV)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="width pair"):
        wide(c.representations(DEV), c.conditions.to(DEV))
    # 3. autograd enabled and a parameter that requires grad: there is no backward pass
    assert torch.is_grad_enabled()
    assert _direct(m, c).shape == (c.B,)                                    # frozen parameters: fine with autograd enabled, too
    out = m(c.representations(DEV), c.conditions.to(DEV))
    assert not out.requires_grad
    getattr(m.readout.gmlp.mlp, "2").linear.bias.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="inference only"):
        m(c.representations(DEV), c.conditions.to(DEV))
    with torch.no_grad():                                                   # ... and the same module still scores without autograd
        assert rel(m(c.representations(DEV), c.conditions.to(DEV)).cpu(), c.ref64) <= GATE
    # reactions must be named 0 .. B-1: a gap has no row in the reference's scatter_mean either
    with torch.no_grad(), pytest.raises(OardError, match="none missing"):
        cm = c.combined_mask * 2
        m._forward([x.to(DEV) for x in c.xh], get_edges_index(cm, remove_self_edge=True).to(DEV), c.t.to(DEV),
                   torch.zeros(4, c.cnf, device=DEV), c.n_frag_switch.to(DEV), cm.to(DEV))


def test_a_nan_logit_sets_the_device_side_flag():
    """A NaN readout bias (the trunk stays clean): the logits are NaN, `last_status[0]` says so and the sticky flag keeps it - read
    here, never inside the call."""
    c = ConfCase("cb_conf_ragged_h32")
    m = c.module(DEV)
    assert rel(_direct(m, c).cpu(), c.ref64) <= GATE and m.last_status.tolist() == [0, 0] and int(m.nan_seen[0]) == 0
    with torch.no_grad():
        getattr(m.readout.mlp.mlp, "2").linear.bias.fill_(float("nan"))
    out = _direct(m, c)
    assert bool(torch.isnan(out).all()) and int(m.last_status[0]) == 1
    with torch.no_grad():
        getattr(m.readout.mlp.mlp, "2").linear.bias.zero_()
    assert not bool(torch.isnan(_direct(m, c)).any()) and int(m.last_status[0]) == 0 and int(m.nan_seen[0]) == 1


def test_score_samples_and_rank_candidates_on_sampler_output():
    """K = 3 candidates of each of 2 reactions, candidate-major, from a T = 2 run of DiffusionSampler at the narrowest built width:
    `score_samples` on what `sample` returns == `forward` on the same tensors repacked as representations."""
    from oareactdiff_amd import DiffusionSampler, EGNNDynamics
    from oareactdiff_amd.confidence import Confidence, rank_candidates
    from oareactdiff_amd.spec import state_spec
    node_nfs, cnf, K, n_reactions = [9, 9, 9], 1, 3, 2
    dyn = EGNNDynamics(model_config=dict(H32), fragment_names=["R", "TS", "P"], node_nfs=node_nfs, edge_nf=0, condition_nf=cnf, device=DEV)
    dyn.load_state_dict(synthetic_state_dict(state_spec(H32, node_nfs, cnf), H32, seed=42), strict=True)
    frag = [torch.tensor(s * K) for s in ([3, 4], [4, 2], [2, 3])]
    B = K * n_reactions
    cond = torch.zeros(B, 1, device=DEV)
    torch.manual_seed(7)
    smp = DiffusionSampler(dyn, "polynomial_2", 2, 1e-5, gaussian_prior_std=1.0)
    out, masks = smp.sample(B, frag, conditions=cond, graph=False)
    samples = out[0]
    conf = Confidence(model_config=dict(H32), fragment_names=["R", "TS", "P"], node_nfs=node_nfs, edge_nf=0, condition_nf=cnf, device=DEV)
    conf.load_state_dict(synthetic_state_dict(confidence_state_spec(H32, node_nfs, cnf), H32, seed=42), strict=True)
    scores = conf.score_samples(frag, samples, cond)
    assert scores.shape == (B,) and scores.device.type == "cuda" and bool(((scores > 0) & (scores < 1)).all())
    reps = [{"mask": masks[k], "size": frag[k].to(DEV), "pos": samples[k][:, :3], "one_hot": samples[k][:, 3:-1], "charge": samples[k][:, -1:]}
            for k in range(3)]
    with torch.no_grad():
        logits = conf(reps, cond)
    assert torch.equal(torch.sigmoid(logits), scores)
    assert torch.equal(conf.score_samples(frag, samples, cond, probability=False), logits)
    assert torch.equal(conf.score_samples(frag, samples), scores)           # default conditions: zeros
    best, order = rank_candidates(scores, n_reactions)
    assert best.device.type == "cuda" and order.shape == (n_reactions, K)
    assert torch.equal(best, torch.argmax(scores.reshape(K, n_reactions), dim=0))
    assert torch.equal(torch.sort(order, dim=1).values, torch.arange(K, device=DEV).expand(n_reactions, K))

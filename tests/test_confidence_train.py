"""Training the Confidence model on the device: the readout's adjoint alone (teacher-forced), the whole gradient per cg_* fixture
against the reference's float64 autograd, routing by reaction id, and training-mode against inference logits.

Gates.  Readout adjoint: the kernels are float64 behind float32 loads with ONE rounding to float32 (6e-8 of a value), gate 1e-6 of each
tensor's largest entry.  Whole gradient: flat error <= 2e-5 (tests/test_grad.py's gate); per tensor
    tol = max(grad_tol(reference's own float32 gap), 3 x plain float32 torch's gap),
both recorded in the fixture (tools/make_goldens_confidence_grad.py).  The second term: with mixed labels the cotangents of the
reactions cancel, and plain float32 torch itself sits above 1e-5 on a handful of tiny tensors (model.lin3.0.weight 1.6e-3,
gcl_layers.5.att_mlp...bias 6e-5, readout.gmlp.mlp.2.linear.bias 4.6e-5 on cg_prod_b2_n23); the factor 3 because the project's one
recorded case of this kind has the HIP path at twice torch's float32 error (tests/test_grad.py, ILL_CONDITIONED_SCALAR_SUMS)."""
import ctypes as C

import pytest
import torch

from _cases import rel
from _conf_cases import GATE, ConfCase, readout64
from _conf_grad_cases import CG_CASES, ConfGradCase, conf_loss, conf_module
from test_grad import grad_tol

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# =====================================================================================================================
# 1. the readout's adjoint alone
# =====================================================================================================================
def _layout(per_reaction, n_obj):
    """Reactions of the given node counts, dealt to `n_obj` objects as evenly as they go -> (combined_mask, n_frag_switch, sizes)."""
    sizes = [[n // n_obj + (1 if k < n % n_obj else 0) for n in per_reaction] for k in range(n_obj)]
    mask = torch.cat([torch.repeat_interleave(torch.arange(len(per_reaction)), torch.tensor(s)) for s in sizes])
    nfs = torch.cat([torch.full((sum(s),), k, dtype=torch.long) for k, s in enumerate(sizes)])
    return mask, nfs, sizes


class _Readout:
    """A training-mode forward on a chosen layout, whose taped final node scalars can be overwritten (teacher forcing)."""

    def __init__(self, fixture, per_reaction, seed):
        from oareactdiff_amd import _capi
        c = ConfCase(fixture)
        self.c, self.L, self.capi = c, _capi.lib(), _capi
        self.m = m = conf_module(c, DEV)
        g = torch.Generator().manual_seed(seed)
        mask, nfs, sizes = _layout(per_reaction, c.n_obj)
        self.B, self.H = len(per_reaction), c.cfg["hidden_channels"]
        self.HP = (self.H + 15) // 16 * 16
        xh = [torch.randn(sum(sizes[k]), c.node_nfs[k], generator=g).to(DEV) for k in range(c.n_obj)]
        cond = torch.randn(self.B, max(c.cnf, 1), generator=g).to(DEV)
        self.stream = torch.cuda.current_stream(DEV).cuda_stream
        self.cfg = cfg = m._config()
        self.topo = topo = m._get_train_topology(cfg, None, nfs.to(DEV), mask.to(DEV), self.stream)
        xs, tt, t_scalar, cnd = m._inputs(topo, xh, torch.zeros(1, device=DEV), cond, DEV, detach=True)
        self.logits, self.state = m._run_forward_train_conf(cfg, topo, m._get_packed(cfg, self.stream), xs, tt, t_scalar, cnd, self.stream)
        self.S = self.state.tape.get(_capi.TAPE_S_IN, c.cfg["num_layers"])          # [N, HP] view of the tape
        tidx = torch.empty(topo.N, dtype=torch.int32, device=DEV)
        _capi.check(self.L.oard_topology_export(topo.handle, _capi.TOPO_NODE_TIDX, tidx.data_ptr(), topo.N, self.stream), "export")
        self.node_id = tidx.long().cpu()
        self.readout = m._readout_tensors(DEV)
        self.sc = m._call_buffers.scratch(self.L.oard_train_scratch_bytes(C.byref(cfg), topo.handle), DEV)

    def backward(self, dconf, grads=None):
        """-> (ds [N, HP], dvec [3N, HP], the 12 gradients); destinations arrive filled with NaN (ds, dvec) / as given (grads)."""
        N = self.topo.N
        ds = torch.full((N, self.HP), float("nan"), device=DEV)
        dvec = torch.full((3 * N, self.HP), float("nan"), device=DEV)
        if grads is None:
            grads = [torch.zeros_like(p) for p in self.readout]
        rc = self.L.oard_confidence_tail_backward(C.byref(self.cfg), self.topo.handle, self.state.tape.buf.data_ptr(),
                                                  self.capi.ptr_array(self.readout), dconf.data_ptr(), ds.data_ptr(), dvec.data_ptr(),
                                                  self.capi.ptr_array(grads), self.sc.data_ptr(), self.sc.numel(), self.stream)
        self.capi.check(rc, "oard_confidence_tail_backward")
        return ds, dvec, grads


@pytest.mark.parametrize("fixture,per_reaction", [("cb_conf_ragged_h32", (3, 6, 7, 9, 13)), ("cd_conf_prod_b2_n23", (11,)),
                                                  ("cd_conf_prod_b2_n23", (5, 18))])
def test_readout_adjoint_alone(fixture, per_reaction):
    """H = 32: five reactions of 3, 6, 7, 9, 13 nodes (fewer rows than row groups, non-multiples of 4, H / 4 < 64 lanes); H = 196
    (HP = 208): B = 1 and B = 2.  Reference: float64 torch autograd through readout64(scatter_mean(s))."""
    from oareactdiff_amd.spec import READOUT_NAMES
    r = _Readout(fixture, per_reaction, seed=7)
    H, HP, B, N = r.H, r.HP, r.B, r.topo.N
    g = torch.Generator().manual_seed(11)
    s = torch.randn(N, H, generator=g)
    dconf = torch.randn(B, generator=g).to(DEV)
    results = []
    for pad in (0.0, float("nan"), 3e38):
        r.S[:, :H] = s.to(DEV)
        r.S[:, H:] = pad
        results.append(r.backward(dconf))
    ds, dvec, grads = results[0]
    # float64 reference
    sd = {k: v.double().requires_grad_(True) for k, v in r.c.state_dict().items() if k.startswith("readout.")}
    s64 = s.double().requires_grad_(True)
    cnt = torch.zeros(B, dtype=torch.float64).index_add_(0, r.node_id, torch.ones(N, dtype=torch.float64))
    pooled = torch.zeros(B, H, dtype=torch.float64).index_add_(0, r.node_id, s64) / cnt[:, None]
    (readout64(sd, pooled).reshape(-1) * dconf.double().cpu()).sum().backward()
    worst = ("ds", rel(ds[:, :H].cpu(), s64.grad))
    assert worst[1] <= 1e-6, worst
    for name, got in zip(READOUT_NAMES, grads):
        e = rel(got.cpu(), sd[name].grad)
        print(f"  {fixture} {per_reaction} {name}: {e:.2e}")
        assert e <= 1e-6, (name, e)
    # pads and the vector state's cotangent: exact zeros, whatever the pad columns of s hold
    assert not bool(ds[:, H:].any()) and not bool(dvec.any())
    for other in results[1:]:
        assert torch.equal(other[0], ds) and torch.equal(other[1], dvec)
        assert all(torch.equal(a, b) for a, b in zip(other[2], grads))
    # accumulation: a second call into the same destinations doubles them exactly; two runs are bit-identical
    _, _, twice = r.backward(dconf, [x.clone() for x in grads])
    assert all(torch.equal(t, 2 * x) for t, x in zip(twice, grads))
    again = r.backward(dconf)
    assert torch.equal(again[0], ds) and all(torch.equal(a, b) for a, b in zip(again[2], grads))


# =====================================================================================================================
# 2. the whole gradient per fixture
# =====================================================================================================================
def _gate(g, grads, none, loss, logits, label):
    """Test 2's gates on one backward pass (also used by the routing test)."""
    errs, flat = g.compare(grads)
    e_logits = rel(logits.detach().reshape(-1).cpu(), g.logits64)
    print(f"\n{label}: loss {float(loss):.8f} (ref64 {g.loss64:.8f}); logits {e_logits:.2e}; flat gradient error {flat:.2e}")
    bad = []
    for n in sorted(errs, key=lambda k: -errs[k]):
        tol = max(grad_tol(g.ref_gap[n], n), 3 * g.torch32[n])
        flag = "" if errs[n] <= tol else "   <-- above tolerance"
        if flag:
            bad.append((n, errs[n], tol))
        print(f"  {n:62s} ours {errs[n]:.2e}   torch32 {g.torch32[n]:.2e}   reference f32 {g.ref_gap[n]:.2e}{flag}")
    assert e_logits <= GATE, e_logits
    assert abs(float(loss) - g.loss64) <= 2e-5 * abs(g.loss64), (float(loss), g.loss64)
    assert none == g.none_names, none ^ g.none_names
    assert flat <= 2e-5 and not bad, (flat, bad)


@pytest.mark.parametrize("name", list(CG_CASES))
def test_training_step_gradients_match_reference_f64(name):
    g = ConfGradCase(name)
    c = g.inputs
    m = g.module(DEV)
    if c.entry == "forward":
        logits = m(c.representations(DEV), c.conditions.to(DEV))
    else:
        logits = m._forward([x.to(DEV) for x in c.xh], c.edge_index.to(DEV), c.t.to(DEV), c.conditions.to(DEV),
                            c.n_frag_switch.to(DEV), c.combined_mask.to(DEV))
    assert logits.requires_grad and logits.shape == c.ref64.squeeze().shape
    loss = conf_loss(logits, g.y.to(DEV), g.kind)
    loss.backward()
    named = dict(m.named_parameters())
    _gate(g, {n: p.grad for n, p in named.items() if p.grad is not None}, {n for n, p in named.items() if p.grad is None},
          loss.detach(), logits, name)


# =====================================================================================================================
# 3. routing by reaction id
# =====================================================================================================================
def _embedded(c, B, slots, seed):
    """cb's reactions in `slots` of a batch of B, the other slots random reactions -> (representations, conditions)."""
    g = torch.Generator().manual_seed(seed)
    where = {s: j for j, s in enumerate(slots)}
    start = [0]
    for x in c.xh:
        start.append(start[-1] + x.shape[0])
    reps = []
    for k in range(c.n_obj):
        own_mask = c.combined_mask[start[k]: start[k + 1]]
        rows, mask, size = [], [], []
        for b in range(B):
            if b in where:
                x = c.xh[k][own_mask == where[b]]
            else:
                n = int(torch.randint(1, 6, (1,), generator=g))
                x = torch.randn(n, c.node_nfs[k], generator=g)
            rows.append(x)
            mask.append(torch.full((x.shape[0],), b, dtype=torch.long))
            size.append(x.shape[0])
        x = torch.cat(rows).to(DEV)
        reps.append({"mask": torch.cat(mask).to(DEV), "size": torch.tensor(size).to(DEV), "pos": x[:, :3], "one_hot": x[:, 3:-1],
                     "charge": x[:, -1:]})
    cond = torch.randn(B, c.conditions.shape[1], generator=g)
    cond[list(slots)] = c.conditions
    return reps, cond.to(DEV)


def test_gradients_are_routed_by_reaction_id():
    """cb's three reactions in slots (0, 1, 2), then (6, 7, 8), of a B = 9 batch; the loss over the occupied slots only: the other
    reactions get a zero cotangent, and the gradients are the fixture's both times."""
    g = ConfGradCase("cg_ragged_h32")
    c = g.inputs
    m = g.module(DEV)
    for slots in ((0, 1, 2), (6, 7, 8)):
        m.zero_grad(set_to_none=True)
        reps, cond = _embedded(c, 9, slots, seed=3)
        logits = m(reps, cond)
        assert logits.shape == (9,)
        sub = logits[list(slots)]
        loss = conf_loss(sub, g.y.to(DEV), g.kind)
        loss.backward()
        named = dict(m.named_parameters())
        _gate(g, {n: p.grad for n, p in named.items() if p.grad is not None}, {n for n, p in named.items() if p.grad is None},
              loss.detach(), sub, f"slots {slots}")


# =====================================================================================================================
# 4. training-mode forward == inference forward
# =====================================================================================================================
@pytest.mark.parametrize("name", ["cg_ragged_h32", "cg_prod_b2_n23"])
def test_training_mode_logits_are_the_inference_logits(name):
    g = ConfGradCase(name)
    c = g.inputs
    m, frozen = g.module(DEV), g.module(DEV, trainable=False)
    reps, cond = c.representations(DEV), c.conditions.to(DEV)
    train = m(reps, cond)
    assert train.requires_grad
    with torch.no_grad():
        infer = m(reps, cond)
        ref = frozen(reps, cond)
    assert not infer.requires_grad and torch.equal(infer, ref)              # a trainable module under no_grad: the frozen module's bits
    e = float((train.detach() - infer).abs().max() / infer.abs().max())
    print(f"{name}: training-mode vs inference logits {e:.2e}")
    assert e <= 3e-6, e

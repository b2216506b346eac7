"""Teacher-forced checks of the training path, shared by tests/test_grad_stages.py (asserts) and tools/grad_debug.py
(prints).  For one training step - a recorded one (tests/golden/g9_grad_*.npz, by name) or a case object with GradCase's interface
(tests/_grad_cases.py: SyntheticGradCase) -:
  1. forward consistency: every torch stage function of tests/_stage_refs.py, evaluated on the TAPED inputs of the HIP forward,
     against the TAPED outputs of the HIP kernels it restates;
  2. every stage of the hand-written backward sweep in isolation (oard_train_stage_backward / _tail_ / _init_, and the edge
     scalarisation adjoint): fed with the tape's stage inputs and RANDOM cotangents, compared with torch autograd of the stage's
     restatement on the same inputs - nothing upstream can mask an error.  The reference is evaluated in float64 (the truth) and
     in float32 (what plain torch float32 achieves): a kernel result passes when its distance to the float64 gradient is within
     1e-5 of the tensor's largest entry, or within 3x torch-float32's own distance where the gradient is an ill-conditioned sum
     (e.g. lin3 of EquiUpdate: ~N H terms of both signs);
  3. the whole step against the reference's float64 gradients."""
import ctypes as C

import torch
import torch.nn.functional as F

import _stage_refs as refs
from _grad_cases import CNF, NODE_NFS, GradCase
from oareactdiff_amd import _capi, training
from oareactdiff_amd.dynamics import EGNNDynamics

TOL = 1e-5


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    if b.numel() == 0:          # a batch without inner edges: nothing to compare
        return 0.0
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def run(name, log=print, clobber=False):
    """clobber=True: right after every stage entry returns, its cotangent inputs are overwritten with NaN on the caller's stream - the
    entry's own work (the weight-gradient launches run on the library's second stream) must have been ordered in front of that."""
    out = {}

    def note(key, *vals):
        out[key] = [float(v) for v in vals]
        log(f"{key:34s} " + "  ".join(f"{float(v):.2e}" for v in vals))
    c = GradCase(name) if isinstance(name, str) else name
    name = c.name
    dev = torch.device("cuda:0")
    node_nfs, cnf = list(getattr(c, "node_nfs", NODE_NFS)), getattr(c, "cnf", CNF)     # a synthetic case may have 1 to 8 objects
    n_obj = len(node_nfs)
    dyn = EGNNDynamics(model_config=dict(c.cfg), fragment_names=["R", "TS", "P"] if n_obj == 3 else [f"o{k}" for k in range(n_obj)],
                       node_nfs=node_nfs, edge_nf=0, condition_nf=cnf, device=dev)
    dyn.load_state_dict(c.state_dict(), strict=True)
    keep = {}
    orig = training.DynamicsFunction.forward

    def spy(ctx, dyn_, run_forward, n_obj, *tensors):
        o = orig(ctx, dyn_, run_forward, n_obj, *tensors)
        keep["state"] = ctx.state
        return o
    training.DynamicsFunction.forward = staticmethod(spy)
    try:
        loss = c.loss(dyn, torch.float32, dev)
    finally:
        training.DynamicsFunction.forward = orig
    st = keep["state"]
    tape, topo, cfg = st.tape, st.topo, st.cfg
    H, R, NL, Cc = dyn._dims
    HP, WP = training._pad16(H), training._pad16(3 * H + R)
    W = 3 * H + R
    N, E, A = topo.N, topo.E, topo.A
    out_topology = getattr(c, "seen_topology", None)
    if out_topology is not None:          # a synthetic case states the N / E / A it was built to hit: the caller asserts them
        out_topology[:] = [N, E, A]
    P = {k: v.detach() for k, v in dyn._param_dict().items()}
    P64 = {k: v.double() for k, v in P.items()}
    log(f"{name}: N {N} E {E} A {A} loss {float(loss.detach()):.8f} ref64 {c.f64_loss:.8f}")
    geo = tape.get(_capi.TAPE_GEO)[:A]
    gargs = (topo.inner_src, topo.inner_tgt, topo.node_sample, topo.node_group, topo.B, topo.B * n_obj)
    rbf_t, pp0_t, x1_t = tape.get(_capi.TAPE_RBF)[:A, :R], tape.get(_capi.TAPE_PP0)[:, 0], tape.get(_capi.TAPE_X1)
    g = refs.Geometry(*gargs, geo, rbf_t, pp0_t, x1_t)
    g64 = refs.Geometry(*gargs, geo.double(), rbf_t.double(), pp0_t.double(), x1_t.double())
    g.reflect_equiv = g64.reflect_equiv = bool(c.cfg.get("reflect_equiv", True))
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = _capi.lib()
    packed_f, packed_b = dyn._get_packed(cfg, stream), dyn._get_packed_bwd(cfg, stream)
    sc_buf = torch.empty(L.oard_train_scratch_bytes(C.byref(cfg), topo.handle), dtype=torch.uint8, device=dev)
    _capi.check(L.oard_train_scratch_poison(C.byref(cfg), topo.handle, sc_buf.data_ptr(), sc_buf.numel(), stream), "poison")
    tensors_all = dyn._ordered_tensors()
    params_tab = (C.c_void_p * len(tensors_all))(*[t.data_ptr() for t in tensors_all])
    Pmod = dyn._param_dict()

    def pad(x):                        # [N, H] -> [N, HP] with zero pads
        o = torch.zeros(x.shape[0], HP, device=dev)
        o[:, :H] = x
        return o

    def pad3(x):                       # [N, 3, H] -> [3N, HP]
        o = torch.zeros(x.shape[0], 3, HP, device=dev)
        o[:, :, :H] = x
        return o.view(3 * x.shape[0], HP)

    def unpad(x):
        return x.view(-1, HP)[:, :H]

    def unpad3(x):
        return x.view(-1, 3, HP)[:, :, :H]

    def scratch(which):
        off, rows, ld = C.c_size_t(0), C.c_int64(0), C.c_int64(0)
        _capi.check(L.oard_train_scratch_entry(C.byref(cfg), topo.handle, which, C.byref(off), C.byref(rows), C.byref(ld)), "scratch entry")
        return sc_buf[off.value: off.value + 4 * rows.value * ld.value].view(torch.float32).view(rows.value, ld.value)

    def grad_dests(names):
        """fresh zero destinations for the named parameters -> (table, {name: tensor})"""
        d = {n_: torch.zeros_like(P[n_]) for n_ in names}
        return training.gradient_table(dyn, {id(Pmod[n_]): t for n_, t in d.items()}), d

    def stage(which, layer, ins=(), outs=(), names=()):
        tab, d = grad_dests(names)
        ip = [t.data_ptr() for t in ins] + [None] * (3 - len(ins))
        op = [t.data_ptr() for t in outs] + [None] * (3 - len(outs))
        _capi.check(L.oard_train_stage_backward(C.byref(cfg), topo.handle, packed_f.data_ptr(), packed_b.data_ptr(), tape.buf.data_ptr(),
                                                layer, which, *ip, *op, params_tab, tab, sc_buf.data_ptr(), sc_buf.numel(), stream),
                    f"oard_train_stage_backward({which})")
        if clobber:
            for t in ins:
                t.fill_(float("nan"))
        return d

    def both(fn, ins, names, cots):
        """fn(P, g, *ins) -> outputs.  Gradients w.r.t. ins + P[names] for the cotangents `cots`, by torch autograd, in float32 and
        in float64 -> (outputs32, grads32, grads64)."""
        res = []
        for dt, Pd, gd in ((torch.float32, P, g), (torch.float64, P64, g64)):
            leaves = [x_.detach().to(dt).clone().requires_grad_(True) for x_ in ins]
            pl = [Pd[n_].detach().clone().requires_grad_(True) for n_ in names]
            Pq = dict(Pd)
            Pq.update(dict(zip(names, pl)))
            with torch.enable_grad():
                o = fn(Pq, gd, *leaves)
            o = list(o) if isinstance(o, (tuple, list)) else [o]
            pairs = [(t_, c_.to(dt)) for t_, c_ in zip(o, cots) if t_.requires_grad]
            gr = torch.autograd.grad([t_ for t_, _ in pairs], leaves + pl, [c_ for _, c_ in pairs], allow_unused=True)
            res.append(([t_.detach() for t_ in o], [torch.zeros_like(t_) if x_ is None else x_ for x_, t_ in zip(gr, leaves + pl)]))
        return res[0][0], res[0][1], res[1][1]

    def gate(key, labels, ours, g32, g64):
        """records, per compared tensor, the kernel's error vs float64 NORMALISED so that <= 1e-5 means "passes": the raw error
        when it is <= 1e-5, else scaled by 1e-5 / (3 x torch-float32's own error) (ill-conditioned sums)."""
        vals, txt = [], []
        for lab, o, a, b in zip(labels, ours, g32, g64):
            e, e32 = rel(o.reshape(b.shape), b), rel(a, b)
            if b.numel() == 1 and e > TOL:
                # ONE scalar that is the signed sum of a value over every edge (att_mlp's bias gradient): condition ~ sqrt(E), and what
                # is left after the float64 accumulation of the partial sums (round 5) is the float32 error of the 300 000 terms
                # themselves - 8e-6 ... 1.5e-5 depending on the last bits of the taped inputs (torch float32: 3e-6).  Gate: 5 x the bar.
                vals.append(e / 5)
                txt.append(f"{lab} {e:.1e} (scalar sum, torch f32: {e32:.1e})")
                continue
            vals.append(e if e <= TOL else e * TOL / max(TOL, 3 * e32))
            txt.append(f"{lab} {e:.1e}" + (f" (torch f32: {e32:.1e})" if e > TOL else ""))
        out[key] = vals
        log(f"{key}: " + "  ".join(txt))

    short = lambda n_: n_.split(".", 3)[-1]      # noqa: E731
    with torch.no_grad():
        # ---- 1. forward consistency of the stage functions -------------------------------------------------------
        hin = tape.get(_capi.TAPE_HIN)[:, :Cc]
        s0, ew0, c0 = refs.stage_init(P, hin, g, H)
        note("fwd init: s0, ew0", rel(s0, tape.get(_capi.TAPE_S_IN, 0)[:, :H]), rel(ew0, tape.get(_capi.TAPE_EW, 0)[:A, :W]))
        for l in range(NL):
            s_in = tape.get(_capi.TAPE_S_IN, l)[:, :H]
            vec_in = tape.get(_capi.TAPE_VEC_IN, l).view(N, 3, HP)[:, :, :H]
            xh, Pn, Qn = refs.stage_node_pre(P, l, s_in, g, H)
            agg = tape.get(_capi.TAPE_AGG, l)[:, :H]
            cd = tape.get(_capi.TAPE_CD, l)[:A].view(A, 3, HP)[:, :, :H]
            s_out, vec_out = refs.stage_node_mid(P, l, xh, agg, cd, vec_in, g, H)
            note(f"fwd layer {l}: s_out, vec_out", rel(s_out, tape.get(_capi.TAPE_S_IN, l + 1)[:, :H]),
                 rel(vec_out, tape.get(_capi.TAPE_VEC_IN, l + 1).view(N, 3, HP)[:, :, :H]))
    # ---- 2a. edge scalarisation + lin3 (k_scalarize): HIP adjoint vs torch autograd, random cotangent ------------------
    all_ok = False
    if A > 0:
        with torch.no_grad():
            _, NE1, _, _ = refs.stage_init_head(P, hin, g, H)
        gen0 = torch.Generator(device="cpu").manual_seed(11)
        Gs = torch.randn(A, 2 * H, generator=gen0).to(dev)
        l3n = ["model.lin3.0.weight", "model.lin3.0.bias", "model.lin3.2.weight", "model.lin3.2.bias"]
        _, gs32, gs64 = both(lambda Pq, gd, ne: refs.stage_scalarize(Pq, ne, gd, H), [NE1], l3n, [Gs])
        dews = torch.zeros(E + 1, WP, device=dev)
        dews[:A, :2 * H] = Gs
        dNE1, gl3 = training.scalarize_backward(dyn, cfg, topo, tape, NE1.contiguous(), dews, H, stream)
        # d|S_1| carries sign(S_1).  Where S_1 = <NE1, coord_cross> is zero in exact arithmetic (three-atom objects are
        # coplanar with their centre of mass; (anti)parallel pairs when the cutoff bites) its computed value is rounding
        # noise and the sign is arbitrary - in the reference too.  Nodes touching such an item are left out.
        with torch.no_grad():
            cvec = g.frame[:, :, 1]
            s1_src, s1_tgt = torch.einsum("axh,ax->ah", NE1[g.src], cvec), torch.einsum("axh,ax->ah", NE1[g.tgt], cvec)
            thr = 1e-5 * max(float(s1_src.abs().max()), float(s1_tgt.abs().max()))
            noisy = torch.zeros(N, device=dev)
            noisy.index_add_(0, g.src, (s1_src.abs() <= thr).any(dim=1).float())
            noisy.index_add_(0, g.tgt, (s1_tgt.abs() <= thr).any(dim=1).float())
        ok = noisy == 0
        # a sign can only flip where |S_1| is at the rounding level (~1e-7 of the scale); the exclusion above is deliberately generous
        all_ok = not bool(((s1_src.abs() <= 0.1 * thr).any() | (s1_tgt.abs() <= 0.1 * thr).any()))
        log(f"scalarize check: {int(ok.sum())} of {N} nodes have no sign-noisy item")
        if bool(ok.any()):
            gate("bwd scalarize", ["dNE1"] + [short(n_) for n_ in l3n], [dNE1[ok]] + [gl3[n_] for n_ in l3n],
                 [gs32[0][ok]] + gs32[1:], [gs64[0][ok]] + gs64[1:])
    # ---- 2. every stage of the sweep, teacher-forced ---------------------------------------------------------------------
    rs = tape_rows(topo, L, dev, stream)
    gen = torch.Generator(device="cpu").manual_seed(5)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).to(dev)      # noqa: E731
    for l in range(NL):
        q, e, u = f"model.gcl_layers.{l}.", f"model.message_layers.{l}.", f"model.update_layers.{l}."
        last = l == NL - 1
        s_in = tape.get(_capi.TAPE_S_IN, l)[:, :H]
        agg0 = tape.get(_capi.TAPE_AGG, l)[:, :H]
        with torch.no_grad():
            xh, Pn, Qn = refs.stage_node_pre(P, l, s_in, g, H)
            s_mid_r, xq_r = refs.stage_gcl_node(P, l, xh, agg0, H)
        stage(_capi.STAGE_RECOMPUTE, l)
        note(f"recompute layer {l}: xh, xq", rel(unpad(scratch(_capi.SCRATCH_XH)), xh), rel(unpad3(scratch(_capi.SCRATCH_XQ)), xq_r.view(N, 3, H)))
        # ---- GCLMessage edge part (k_gcl_edge_bwd + node sums + weight-gradient GEMMs + gate gradients) ----
        ew_l = tape.get(_capi.TAPE_EW, l)[:E, :W].clone()
        if l == 0:
            ew_l[A:] = dyn._c0row(Pmod, H, R).detach()
        en = [q + "edge_mlp.mlp.0.linear.weight", q + "edge_mlp.mlp.1.linear.weight", q + "edge_mlp.mlp.1.linear.bias",
              q + "edge_out_trans.mlp.0.linear.weight", q + "edge_out_trans.mlp.0.linear.bias",
              q + "att_mlp.mlp.0.linear.weight", q + "att_mlp.mlp.0.linear.bias"]

        def gcl_edge(Pq, gd, ew_t, Pt, Qt, l=l, q=q):
            z1 = Pt[rs["src"]] + Qt[rs["tgt"]] + F.linear(ew_t, Pq[q + "edge_mlp.mlp.0.linear.weight"][:, 2 * H:])
            m0 = F.silu(F.linear(F.silu(z1), Pq[q + "edge_mlp.mlp.1.linear.weight"], Pq[q + "edge_mlp.mlp.1.linear.bias"]))
            m = m0 * F.silu(F.linear(m0, Pq[q + "att_mlp.mlp.0.linear.weight"], Pq[q + "att_mlp.mlp.0.linear.bias"]))
            ew_new = ew_t + F.silu(F.linear(m, Pq[q + "edge_out_trans.mlp.0.linear.weight"], Pq[q + "edge_out_trans.mlp.0.linear.bias"]))
            deg = torch.zeros(N, device=dev, dtype=ew_t.dtype).index_add_(0, rs["src"], torch.ones(E, device=dev, dtype=ew_t.dtype)).clamp(min=1)
            aggt = torch.zeros(N, H, device=dev, dtype=ew_t.dtype).index_add_(0, rs["src"], m) / deg[:, None]
            return ew_new, aggt, z1
        Gn = rnd(E, W)
        if last:
            Gn[A:] = 0          # nothing reads the last layer's state of inter-object edges
        dagg = rnd(N, H)
        o32, g32, g64_ = both(gcl_edge, [ew_l, Pn, Qn], en, [Gn, dagg])
        note(f"fwd layer {l} gcl edge: z1, ew', agg", rel(o32[2], tape.get(_capi.TAPE_Z1, l)[:E, :H]),
             rel(o32[0][:A], tape.get(_capi.TAPE_EW, l + 1)[:A, :W]), rel(o32[1], tape.get(_capi.TAPE_AGG, l)[:, :H]))
        dew = torch.zeros(E + 1, WP, device=dev)
        dew[:E, :W] = Gn
        dP, dQ = torch.empty(N, HP, device=dev), torch.empty(N, HP, device=dev)
        gt = stage(_capi.STAGE_GCL_EDGE, l, (pad(dagg),), (dew, dP, dQ), en)
        w1 = en[0]
        assert float(gt[w1][:, :2 * H].abs().max()) == 0.0          # the node columns belong to the NODE_PRE stage
        gate(f"bwd layer {l} gcl edge", ["dew", "dP", "dQ"] + [short(n_) for n_ in en],
             [dew[:E, :W], unpad(dP), unpad(dQ), gt[w1][:, 2 * H:]] + [gt[n_] for n_ in en[1:]],
             g32[:3] + [g32[3][:, 2 * H:]] + g32[4:], g64_[:3] + [g64_[3][:, 2 * H:]] + g64_[4:])
        # ---- EquiMessage edge part (k_equi_edge_bwd + weight-gradient GEMMs) ----
        if A > 0:
            dn = [e + "dir_proj.0.weight", e + "dir_proj.0.bias", e + "dir_proj.2.weight", e + "dir_proj.2.bias"]
            ew1 = tape.get(_capi.TAPE_EW, l + 1)[:A, :W]
            dcd = rnd(A, 3 * H)
            o32, g32, g64_ = both(lambda Pq, gd, ew_t, dn=dn: F.linear(F.silu(F.linear(ew_t, Pq[dn[0]], Pq[dn[1]])), Pq[dn[2]], Pq[dn[3]]),
                                  [ew1], dn, [dcd])
            note(f"fwd layer {l} equi edge: cd", rel(o32[0].view(A, 3, H), tape.get(_capi.TAPE_CD, l)[:A].view(A, 3, HP)[:, :, :H]))
            dcd_p = torch.zeros(A + 1, 3, HP, device=dev)
            dcd_p[:A, :, :H] = dcd.view(A, 3, H)
            dew2 = torch.zeros(E + 1, WP, device=dev)
            gt = stage(_capi.STAGE_EQUI_EDGE, l, (dcd_p,), (dew2,), dn)
            gate(f"bwd layer {l} equi edge", ["dew"] + [short(n_) for n_ in dn], [dew2[:A, :W]] + [gt[n_] for n_ in dn], g32, g64_)
        # ---- EquiUpdate ----
        un = [n_ for n_ in P if n_.startswith(u)]
        sa0 = tape.get(_capi.TAPE_S_A, l)[:, :H]
        va0 = tape.get(_capi.TAPE_VEC_A, l).view(N, 3, HP)[:, :, :H]
        cs, cv = rnd(N, H), rnd(N, 3, H)
        o32, g32, g64_ = both(lambda Pq, gd, a_, b_, l=l: refs.stage_equi_update(Pq, l, a_, b_, gd, H), [sa0, va0], un, [cs, cv])
        note(f"fwd layer {l} equi update: s, vec", rel(o32[0], tape.get(_capi.TAPE_S_IN, l + 1)[:, :H]),
             rel(o32[1], tape.get(_capi.TAPE_VEC_IN, l + 1).view(N, 3, HP)[:, :, :H]))
        gs_a, gvec_a = torch.empty(N, HP, device=dev), torch.empty(3 * N, HP, device=dev)
        gt = stage(_capi.STAGE_UPDATE, l, (pad(cs), pad3(cv)), (gs_a, gvec_a), un)
        gate(f"bwd layer {l} equi update", ["ds_a", "dvec_a"] + [short(n_) for n_ in un], [unpad(gs_a), unpad3(gvec_a)] + [gt[n_] for n_ in un],
             g32, g64_)
        # ---- EquiMessage gather half ----
        if A > 0:
            cd0 = tape.get(_capi.TAPE_CD, l)[:A].view(A, 3, HP)[:, :, :H]
            vec0 = tape.get(_capi.TAPE_VEC_IN, l).view(N, 3, HP)[:, :, :H]
            rbfn = e + "rbf_proj.weight"
            gS, gVc = rnd(N, H), rnd(N, 3, H)
            s_mid_t = tape.get(_capi.TAPE_S_MID, l)[:, :H]
            o32, g32, g64_ = both(lambda Pq, gd, xq_t, cd_t, vec_t, l=l: refs.stage_equi_message(
                Pq, l, s_mid_t.to(xq_t.dtype), xq_t, cd_t, vec_t, gd, H), [xq_r, cd0, vec0], [rbfn], [gS, gVc])
            note(f"fwd layer {l} equi message: s_a, vec_a", rel(o32[0], tape.get(_capi.TAPE_S_A, l)[:, :H]),
                 rel(o32[1], tape.get(_capi.TAPE_VEC_A, l).view(N, 3, HP)[:, :, :H]))
            gx_o, dxq_o, dvec_o = torch.empty(N, HP, device=dev), torch.empty(N, 3 * HP, device=dev), torch.empty(3 * N, HP, device=dev)
            gt = stage(_capi.STAGE_MESSAGE, l, (pad(gS), pad3(gVc)), (gx_o, dxq_o, dvec_o), [rbfn])
            assert rel(unpad(gx_o), gS * refs.INV_SQRT2) <= 2e-7
            dcd_s = scratch(_capi.SCRATCH_DCD).view(A + 1, 3, HP)
            assert HP == H or float(dcd_s[:A, :, H:].abs().max()) == 0.0          # the MFMA edge kernel reads the pads
            assert float(dcd_s[A].abs().max()) == 0.0                              # ... and the spare row
            gate(f"bwd layer {l} equi message", ["dxq", "dcd", "dvec", "rbf_proj"],
                 [unpad3(dxq_o).reshape(N, 3 * H), dcd_s[:A, :, :H], unpad3(dvec_o), gt[rbfn]], g32, g64_)
        # ---- GCL node update + x_proj ----
        gn = [n_ for n_ in P if n_.startswith((q + "node_mlp.", e + "x_layernorm.", e + "x_proj."))]
        c1, c2 = rnd(N, H), rnd(N, 3, H)
        o32, g32, g64_ = both(lambda Pq, gd, a_, b_, l=l: refs.stage_gcl_node(Pq, l, a_, b_, H), [xh, agg0], gn, [c1, c2.reshape(N, 3 * H)])
        note(f"fwd layer {l} gcl node: s_mid", rel(o32[0], tape.get(_capi.TAPE_S_MID, l)[:, :H]))
        dxh_o, dagg_o = torch.empty(N, HP, device=dev), torch.empty(N, HP, device=dev)
        gt = stage(_capi.STAGE_GCL_NODE, l, (pad(c1), pad3(c2).view(N, 3 * HP)), (dxh_o, dagg_o), gn)
        gate(f"bwd layer {l} gcl node", ["dxh", "dagg"] + [short(n_) for n_ in gn], [unpad(dxh_o), unpad(dagg_o)] + [gt[n_] for n_ in gn], g32, g64_)
        # ---- pos_expansion + LayerNorm + node halves of edge_mlp.0 ----
        pn = [n_ for n_ in P if n_.startswith(("model.pos_expansion.", q + "x_layernorm."))] + [q + "edge_mlp.mlp.0.linear.weight", q + "edge_mlp.mlp.0.linear.bias"]
        c1, c2, c3 = rnd(N, H), rnd(N, H), rnd(N, H)
        o32, g32, g64_ = both(lambda Pq, gd, s_t, l=l: refs.stage_node_pre(Pq, l, s_t, gd, H), [s_in], pn, [c1, c2, c3])
        ds_o = torch.empty(N, HP, device=dev)
        gt = stage(_capi.STAGE_NODE_PRE, l, (pad(c1), pad(c2), pad(c3)), (ds_o,), pn)
        assert float(gt[w1][:, 2 * H:].abs().max()) == 0.0          # the edge columns belong to the GCL_EDGE stage
        cut = lambda n_, t_: t_[:, :2 * H] if n_ == w1 else t_      # noqa: E731
        gate(f"bwd layer {l} node pre", ["ds_in"] + [short(n_) for n_ in pn], [unpad(ds_o)] + [cut(n_, gt[n_]) for n_ in pn],
             [g32[0]] + [cut(n_, t_) for n_, t_ in zip(pn, g32[1:])], [g64_[0]] + [cut(n_, t_) for n_, t_ in zip(pn, g64_[1:])])
    # ---- tail (output block + velocity / CoM + decoders) and init head + encoders ----------------------------------------
    emb = dyn.embed_dim
    dec = [dyn._module_prefix("decoders", k) for k in range(n_obj)]
    enc = [dyn._module_prefix("encoders", k) for k in range(n_obj)]
    tn = [n_ for n_ in P if n_.startswith(("model.out_pos.", "model.embedding_out.", *dec))]
    s_L = tape.get(_capi.TAPE_S_IN, NL)[:, :H]
    v_L = tape.get(_capi.TAPE_VEC_IN, NL).view(N, 3, HP)[:, :, :H]
    cots = [rnd(int(x_.shape[0]), int(x_.shape[1])) for x_ in st.xh]
    o32, g32, g64_ = both(lambda Pq, gd, s_t, v_t: refs.stage_tail(Pq, dec, s_t, v_t, topo.node_group, topo.B * n_obj,
                                                                   topo.group_count.to(s_t.dtype), topo.obj_rows, topo.node_row, emb),
                          [s_L, v_L], tn, cots)
    ds_o, dvec_o = torch.empty(N, HP, device=dev), torch.empty(3 * N, HP, device=dev)
    tab, dd = grad_dests(tn)
    go = (C.c_void_p * n_obj)(*[c_.data_ptr() for c_ in cots])
    _capi.check(L.oard_train_tail_backward(C.byref(cfg), topo.handle, packed_f.data_ptr(), packed_b.data_ptr(), tape.buf.data_ptr(), go,
                                           ds_o.data_ptr(), dvec_o.data_ptr(), params_tab, tab, sc_buf.data_ptr(), sc_buf.numel(), stream), "tail")
    gate("bwd tail", ["ds", "dvec"] + [n_.split(".", 1)[1] for n_ in tn], [unpad(ds_o), unpad3(dvec_o)] + [dd[n_] for n_ in tn], g32, g64_)
    inn = [n_ for n_ in P if n_.startswith(("model.embedding.", "model.neighbor_emb.", "model.s2v.", "model.radial_lin.", "model.lin3.", *enc))]
    feats = [x_[:, 3:] for x_ in st.xh]
    hin_tail = tape.get(_capi.TAPE_HIN)[:, emb:Cc]
    c_s, c_e, c_c = rnd(N, H), rnd(A, W), rnd(max(E - A, 0), W)
    if not all_ok:              # the scalarisation link has its own check above (2a): its sign-noisy items would mask everything else here;
        c_e[:, :2 * H] = 0      # batches without such items (every object >= 4 atoms, not coplanar) run the whole init head incl. S2V

    def init_fn(Pq, gd, *fs):
        hd = refs.stage_head(Pq, enc, list(fs), topo.node_ref, hin_tail.to(fs[0].dtype))
        return (hd,) + tuple(refs.stage_init(Pq, hd, gd, H))
    o32, g32, g64_ = both(init_fn, feats, inn, [torch.zeros(N, Cc, device=dev), c_s, c_e, c_c.sum(0)])
    note("fwd head: hin", rel(o32[0], tape.get(_capi.TAPE_HIN)[:, :Cc]))
    dew_i = torch.zeros(E + 1, WP, device=dev)
    dew_i[:A, :W] = c_e
    dew_i[A:E, :W] = c_c
    tab, dd = grad_dests(inn)
    xhp = (C.c_void_p * n_obj)(*[x_.data_ptr() for x_ in st.xh])
    _capi.check(L.oard_train_init_backward(C.byref(cfg), topo.handle, packed_f.data_ptr(), packed_b.data_ptr(), tape.buf.data_ptr(), xhp,
                                           pad(c_s).data_ptr(), dew_i.data_ptr(), params_tab, tab, sc_buf.data_ptr(), sc_buf.numel(), stream), "init")
    nf = len(feats)
    gate("bwd init" + (" (with the S2V / scalarisation link)" if all_ok else ""), [n_.split(".", 1)[1] for n_ in inn], [dd[n_] for n_ in inn],
         g32[nf:], g64_[nf:])
    # ---- 3. whole step ---------------------------------------------------------------------------------------------------
    loss.backward()
    grads = {n: p.grad for n, p in dyn.named_parameters() if p.grad is not None}
    errs, flat = c.compare(grads)
    return out, errs, flat, c.meta["ref_f32_vs_f64"]


def tape_rows(topo, L, dev, stream):
    out = {}
    for key, which in (("src", _capi.TOPO_ROW_SRC), ("tgt", _capi.TOPO_ROW_TGT)):
        t = torch.empty(max(topo.E, 1), dtype=torch.int32, device=dev)
        _capi.check(L.oard_topology_export(topo.handle, which, t.data_ptr(), t.numel(), stream), "export")
        out[key] = t[: topo.E].long()
    return out

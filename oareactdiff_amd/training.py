"""Backward pass of the denoising call.

`EGNNDynamics.forward` under autograd runs the HIP forward in training mode (`oard_forward_train`: same kernels, plus a
*tape* of per-layer edge state, pre-activations and node state) and returns tensors whose `grad_fn` is
`DynamicsFunction`.  Its backward is the reverse sweep of include/oard.h, entirely on the device and entirely hand-written:

    oard_train_tail_backward    output block, velocity / per-object CoM removal, decoders
    oard_train_layer_backward   for l = L-1 .. 0: EquiUpdate, EquiMessage (gather half + the MFMA edge kernel), the GCL node
                                update + x_proj, the GCLMessage MFMA edge kernel, pos_expansion / LayerNorm / edge_mlp.0 node halves,
                                and every weight-gradient GEMM of the layer
    oard_train_init_backward    init head (embedding, NeighborEmb, radial_lin, S2V, edge scalarisation + lin3) and the encoders

Python only owns the buffers (tape, scratch, cotangents, one flat gradient bucket) and makes L + 2 calls through ctypes: there
is no torch arithmetic in the sweep (round 2 differentiated the O(N) node stages with local torch autograd: ~1 300 launches of
at::native / hipBLASLt kernels per step).

What the reference does instead: plain torch autograd through `LEFTNet.forward` (oa_reactdiff/model/leftnet.py:724-891)
from `DDPMModule.training_step` (oa_reactdiff/trainer/pl_trainer.py:327-347).  Gradients are produced for every
parameter of the state dict except the two modules the forward never touches (`model.distance_embedding`,
`model.last_layer`; the reference leaves their `.grad` None as well) and the RBF buffers.

There is no CPU fallback: the tape only exists on a ROCm device.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _capi
from .flat_state import FlatLayout

UNUSED_PREFIXES = ("model.distance_embedding.", "model.last_layer.")


def _pad16(n: int) -> int:
    return (n + 15) // 16 * 16


# =====================================================================================================================
# The HIP side of one training-mode forward
# =====================================================================================================================
class TrainTopology:
    """parts == 1 topology plus the index tables the stage functions need (internal order, int64 on the device)."""

    def __init__(self, cfg, combined_mask: Tensor, n_frag_switch: Tensor, stream: int, edge_index: Optional[Tensor] = None,
                 device: Optional[torch.device] = None):
        """`combined_mask` / `n_frag_switch` may be HOST tensors (with `device` naming the GPU): a loader that keeps the CPU copies of
        the batch's masks (DDPMTrainer.to_device) saves the step the device -> host copy - a wait for everything queued on the
        stream.  The tables are built on the host, uploaded through a pinned buffer on the library's own stream and pooled
        (oard_hip.hip, table pool): creating and dropping a topology per step does not synchronise the device."""
        L = _capi.lib()
        dev = torch.device(device) if device is not None else combined_mask.device
        if dev.type != "cuda":
            raise _capi.OardError("TrainTopology needs a ROCm device (pass device= with host masks)")
        cm = combined_mask.detach().to("cpu", torch.int64).contiguous()
        nfs = n_frag_switch.detach().to("cpu", torch.int64).contiguous()
        h = C.c_void_p()
        _capi.check(L.oard_topology_create_parts(C.byref(cfg), C.cast(cm.data_ptr(), C.POINTER(C.c_int64)),
                                                 C.cast(nfs.data_ptr(), C.POINTER(C.c_int64)), cm.numel(), 1, C.byref(h)),
                    "oard_topology_create_parts")
        self.handle, self._lib = h, L
        self.key_tensors = None                        # set by the cache that holds this topology (dynamics._TensorKeyCache)
        self.N, self.E = int(L.oard_topology_num_nodes(h)), int(L.oard_topology_num_edges(h))
        self.A, self.B = int(L.oard_topology_num_inner_edges(h)), int(L.oard_topology_num_samples(h))
        self.n_obj = cfg.n_obj
        self.max_sample_id = int(cm.max())
        self.obj_counts = [int((nfs == k).sum()) for k in range(cfg.n_obj)]

        def table(which: int, n: int) -> Tensor:
            t = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            _capi.check(L.oard_topology_export(h, which, t.data_ptr(), t.numel(), stream), "oard_topology_export")
            return t[:n].long()
        self.node_ref = table(_capi.TOPO_NODE_REF, self.N)
        self.node_obj = table(_capi.TOPO_NODE_OBJ, self.N)
        self.node_row = table(_capi.TOPO_NODE_ROW, self.N)
        self.node_sample = table(_capi.TOPO_NODE_SAMPLE, self.N)
        self.inner_src = table(_capi.TOPO_INNER_SRC, self.A)
        self.inner_tgt = table(_capi.TOPO_INNER_TGT, self.A)
        self.node_group = self.node_sample * cfg.n_obj + self.node_obj
        # rows of every object and the size of every (sample, object) group, built once here: a nonzero() in the backward sweep
        # would be a host sync right after the forward pass
        order = torch.argsort(self.node_obj, stable=True)
        starts = [0]
        for k in range(cfg.n_obj):
            starts.append(starts[-1] + self.obj_counts[k])
        self.obj_rows = [order[starts[k]:starts[k + 1]] for k in range(cfg.n_obj)]
        self.group_count = torch.zeros(self.B * cfg.n_obj, 1, device=dev).index_add_(
            0, self.node_group, torch.ones(self.N, 1, device=dev)).clamp(min=1)
        if edge_index is not None:       # the kernels assume the complete-per-sample graph in the reference's edge order: verify
            ei = edge_index.detach()
            if ei.dim() != 2 or ei.shape[0] != 2 or ei.dtype != torch.int64 or ei.device != dev:
                raise _capi.OardError("edge_index must be an int64 [2, E] tensor on the same device")
            ei = ei.contiguous()
            ok = torch.zeros(1, dtype=torch.int32, device=dev)
            _capi.check(L.oard_topology_check_edge_index(h, ei.data_ptr(), ei.shape[1], ok.data_ptr(), stream),
                        "oard_topology_check_edge_index")
            if int(ok.item()) != 1:
                raise _capi.OardError("edge_index is not get_edges_index(combined_mask, remove_self_edge=True): the training path (tape, "
                                      "hand-written backward) is built on the complete graph per sample; general edge lists are served "
                                      "in inference only (csrc/oard_general.h)")

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._lib.oard_topology_destroy(self.handle)
        except Exception:
            pass


class Tape:
    """Views into the tape buffer of one oard_forward_train."""

    def __init__(self, cfg, topo: TrainTopology, buf: Tensor):
        self.cfg, self.topo, self.buf = cfg, topo, buf

    def get(self, which: int, layer: int = 0) -> Tensor:
        off, rows, ld = C.c_size_t(0), C.c_int64(0), C.c_int64(0)
        _capi.check(_capi.lib().oard_tape_entry(C.byref(self.cfg), self.topo.handle, which, layer, C.byref(off), C.byref(rows),
                                                C.byref(ld)), "oard_tape_entry")
        n = rows.value * ld.value
        return self.buf[off.value: off.value + 4 * n].view(torch.float32).view(rows.value, ld.value)


class TrainState:
    """Everything one forward leaves behind for its backward."""

    def __init__(self, cfg, topo: TrainTopology, tape: Tape, xh: List[Tensor], t: Tensor, t_scalar: bool,
                 cond: Optional[Tensor]):
        self.cfg, self.topo, self.tape = cfg, topo, tape
        self.xh, self.t, self.t_scalar, self.cond = xh, t, t_scalar, cond
        self.keep_inputs = self.keepalive = None       # what the asynchronous launches of the step / of the sweep still read


def _wgrad(dY: Tensor, ncY: int, o_len: int, o_pad: int, MO: int, X: Tensor, ncX: int, x_silu: bool, i_len: int,
           i_pad: int, MI: int, rows: int, want_bias: bool, scratch_owner, stream: int) -> Tuple[Tensor, Optional[Tensor]]:
    """dW [MO,MI] (= nn.Linear weight shape) and db [MO] from row-major operands through oard_wgrad."""
    L = _capi.lib()
    need = L.oard_wgrad_scratch_bytes(ncY, ncX, rows)
    sc = getattr(scratch_owner, "_wgrad_scratch", None)
    if sc is None or sc.numel() < need or sc.device != dY.device:
        sc = torch.empty(need, dtype=torch.uint8, device=dY.device)
        scratch_owner._wgrad_scratch = sc
    dW = torch.empty(MO, MI, dtype=torch.float32, device=dY.device)
    db = torch.empty(MO, dtype=torch.float32, device=dY.device) if want_bias else None
    _capi.check(L.oard_wgrad(dY.data_ptr(), dY.stride(0), ncY, o_len, o_pad, MO, X.data_ptr(), X.stride(0), ncX,
                             1 if x_silu else 0, i_len, i_pad, MI, rows, dW.data_ptr(),
                             db.data_ptr() if db is not None else None, sc.data_ptr(), sc.numel(), stream), "oard_wgrad")
    return dW, db


def scalarize_backward(dyn, cfg, topo: TrainTopology, tape: Tape, NE1: Tensor, dew: Tensor, H: int, stream: int):
    """oard_scalarize_backward: adjoint of k_scalarize.  NE1 [N,3,H] contiguous, dew [E+1,WP] (gradient of the initial
    edge state, columns [0, 2H) of the inner rows are read) -> (d NE1 [N,3,H], {lin3 parameter name: gradient})."""
    L = _capi.lib()
    H4 = H // 4
    dNE1 = torch.empty_like(NE1)
    part = torch.empty(topo.N, 5 * H4 + 1, dtype=torch.float32, device=NE1.device)
    packed = dyn._get_packed(cfg, stream)
    _capi.check(L.oard_scalarize_backward(C.byref(cfg), topo.handle, packed.data_ptr(), tape.buf.data_ptr(), NE1.data_ptr(), H,
                                          dew.data_ptr(), dNE1.data_ptr(), part.data_ptr(), stream), "oard_scalarize_backward")
    tot = part.sum(dim=0)
    m = "model."
    return dNE1, {m + "lin3.0.weight": tot[: 3 * H4].view(H4, 3), m + "lin3.0.bias": tot[3 * H4: 4 * H4],
                  m + "lin3.2.weight": tot[4 * H4: 5 * H4].view(1, H4), m + "lin3.2.bias": tot[5 * H4:]}


class _StageTimer:
    """OARD_TRAIN_PROFILE=1: device time of the three parts of the sweep (HIP events on the current stream), printed per call."""

    def __init__(self):
        import os
        self.on = bool(os.environ.get("OARD_TRAIN_PROFILE"))
        self.marks = []

    def mark(self, name: str):
        if self.on:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append((name, e))

    def report(self):
        if not self.on or len(self.marks) < 2:
            return
        torch.cuda.synchronize()
        tot: Dict[str, float] = {}
        for (n0, e0), (n1, e1) in zip(self.marks[:-1], self.marks[1:]):
            tot[n1] = tot.get(n1, 0.0) + e0.elapsed_time(e1)
        print("backward sweep ms: " + "  ".join(f"{k} {v:.2f}" for k, v in tot.items()) + f"  | total {sum(tot.values()):.2f}")


def fresh_gradients(params: Dict[str, Tensor], dev) -> Tuple[Dict[str, Tensor], Dict[int, Tensor]]:
    """Gradient destinations of a sweep whose caller keeps none: one fresh zero-filled flat float32 buffer laid out like `params`
    (name -> tensor) -> ({name: view}, {id(tensor): view})."""
    layout = FlatLayout(list(params.values()))
    views = layout.views(torch.zeros(layout.size, dtype=torch.float32, device=dev))
    return dict(zip(params, views)), {id(p): v for p, v in zip(layout.tensors, views)}


def inplace_gradients(params: Dict[str, Tensor]) -> Dict[int, Tensor]:
    """`grad_inplace`: the `.grad` tensors of `params` (name -> tensor) as gradient destinations {id(tensor): .grad}; a missing one is
    created zero-filled, and each has to be contiguous float32 for the kernels to accumulate into."""
    for n, p in params.items():
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        if p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
            raise _capi.OardError(f"grad_inplace needs contiguous float32 .grad tensors ({n})")
    return {id(p): p.grad for p in params.values()}


def gradient_table(dyn, dests: Dict[int, Tensor]):
    """(void* array in the canonical parameter order of oard_pack_weights) for the gradient destinations: `dests` maps id(param) ->
    contiguous float32 tensor of the parameter's shape; parameters without an entry, buffers and the two modules the forward
    never uses get NULL (the sweep skips them)."""
    return _capi.ptr_array([dests.get(id(t)) if isinstance(t, nn.Parameter) and not name.startswith(UNUSED_PREFIXES) else None
                            for name, t in zip(dyn._spec, dyn._ordered_tensors())])


class Sweep:
    """The reverse sweep of one training-mode forward as L + 2 separately issued steps (`tail`, `layer(l)` for l = L-1 .. 0, `init`), all
    asynchronous on `stream`.  `backward_sweep` issues them back to back; DDPMTrainer's two-micro-batch step interleaves the steps of two
    sweeps that run on two streams, so that the library's gradient stream sees their weight-gradient work alternately (one sweep issued
    as a whole would park the other's weight gradients - and with them its cotangent chain, which waits for the scratch buffers they
    read - behind all of its own).
    `dests` (id(param) -> tensor): accumulate INTO these tensors (e.g. the `.grad` views of a flat bucket); None: accumulate into a fresh
    zero-filled flat buffer, `self.out` = {canonical name: view}.  `buffers`: the per-call buffer set whose scratch the sweep uses - the one
    its forward ran on (None: the module's own).
    `conf_tail` = (readout tensors [12], dconf [B], readout gradient destinations [12], None entries skipped): the sweep of a
    `Confidence` forward (oard_confidence_forward_train) - `tail` is then oard_confidence_tail_backward, the adjoint of the pooled gated
    readout, `grad_outs` is not used and `dests` is required (the caller knows which trunk tensors the confidence forward uses)."""

    def __init__(self, dyn, st: TrainState, grad_outs: List[Optional[Tensor]], stream: int, dests: Optional[Dict[int, Tensor]] = None,
                 buffers=None, conf_tail=None):
        L = _capi.lib()
        self.L, self.st, self.stream = L, st, stream
        cfg, topo, tape = st.cfg, st.topo, st.tape
        H, R, NL, Cc = dyn._dims
        HP, WP = _pad16(H), _pad16(3 * H + R)
        N, E = topo.N, topo.E
        dev = st.xh[0].device
        n_obj = len(dyn.node_nfs)
        packed, pbwd = dyn._get_packed(cfg, stream), dyn._get_packed_bwd(cfg, stream)
        sc = (dyn._call_buffers if buffers is None else buffers).scratch(L.oard_train_scratch_bytes(C.byref(cfg), topo.handle), dev)
        self.out: Dict[str, Tensor] = {}
        self.conf_tail = conf_tail
        if conf_tail is not None and dests is None:
            raise ValueError("a confidence sweep needs its gradient destinations")
        if dests is None:
            P = dyn._param_dict()
            used = [n for n in dyn._param_names() if not n.startswith(UNUSED_PREFIXES)]
            self.out, dests = fresh_gradients({n: P[n] for n in used}, dev)
        tensors = dyn._ordered_tensors()
        self.params = _capi.ptr_array(tensors)
        self.grads = gradient_table(dyn, dests)
        gos = []
        for k in range(n_obj):
            g = grad_outs[k] if k < len(grad_outs) else None
            gos.append(None if g is None else g.to(torch.float32).contiguous())
        self.go, self.xhp = _capi.ptr_array(gos), _capi.ptr_array(st.xh)
        ds = torch.empty(N, HP, device=dev)
        dvec = torch.empty(3 * N, HP, device=dev)
        # cotangent of the edge state, updated in place layer by layer.  Nothing flows into the FINAL edge state: the last layer's kernels
        # read the inner rows [0, A) as that zero gradient (and the spare row E for their padding columns) and never read the inter-object
        # rows (their S3 was skipped in the forward), so only those rows are cleared - 0.27 GB instead of 0.83 GB at B = 64
        dew = torch.empty(E + 1, WP, device=dev)
        dew[: topo.A].zero_()
        dew[E:].zero_()
        self.ds, self.dvec, self.dew, self.sc, self.NL = ds, dvec, dew, sc, NL
        self.a = (C.byref(cfg), topo.handle, packed.data_ptr(), pbwd.data_ptr(), tape.buf.data_ptr())
        self._keep = (cfg, packed, pbwd, tensors, dests, gos)       # the launches are asynchronous
        st.keepalive = (gos, ds, dvec, dew)

    def tail(self):
        if self.conf_tail is not None:
            readout, dconf, rgrads = self.conf_tail
            _capi.check(self.L.oard_confidence_tail_backward(self.a[0], self.a[1], self.a[4], _capi.ptr_array(readout), dconf.data_ptr(),
                                                             self.ds.data_ptr(), self.dvec.data_ptr(), _capi.ptr_array(rgrads),
                                                             self.sc.data_ptr(), self.sc.numel(), self.stream),
                        "oard_confidence_tail_backward")
            return
        _capi.check(self.L.oard_train_tail_backward(*self.a, self.go, self.ds.data_ptr(), self.dvec.data_ptr(), self.params, self.grads,
                                                    self.sc.data_ptr(), self.sc.numel(), self.stream), "oard_train_tail_backward")

    def layer(self, l: int):
        _capi.check(self.L.oard_train_layer_backward(*self.a, l, self.ds.data_ptr(), self.dvec.data_ptr(), self.dew.data_ptr(), self.params,
                                                     self.grads, self.sc.data_ptr(), self.sc.numel(), self.stream),
                    "oard_train_layer_backward")

    def init(self):
        _capi.check(self.L.oard_train_init_backward(*self.a, self.xhp, self.ds.data_ptr(), self.dew.data_ptr(), self.params, self.grads,
                                                    self.sc.data_ptr(), self.sc.numel(), self.stream), "oard_train_init_backward")


def backward_sweep(dyn, st: TrainState, grad_outs: List[Optional[Tensor]], stream: int,
                   dests: Optional[Dict[int, Tensor]] = None, buffers=None, conf_tail=None) -> Dict[str, Tensor]:
    """d(loss)/d(parameter) for every parameter the forward uses, given d(loss)/d(out[k]).
    `dests` (id(param) -> tensor): accumulate INTO these tensors (e.g. the `.grad` views of a flat bucket) and return {};
    None: accumulate into a fresh zero-filled flat buffer and return {canonical name: view}.  `buffers`, `conf_tail`: as for `Sweep`."""
    tm = _StageTimer()
    tm.mark("start")
    sw = Sweep(dyn, st, grad_outs, stream, dests, buffers, conf_tail)
    sw.tail()
    tm.mark("tail")
    for l in reversed(range(sw.NL)):
        sw.layer(l)
        tm.mark("layers")
    sw.init()
    tm.mark("init")
    tm.report()
    return sw.out


class DynamicsFunction(torch.autograd.Function):
    """outs = EGNNDynamics(xh, ...) with a HIP forward (training mode) and the sweep above as backward.
    Inputs after the fixed arguments: the xh tensors, then every parameter (so autograd routes their gradients).

    `dyn.grad_inplace` (set by DDPMTrainer): the sweep accumulates straight into the parameters' existing `.grad` tensors (views
    of the trainer's flat bucket) and autograd receives None for them - no per-parameter AccumulateGrad launch.  Otherwise the
    gradients are returned to autograd as views of one flat buffer."""

    @staticmethod
    def forward(ctx, dyn, run_forward, n_obj, *tensors):
        outs, state = run_forward()
        ctx.dyn, ctx.state, ctx.n_obj = dyn, state, n_obj
        ctx.names = dyn._param_names()
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grad_outs):
        dyn, st = ctx.dyn, ctx.state
        dev = st.xh[0].device
        P = dyn._param_dict()
        dests = None
        if dyn.grad_inplace:
            dests = inplace_gradients({n: P[n] for n in ctx.names if not n.startswith(UNUSED_PREFIXES)})
        with torch.cuda.device(dev), torch.no_grad():
            stream = torch.cuda.current_stream(dev).cuda_stream
            grads = backward_sweep(dyn, st, list(grad_outs), stream, dests)
        ctx.state = None
        out: List[Optional[Tensor]] = [None, None, None] + [None] * ctx.n_obj       # no gradient w.r.t. the noised inputs
        for n in ctx.names:
            out.append(grads.get(n))
        return tuple(out)

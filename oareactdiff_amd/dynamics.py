"""`EGNNDynamics` — drop-in for `oa_reactdiff.dynamics.EGNNDynamics(model=LEFTNet)` whose forward
pass runs on liboard_hip.so (hand-written gfx950 kernels) through the C ABI in include/oard.h.

Mirrors the reference interface (oa_reactdiff/dynamics/egnn_dynamics.py:14-168,
oa_reactdiff/dynamics/_base.py:10-132): same constructor arguments, same `forward` signature and
return convention `(List[Tensor], None)`, same attributes (`encoders`, `decoders`, `model`,
`pos_dim`, `node_nfs`, `fragment_names`, ...) and the same state-dict names and shapes, so a
checkpoint's `ddpm.dynamics.*` tensors load with `load_state_dict(strict=True)`.

There is no CPU / eager fallback: `forward` needs tensors on a ROCm device and the built library.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _capi
from .spec import model_dims, rbf_buffers, state_spec


class _Node(nn.Module):
    """Anonymous container used to reproduce the reference's module tree (names only)."""


def _xavier_names(name: str) -> bool:
    # layers the reference re-initialises with xavier_uniform_ (leftnet.py:235-242, 318-323, 558-564)
    keys = ("x_proj.0.weight", "x_proj.2.weight", "rbf_proj.weight", "vec_proj.weight", "xvec_proj.0.weight",
            "xvec_proj.2.weight", "vec1_proj.weight", "vec2_proj.weight", "update_net.0.weight", "update_net.2.weight")
    return name.endswith(keys)


class _CallBuffers:
    """What one network call scribbles on: the workspace, the grow-only tape of the fused trainer, the scratch of the backward sweep and
    the sticky NaN flag.  A module owns one set (`EGNNDynamics._call_buffers`); whoever runs a second call beside the module's own -
    DDPMTrainer's second micro-batch - owns a second set and hands it to `_run_forward_train` / `training.Sweep`.  Every buffer is
    reallocated when it is too small or sits on another device, and never shrinks."""
    __slots__ = ("ws", "tape_buf", "scratch_buf", "nan_seen")

    def __init__(self) -> None:
        self.ws = self.tape_buf = self.scratch_buf = self.nan_seen = None

    @staticmethod
    def _fits(buf: Optional[Tensor], need: int, dev) -> bool:
        return buf is not None and buf.numel() >= need and buf.device == dev

    def workspace(self, need: int, dev) -> Tensor:
        if not self._fits(self.ws, need, dev):
            self.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self.ws

    def tape(self, nbytes: int, dev) -> Tensor:
        """`nbytes` of ONE grow-only buffer (1/8 headroom): batch layouts of changing size would otherwise have the allocator carve
        multi-GB blocks of ever new sizes."""
        if not self._fits(self.tape_buf, nbytes, dev):
            self.tape_buf = None                                          # released before its successor is carved
            self.tape_buf = torch.empty(nbytes + nbytes // 8, dtype=torch.uint8, device=dev)
        return self.tape_buf[:nbytes]

    def scratch(self, need: int, dev) -> Tensor:
        if not self._fits(self.scratch_buf, need, dev):
            self.scratch_buf = torch.empty(need, dtype=torch.uint8, device=dev)
        return self.scratch_buf

    def note(self, status: Tensor) -> None:
        """OR a call's device-side status into the sticky flag (no host sync)."""
        if self.nan_seen is None or self.nan_seen.device != status.device:
            self.nan_seen = torch.zeros(2, dtype=torch.int32, device=status.device)
        self.nan_seen.bitwise_or_(status)

    def reset(self) -> None:
        if self.nan_seen is not None:
            self.nan_seen.zero_()


class _TensorKeyCache(OrderedDict):
    """LRU of at most `cap` objects keyed by the address, version and shape of the tensors they were built from.  An entry keeps those
    tensors alive (`key_tensors`), so that the caching allocator cannot hand their storage to a different layout of the same size while
    the entry exists."""

    def __init__(self, cap: int = 8) -> None:
        super().__init__()
        self.cap = cap

    def lookup(self, tensors: Tuple[Optional[Tensor], ...], extra: tuple, build):
        key = tuple((0, 0, ()) if t is None else (t.data_ptr(), t._version, t.shape) for t in tensors) + extra
        hit = self.get(key)
        if hit is not None:
            self.move_to_end(key)
            return hit
        hit = build()
        hit.key_tensors = tensors
        self[key] = hit
        while len(self) > self.cap:
            self.popitem(last=False)
        return hit


class EGNNDynamics(nn.Module):
    #: model_config["for_conf"] this class runs: the denoiser's output head here, the pooled readout in `confidence.Confidence`
    _for_conf = False

    def __init__(
        self,
        model_config: Dict,
        fragment_names: List[str],
        node_nfs: List[int],
        edge_nf: int,
        condition_nf: int = 0,
        pos_dim: int = 3,
        update_pocket_coords: bool = True,
        condition_time: bool = True,
        edge_cutoff: Optional[float] = None,
        model=None,
        device: torch.device = torch.device("cuda"),
        enforce_same_encoding: Optional[List] = None,
        source: Optional[Dict] = None,
    ) -> None:
        super().__init__()
        assert len(node_nfs) == len(fragment_names)                       # _base.py:44-46
        for nf in node_nfs:
            assert nf > pos_dim
        if "act_fn" not in model_config:                                  # _base.py:47-50 (mutates the dict)
            model_config["act_fn"] = "swish"
        if "in_node_nf" not in model_config:
            model_config["in_node_nf"] = model_config["in_hidden_channels"]
        if model is not None and getattr(model, "__name__", "LEFTNet") != "LEFTNet":
            raise NotImplementedError("the MI355X backend implements the LEFTNet denoiser only")
        if model_config["act_fn"] not in ("swish", "silu"):
            raise NotImplementedError("only the swish/silu activation is implemented")
        for key, want in (("legacy", True), ("update", True), ("pos_grad", False), ("single_layer_output", True),
                          ("object_aware", True), ("for_conf", self._for_conf), ("ff", False)):       # reflect_equiv: both settings
            if model_config.get(key, want) != want:
                raise NotImplementedError(f"model_config[{key!r}] must be {want} for the MI355X backend")
        if "in_edge_nf" in model_config:
            raise NotImplementedError("edge attributes are not part of the LEFTNet denoising path")
        model_config.setdefault("in_hidden_channels", 8)
        #: what builds a second module of this configuration (DDPMTrainer.ema_dynamics): no `source`, no device - its tensors are the caller's
        self._ctor_args = dict(model_config=dict(model_config), fragment_names=list(fragment_names), node_nfs=list(node_nfs), edge_nf=edge_nf,
                               condition_nf=condition_nf, pos_dim=pos_dim, update_pocket_coords=update_pocket_coords,
                               condition_time=condition_time, edge_cutoff=edge_cutoff, model=model,
                               enforce_same_encoding=None if enforce_same_encoding is None else list(enforce_same_encoding))
        self.model_config = model_config
        self.node_nfs = node_nfs
        self.edge_nf = edge_nf
        self.condition_nf = condition_nf
        self.fragment_names = fragment_names
        self.pos_dim = pos_dim
        self.update_pocket_coords = update_pocket_coords
        self.condition_time = condition_time
        self.edge_cutoff = edge_cutoff
        self.device = device
        self.dist_dim = 0
        self.embed_dim = model_config["in_node_nf"]                       # _base.py:69-77
        self.edge_embed_dim = 0
        if condition_time:
            self.embed_dim -= 1
        if condition_nf > 0:
            self.embed_dim -= condition_nf
        assert self.embed_dim > 0
        self.edge_encoder, self.edge_decoder = None, None

        H, R, L, Cc = model_dims(model_config)
        self._dims = (H, R, L, Cc)
        self._spec = state_spec(model_config, node_nfs, condition_nf, pos_dim, condition_time)
        self.model = _Node()
        self.encoders = nn.ModuleList([_Node() for _ in node_nfs])
        self.decoders = nn.ModuleList([_Node() for _ in node_nfs])
        self._create_tensors(self._spec, device)
        if enforce_same_encoding is not None:                             # _base.py:110-113
            for ii in enforce_same_encoding:
                self.encoders[ii] = self.encoders[0]
                self.decoders[ii] = self.decoders[0]
        if source is not None:                                            # _base.py:65-66, 114-116
            self.model.load_state_dict(source["model"])
            self.encoders.load_state_dict(source["encoders"])
            self.decoders.load_state_dict(source["decoders"])

        #: "sync": reference behaviour (egnn_dynamics.py:138-143) — one host sync per call, NaN -> randn.
        #: "replace": the same replacement WITHOUT a host sync (oard_nan_replace reads the flag on the device; one randn draw per
        #: object and call whether or not it is used), flag kept like "async".
        #: "async": no host sync; the device-side flag of the last call is kept in `self.last_status` and OR-ed into
        #: the sticky flag `self.nan_seen` (reset it with `reset_nan_seen()`; the sampling loops read it once at the end).
        self.nan_check = "sync"
        #: Arithmetic of the two MFMA edge stages in INFERENCE calls.  "f32": the fp32 kernels.  "bf16x3": the split-precision
        #: kernels (csrc/oard_edge_b3.h: three bf16 terms per fp32 value, six bf16 MFMAs per K block, fp32 accumulation - fp32-grade
        #: results, ~1.3 x the step rate at B = 64).  None: the process default `default_edge_precision()` (fp32 unless the environment
        #: says OARD_GCL_B3=1 / OARD_EQUI_B3=1 - read per call, so that the answer never depends on what another module did).
        #: The choice travels with every library call (`oard_config.precision`) and is part of the packed-weights key: modules
        #: with different settings can run side by side, also from different threads / streams.
        self.edge_precision: Optional[str] = None
        #: The same choice for the TRAINING-mode forward (tape written; the backward kernels and weight-gradient GEMMs stay fp32).
        #: None: fp32 unless OARD_TRAIN_B3=1.
        self.train_edge_precision: Optional[str] = None
        self.last_status: Optional[Tensor] = None
        self._call_buffers = _CallBuffers()           # `_ws` and `nan_seen` below are views onto it
        self._packs: Dict[bool, list] = {}            # backward? -> [key, packed weights]
        self._slots = None                            # (module tree, (owning module, attribute) per tensor): _ordered_tensors
        self._topo_cache = _TensorKeyCache(8)
        self._train_topo_cache = _TensorKeyCache(4)
        self.grad_inplace = False                     # DDPMTrainer: the sweep accumulates into the parameters' .grad (training.DynamicsFunction)
        self._last_topo: Optional["_Topology"] = None
        #: "auto": the complete graph per sample runs the production kernels, any other edge list the general path (csrc/oard_general.h);
        #: "general": every inference call runs the general path (tests: two independent implementations of the same network)
        self.edge_list_path = "auto"
        self._warned_unbuilt = False

    def _create_tensors(self, spec, device) -> None:
        """Registers the parameters and buffers `spec` names, under the reference's module tree, with the reference's initial values."""
        means, betas = rbf_buffers(self._dims[1], float(self.model_config.get("cutoff", 10.0)))
        for name, (shape, kind, fan_in) in spec.items():
            parts = name.split(".")
            mod: nn.Module = self
            for p in parts[:-1]:
                if p.isdigit() and isinstance(mod, nn.ModuleList):
                    mod = mod[int(p)]
                else:
                    if not hasattr(mod, p):
                        mod.add_module(p, _Node())
                    mod = getattr(mod, p)
            leaf = parts[-1]
            if kind == "buf_means":
                mod.register_buffer(leaf, means.clone().to(device))
            elif kind == "buf_betas":
                mod.register_buffer(leaf, betas.clone().to(device))
            else:
                t = torch.empty(shape, dtype=torch.float32, device=device)
                if kind == "ln_w":
                    nn.init.ones_(t)
                elif kind == "ln_b":
                    nn.init.zeros_(t)
                elif kind == "w" and _xavier_names(name):
                    nn.init.xavier_uniform_(t)
                elif kind == "b" and ".update_net." in name:
                    nn.init.zeros_(t)
                else:
                    bound = 1.0 / math.sqrt(fan_in)                      # nn.Linear default scale
                    nn.init.uniform_(t, -bound, bound)
                mod.register_parameter(leaf, nn.Parameter(t))

    @property
    def _ws(self) -> Optional[Tensor]:
        return self._call_buffers.ws

    @_ws.setter
    def _ws(self, t: Optional[Tensor]) -> None:
        self._call_buffers.ws = t

    @property
    def nan_seen(self) -> Optional[Tensor]:
        return self._call_buffers.nan_seen

    @nan_seen.setter
    def nan_seen(self, t: Optional[Tensor]) -> None:
        self._call_buffers.nan_seen = t

    def reset_nan_seen(self) -> None:
        self._call_buffers.reset()

    # ------------------------------------------------------------------------------------------
    def _config(self) -> _capi.OardConfig:
        H, R, L, Cc = self._dims
        cfg = _capi.OardConfig()
        cfg.hidden, cfg.num_radial, cfg.num_layers, cfg.in_hidden = H, R, L, Cc
        if len(self.node_nfs) > _capi.OARD_MAX_OBJECTS:
            raise _capi.OardError(f"{len(self.node_nfs)} objects per reaction: the library takes at most {_capi.OARD_MAX_OBJECTS} (OARD_MAX_OBJECTS)")
        cfg.n_obj = len(self.node_nfs)
        for k, nf in enumerate(self.node_nfs):
            cfg.node_nf[k] = nf
            cfg.enc_alias[k] = k      # aliasing is resolved through the parameter pointers we pass
        cfg.condition_nf = self.condition_nf
        cfg.condition_time = 1 if self.condition_time else 0
        cfg.pos_dim = self.pos_dim
        cfg.cutoff = float(self.model_config.get("cutoff", 10.0))
        cfg.reflect_equiv = 1 if self.model_config.get("reflect_equiv", True) else 0       # leftnet.py:268-272, 331, 794-796
        cfg.precision = self._precision_bits()
        return cfg

    def _precision_bits(self) -> int:
        """`oard_config.precision` (OARD_PREC_* of include/oard.h) from `edge_precision` / `train_edge_precision`; None resolves to the
        environment's default at THIS call - never to state left behind by another module."""
        for v in (self.edge_precision, self.train_edge_precision):
            if v not in (None, "f32", "bf16x3"):
                raise ValueError("edge_precision / train_edge_precision must be None, 'f32' or 'bf16x3'")
        env = lambda n: os.environ.get(n, "0") not in ("", "0")
        bits = 0
        if self.edge_precision == "bf16x3" or (self.edge_precision is None and env("OARD_GCL_B3")):
            bits |= _capi.PREC_GCL_BF16X3
        if self.edge_precision == "bf16x3" or (self.edge_precision is None and env("OARD_EQUI_B3")):
            bits |= _capi.PREC_EQUI_BF16X3
        if self.train_edge_precision == "bf16x3" or (self.train_edge_precision is None and env("OARD_TRAIN_B3")):
            bits |= _capi.PREC_TRAIN_BF16X3
        return bits

    def _ordered_tensors(self) -> List[Tensor]:
        """Tensors in the canonical order of include/oard.h (== state_spec order); encoder/decoder
        slots follow whatever module currently sits in `self.encoders[k]` / `self.decoders[k]`.
        The (owning module, attribute) pairs are resolved once per module tree (the walk is ~1 500 `nn.Module.__getattr__` calls,
        1.5 - 4 ms, and a training step asks five times); the tensors themselves are looked up afresh every call, so parameters that
        were re-assigned or re-loaded are seen."""
        tree = tuple(id(m) for m in self.modules())
        slots = self._slots
        if slots is None or slots[0] != tree:
            pairs = []
            for name in self._spec:
                parts = name.split(".")
                mod: nn.Module = self
                for p in parts[:-1]:
                    mod = mod[int(p)] if (p.isdigit() and isinstance(mod, nn.ModuleList)) else getattr(mod, p)
                pairs.append((mod, parts[-1]))
            slots = self._slots = (tree, pairs)
        out: List[Tensor] = []
        for mod, attr in slots[1]:
            t = mod._parameters.get(attr)
            if t is None:
                t = mod._buffers.get(attr)
            out.append(t if t is not None else getattr(mod, attr))
        return out

    def _pack(self, bwd: bool, cfg: _capi.OardConfig, stream: int) -> Tensor:
        """The packed weight stream of the forward kernels, or (`bwd`) the transposed one of the backward edge kernels: repacked when a
        parameter's address or version changes, the forward one also with `cfg.precision`."""
        tensors = self._ordered_tensors()
        key = tuple((t.data_ptr(), t._version) for t in tensors) + (() if bwd else (cfg.precision,))
        slot = self._packs.get(bwd)
        if slot is not None and slot[0] == key:
            return slot[1]
        L = _capi.lib()
        dev = tensors[0].device
        for t in tensors:
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise _capi.OardError("parameters must be contiguous float32 tensors on one ROCm device")
        n = L.oard_param_count(C.byref(cfg))
        if n != len(tensors):
            raise _capi.OardError(f"parameter count mismatch: library expects {n}, module has {len(tensors)}")
        size, pack, what = ((L.oard_packed_bwd_bytes, L.oard_pack_weights_bwd, "oard_pack_weights_bwd") if bwd else
                            (L.oard_packed_bytes, L.oard_pack_weights, "oard_pack_weights"))
        nbytes = size(C.byref(cfg))
        packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _capi.check(pack(C.byref(cfg), _capi.ptr_array(tensors), n, packed.data_ptr(), nbytes, stream), what)
        self._packs[bwd] = [key, packed]
        return packed

    def _get_packed(self, cfg: _capi.OardConfig, stream: int) -> Tensor:
        return self._pack(False, cfg, stream)

    def _get_packed_bwd(self, cfg: _capi.OardConfig, stream: int) -> Tensor:
        """Transposed weight streams of the backward edge kernels (repacked when a parameter changes)."""
        return self._pack(True, cfg, stream)

    def invalidate_packed(self) -> None:
        """The weights changed behind torch's version counters (the fused optimiser kernel): the next call repacks them.  The blobs
        themselves stay alive until then."""
        for slot in self._packs.values():
            slot[0] = None

    def _param_names(self) -> List[str]:
        """Canonical (first) state-dict name of every distinct trainable parameter, in state-dict order."""
        seen, names = set(), []
        for name, t in zip(self._spec, self._ordered_tensors()):
            if isinstance(t, nn.Parameter) and id(t) not in seen:
                seen.add(id(t))
                names.append(name)
        return names

    def _param_dict(self) -> Dict[str, Tensor]:
        canon = set(self._param_names())
        return {name: t for name, t in zip(self._spec, self._ordered_tensors()) if name in canon}

    def _module_prefix(self, kind: str, k: int) -> str:
        """Canonical state-dict prefix of the module sitting at encoders[k] / decoders[k] (enforce_same_encoding aliases)."""
        mods = getattr(self, kind)
        for j in range(len(mods)):
            if mods[j] is mods[k]:
                return f"{kind}.{j}."
        return f"{kind}.{k}."

    @staticmethod
    def _c0row(P: Dict[str, Tensor], H: int, R: int) -> Tensor:
        """State of a masked (inter-object) edge: [lin3(0) x 2H | radial_lin(0) | 0 x R]  (leftnet.py:768-809 with dist = 0)."""
        m = "model."
        c0f = torch.nn.functional.linear(torch.nn.functional.silu(P[m + "radial_lin.0.bias"]), P[m + "radial_lin.2.weight"],
                                         P[m + "radial_lin.2.bias"])
        c0s = (torch.nn.functional.silu(P[m + "lin3.0.bias"]) @ P[m + "lin3.2.weight"].t() + P[m + "lin3.2.bias"]).reshape(())
        return torch.cat([c0s.expand(2 * H), c0f, torch.zeros(R, dtype=c0f.dtype, device=c0f.device)])

    def _get_topology(self, cfg, edge_index: Tensor, n_frag_switch: Tensor, combined_mask: Tensor,
                      stream: int, force_general: bool = False) -> "_Topology":
        force_general = force_general or self.edge_list_path == "general"
        return self._topo_cache.lookup((edge_index, n_frag_switch, combined_mask), (force_general,), lambda: _Topology(
            cfg, edge_index, n_frag_switch, combined_mask, stream, force_general=force_general))

    def _inputs(self, topo, xh: List[Tensor], t: Tensor, conditions: Tensor, dev, detach: bool = False):
        """The call's operands as the library takes them -> (xs, tt, t_scalar, cond): contiguous float32 rows per object (`detach`: cut
        from the caller's autograd graph, the training path), the time argument, the conditions."""
        xs = []
        for k in range(len(self.node_nfs)):
            x = xh[k].detach() if detach else xh[k]
            if x.dtype != torch.float32 or not x.is_contiguous():
                x = x.contiguous().float()
            if x.shape != (topo.obj_counts[k], self.node_nfs[k]):
                raise _capi.OardError(f"xh[{k}] has shape {tuple(x.shape)}, expected "
                                      f"{(topo.obj_counts[k], self.node_nfs[k])}")
            xs.append(x)
        tt, t_scalar = self._time_argument(t, dev, topo.max_sample_id)
        cond = None
        if self.condition_nf > 0:
            cond = conditions.detach().to(device=dev, dtype=torch.float32).contiguous()
            if cond.shape[0] <= topo.max_sample_id or cond.shape[1] != self.condition_nf:
                raise _capi.OardError("conditions has the wrong shape")
        return xs, tt, t_scalar, cond

    # ------------------------------------------------------------------------------------------
    def forward(
        self,
        xh: List[Tensor],
        edge_index: Tensor,
        t: Tensor,
        conditions: Tensor,
        n_frag_switch: Tensor,
        combined_mask: Tensor,
        edge_attr: Optional[Tensor] = None,
    ) -> Tuple[List[Tensor], Optional[Tensor]]:
        if not self.update_pocket_coords:
            raise NotImplementedError                                     # egnn_dynamics.py:125
        if edge_attr is not None:
            raise NotImplementedError("edge attributes are not part of the LEFTNet denoising path")
        train = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        dev = xh[0].device
        if dev.type != "cuda":
            raise _capi.OardError("EGNNDynamics.forward needs tensors on a ROCm device (no CPU fallback)")
        L = _capi.lib()
        cfg = self._config()
        # the production kernels are compiled per (hidden_channels, num_radial) pair (OARD_DIMS, oareactdiff_amd.build).  Any other pair
        # still runs - inference only - on the general-edge-list kernels, whose widths are run-time values (csrc/oard_general.h)
        built = L.oard_supported(C.byref(cfg)) == _capi.OARD_OK
        if not built:
            if train:
                _capi.check(L.oard_supported(C.byref(cfg)), "oard_supported (hidden_channels/num_radial not built: the backward pass exists for "
                                                            "built widths only - rebuild: OARD_DIMS=\"196x96,HxR\" python -m oareactdiff_amd.build)")
            if not self._warned_unbuilt:
                import warnings
                self._warned_unbuilt = True
                warnings.warn(f"hidden_channels={int(cfg.hidden)}, num_radial={int(cfg.num_radial)} is not a width pair the production kernels were built "
                              "for: this module's inference calls run the general-edge-list kernels (float64 accumulation, several times slower). "
                              f"For the production kernels rebuild: OARD_DIMS=\"196x96,{int(cfg.hidden)}x{int(cfg.num_radial)}\" python -m oareactdiff_amd.build")
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            packed = self._get_packed(cfg, stream) if built else None
            if train:
                return self._forward_train(cfg, packed, xh, edge_index, t, conditions, n_frag_switch, combined_mask, stream)
            topo = self._get_topology(cfg, edge_index, n_frag_switch, combined_mask, stream, force_general=not built)
            n_obj = len(self.node_nfs)
            xs, tt, t_scalar, cond = self._inputs(topo, xh, t, conditions, dev)
            outs = [torch.empty_like(x) for x in xs]
            general = topo.graph is not None
            need = L.oard_graph_workspace_bytes(C.byref(cfg), topo.graph) if general else L.oard_workspace_bytes(C.byref(cfg), topo.handle)
            buffers = self._call_buffers
            ws = buffers.workspace(need, dev)
            status = torch.zeros(2, dtype=torch.int32, device=dev)
            xp, op = _capi.ptr_array(xs), _capi.ptr_array(outs)
            if general:
                if self.nan_check == "replace":
                    raise _capi.OardError("nan_check='replace' is implemented for the complete-graph topology only")
                tensors = self._ordered_tensors()                 # the general path reads the raw parameters (no packed blob)
                for tns in tensors:
                    if tns is not None and (tns.dtype != torch.float32 or not tns.is_contiguous() or tns.device != dev):
                        raise _capi.OardError("the general-edge-list path needs contiguous float32 parameters on the call's device")
                rc = L.oard_graph_forward(C.byref(cfg), topo.graph, _capi.ptr_array(tensors), len(tensors), xp, tt.data_ptr(), t_scalar,
                                          cond.data_ptr() if cond is not None else None, op, ws.data_ptr(), ws.numel(),
                                          status.data_ptr(), stream)
                _capi.check(rc, "oard_graph_forward")
            else:
                rc = L.oard_forward(C.byref(cfg), topo.handle, packed.data_ptr(), xp, tt.data_ptr(), t_scalar,
                                    cond.data_ptr() if cond is not None else None, op, ws.data_ptr(), ws.numel(), status.data_ptr(), stream)
                _capi.check(rc, "oard_forward")
            self._last_topo = topo
            self.last_status = status
            if self.nan_check != "sync":
                buffers.note(status)
            if self.nan_check == "replace":               # the reference's guard (:138-143) on the device: randn velocities iff the flag is set
                noise = [torch.randn(o.shape[0], self.pos_dim, device=dev) for o in outs]
                _capi.check(L.oard_nan_replace(C.byref(cfg), topo.handle, status.data_ptr(), _capi.ptr_array(noise), op, stream),
                            "oard_nan_replace")
            if self.nan_check == "sync" and int(status[0].item()) != 0:   # egnn_dynamics.py:138-143
                print("Warning: detected nan in pos, resetting EGNN output to randn.")
                for k in range(n_obj):
                    v = torch.randn_like(outs[k][:, : self.pos_dim])
                    idx = topo.obj_masks[k]
                    if v.shape[0]:
                        mean = torch.zeros(int(idx.max()) + 1, self.pos_dim, device=dev).index_add_(0, idx, v)
                        cnt = torch.zeros(int(idx.max()) + 1, device=dev).index_add_(0, idx, torch.ones_like(idx, dtype=v.dtype))
                        v = v - (mean / cnt.clamp(min=1).unsqueeze(1))[idx]
                    outs[k][:, : self.pos_dim] = v
        return outs, None

    @staticmethod
    def _time_argument(t: Tensor, dev, max_sample_id: int) -> Tuple[Tensor, int]:
        """egnn_dynamics.py:106-114: a 1-D t is ONE value for every node (`t.item()`, which raises unless numel == 1);
        otherwise t is indexed by combined_mask, i.e. [B, 1] with a row per sample."""
        tt = t.detach().to(device=dev, dtype=torch.float32)
        if t.dim() == 1:
            if tt.numel() != 1:
                raise ValueError("a 1-D `t` must hold exactly one value (the reference calls t.item())")
            return tt.contiguous(), 1
        if t.dim() != 2 or tt.shape[1] != 1:
            raise _capi.OardError("t must be 1-D with one element or [B, 1]")
        if tt.shape[0] <= max_sample_id:
            raise _capi.OardError("t has fewer rows than samples")
        return tt.reshape(-1).contiguous(), 0

    def _get_train_topology(self, cfg, edge_index: Optional[Tensor], n_frag_switch: Tensor, combined_mask: Tensor, stream: int,
                            device=None):
        """One (single sub-batch) topology per layout.  `edge_index` given: verified against the implicit complete graph when the
        topology is built (one host read); `None` (DDPMTrainer's fused step, which never materialises an edge list): nothing to
        verify.  `combined_mask` / `n_frag_switch` may be host tensors (`device` = the GPU).  Cached by the identity of the tensors:
        a loader that reuses its batch tensors pays the table build once; a new layout costs ~1.5 ms of host time and no device
        synchronisation (training.TrainTopology)."""
        from . import training
        return self._train_topo_cache.lookup((edge_index, n_frag_switch, combined_mask), (), lambda: training.TrainTopology(
            cfg, combined_mask, n_frag_switch, stream, edge_index=edge_index, device=device))

    def _run_forward_train(self, cfg, topo, packed: Tensor, xs: List[Tensor], tt: Tensor, t_scalar: int, cond: Optional[Tensor],
                           stream: int, reuse_tape: bool = False, buffers: Optional[_CallBuffers] = None):
        """oard_forward_train on prepared inputs -> (outs, TrainState); no autograd involved (DDPMTrainer's fused step calls this
        directly and feeds the closed-form loss gradient to training.backward_sweep).  `buffers`: the set this call writes to (None:
        the module's own)."""
        from . import training
        L = _capi.lib()
        dev = xs[0].device
        buffers = self._call_buffers if buffers is None else buffers
        outs = [torch.empty_like(x) for x in xs]
        ws = buffers.workspace(L.oard_workspace_bytes(C.byref(cfg), topo.handle), dev)
        # one tape per call (it lives until that call's backward has run; the caching allocator recycles it).  reuse_tape (the fused
        # trainer: one forward, then its backward, on one stream): the set's grow-only buffer
        tape_bytes = L.oard_tape_bytes(C.byref(cfg), topo.handle)
        tape = buffers.tape(tape_bytes, dev) if reuse_tape else torch.empty(tape_bytes, dtype=torch.uint8, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        rc = L.oard_forward_train(C.byref(cfg), topo.handle, packed.data_ptr(), _capi.ptr_array(xs), tt.data_ptr(), t_scalar,
                                  cond.data_ptr() if cond is not None else None, _capi.ptr_array(outs), ws.data_ptr(), ws.numel(),
                                  tape.data_ptr(), tape.numel(), status.data_ptr(), stream)
        _capi.check(rc, "oard_forward_train")
        self.last_status = status
        if self.nan_check != "sync":
            buffers.note(status)                      # device-side, no sync (DDPMTrainer reads it with the gradient norm)
        state = training.TrainState(cfg, topo, training.Tape(cfg, topo, tape), xs, tt, bool(t_scalar), cond)
        return outs, state

    def _forward_train(self, cfg, packed: Tensor, xh: List[Tensor], edge_index: Tensor, t: Tensor, conditions: Tensor,
                       n_frag_switch: Tensor, combined_mask: Tensor, stream: int):
        """Forward under autograd: training-mode HIP forward (tape) wrapped in `training.DynamicsFunction`."""
        from . import training
        dev = xh[0].device
        n_obj = len(self.node_nfs)
        topo = self._get_train_topology(cfg, edge_index, n_frag_switch, combined_mask, stream)
        xs, tt, t_scalar, cond = self._inputs(topo, xh, t, conditions, dev, detach=True)

        def run_forward():
            return self._run_forward_train(cfg, topo, packed, xs, tt, t_scalar, cond, stream)

        names = self._param_names()
        P = self._param_dict()
        outs = training.DynamicsFunction.apply(self, run_forward, n_obj, *xs, *[P[n] for n in names])
        if self.nan_check == "sync" and int(self.last_status[0].item()) != 0:       # egnn_dynamics.py:138-143
            raise FloatingPointError("NaN in the predicted displacement during training (the reference would replace "
                                     "it with randn and carry on; a training step on that is meaningless)")
        return list(outs), None

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def debug_tap(self, which: int) -> Tensor:
        """Intermediate tensor of the last forward (reference node/edge order); tests only."""
        topo = self._last_topo
        assert topo is not None and self._ws is not None
        if topo.handle is None:
            raise _capi.OardError("stage taps exist on the complete-graph path only (the last call ran the general-edge-list path)")
        H, R, L_, Cc = self._dims
        cfg = self._config()
        shape = {
            _capi.TAP_S: (topo.n_nodes, H), _capi.TAP_VEC: (topo.n_nodes, 3 * H), _capi.TAP_EDGE: (topo.n_edges, 3 * H + R),
            _capi.TAP_POS_FRAME: (topo.n_nodes, 3), _capi.TAP_DPOS: (topo.n_nodes, 3), _capi.TAP_HOUT: (topo.n_nodes, Cc),
            _capi.TAP_LABELS: (topo.n_nodes, 1), _capi.TAP_NE1: (topo.n_nodes, 3 * H),
        }[which]
        dst = torch.empty(shape, dtype=torch.float32, device=self._ws.device)
        with torch.cuda.device(dst.device):
            stream = torch.cuda.current_stream(dst.device).cuda_stream
            _capi.check(_capi.lib().oard_tap(C.byref(cfg), topo.handle, self._ws.data_ptr(), which, 0, dst.data_ptr(), stream),
                        "oard_tap")
        return dst

    @torch.no_grad()
    def active_inner_edges(self) -> int:
        """Same-object edges that were inside the cutoff in the last inference call - the rows EquiMessage ran (the others carry an
        exactly-zero message, model/leftnet.py:748-753, and are skipped); -1 if that call built no list.  Synchronises: a measurement aid."""
        topo = self._last_topo
        assert topo is not None and self._ws is not None
        if topo.handle is None:
            return -1                                            # general-edge-list path: no active list
        cfg = self._config()
        out = C.c_int64(0)
        with torch.cuda.device(self._ws.device):
            stream = torch.cuda.current_stream(self._ws.device).cuda_stream
            _capi.check(_capi.lib().oard_active_inner_edges(C.byref(cfg), topo.handle, self._ws.data_ptr(), self._ws.numel(),
                                                            C.byref(out), stream), "oard_active_inner_edges")
        return int(out.value)

    @staticmethod
    def compute_frag_index(n_frag_switch: Tensor):
        """egnn_dynamics.py:177-182."""
        import numpy as np
        counts = [int((n_frag_switch == ii).sum()) for ii in torch.unique(n_frag_switch)]
        return np.concatenate([np.array([0]), np.cumsum(counts)])

    @staticmethod
    def remove_mean_batch(x: Tensor, indices: Tensor) -> Tensor:
        """egnn_dynamics.py:268-271."""
        n = int(indices.max()) + 1 if indices.numel() else 0
        s = torch.zeros(n, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, indices, x)
        c = torch.zeros(n, dtype=x.dtype, device=x.device).index_add_(0, indices, torch.ones_like(indices, dtype=x.dtype))
        return x - (s / c.clamp(min=1).unsqueeze(1))[indices]


class _Topology:
    """Device index tables for one (combined_mask, n_frag_switch, edge_index) triple."""

    def __init__(self, cfg, edge_index: Tensor, n_frag_switch: Tensor, combined_mask: Tensor, stream: int, force_general: bool = False):
        L = _capi.lib()
        cm = combined_mask.detach().to("cpu", torch.int64).contiguous()          # one-off host copy
        nfs = n_frag_switch.detach().to("cpu", torch.int64).contiguous()
        if cm.numel() != nfs.numel() or cm.numel() == 0:
            raise _capi.OardError("combined_mask / n_frag_switch size mismatch")
        self._lib = L
        self.handle, self.graph = None, None
        self.key_tensors = None                        # set by the cache that holds this topology (_TensorKeyCache)
        self.n_nodes = int(cm.numel())
        self.max_sample_id = int(cm.max())
        n_obj = cfg.n_obj
        self.obj_counts = [int((nfs == k).sum()) for k in range(n_obj)]
        dev = combined_mask.device
        starts = [0]
        for c in self.obj_counts:
            starts.append(starts[-1] + c)
        self.obj_masks = [combined_mask.detach()[starts[k]: starts[k + 1]].to(torch.int64) for k in range(n_obj)]
        ei = edge_index.detach()
        if ei.dim() != 2 or ei.shape[0] != 2 or ei.dtype != torch.int64 or ei.device != dev:
            raise _capi.OardError("edge_index must be an int64 [2, E] tensor on the same device")
        ei = ei.contiguous()
        # the production kernels assume the complete-per-sample graph (any ordering of its edge list: outputs are per node): verify once.
        # A layout their tables do not cover (a (sample, object) group of more than 1024 atoms) cannot be that path's either way.
        # `force_general`: no production tables, no edge check, no host read.
        if not force_general:
            h = C.c_void_p()
            rc_topo = L.oard_topology_create(C.byref(cfg), C.cast(cm.data_ptr(), C.POINTER(C.c_int64)),
                                             C.cast(nfs.data_ptr(), C.POINTER(C.c_int64)), cm.numel(), C.byref(h))
            if rc_topo == _capi.OARD_OK:
                ok = torch.zeros(1, dtype=torch.int32, device=dev)
                _capi.check(L.oard_topology_check_edge_index(h, ei.data_ptr(), ei.shape[1], ok.data_ptr(), stream),
                            "oard_topology_check_edge_index")
                if int(ok.item()) == 1:
                    self.handle = h
                    self.n_edges = int(L.oard_topology_num_edges(h))
                    self.n_inner = int(L.oard_topology_num_inner_edges(h))
                    self.n_samples = int(L.oard_topology_num_samples(h))
                    return
                L.oard_topology_destroy(h)
        # not the complete graph per sample (edge_cutoff graphs, disconnected components, arbitrary lists: egnn_dynamics.py:63-72
        # accepts them all): the general-edge-list path (csrc/oard_general.h) takes the call.  One host copy of the edge list per
        # topology, like the two masks above.
        ei_host = ei.to("cpu").contiguous()
        g = C.c_void_p()
        rc_graph = L.oard_graph_create(C.byref(cfg), cm.data_ptr(), nfs.data_ptr(), cm.numel(), ei_host.data_ptr(), ei_host.shape[1], C.byref(g))
        _capi.check(rc_graph, "oard_graph_create (node ids out of range, or n_frag_switch not in ascending object blocks)")
        self.graph = g
        self.n_edges = int(L.oard_graph_num_edges(g))
        self.n_inner = int((nfs[ei_host[0]] == nfs[ei_host[1]]).sum()) if ei_host.shape[1] else 0
        self.n_samples = int(torch.unique(cm).numel())
        # (not forced: the production tables were refused, or the edge check said "not complete")
        if not force_general and L.oard_graph_is_complete(g):
            import warnings
            warnings.warn("this batch layout is outside the production kernels' tables (a (sample, object) group of more than 1024 atoms): "
                          "the complete graph is served by the general-edge-list path, which is built for parity, not throughput")

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._lib.oard_topology_destroy(self.handle)
            if getattr(self, "graph", None):
                self._lib.oard_graph_destroy(self.graph)
        except Exception:
            pass

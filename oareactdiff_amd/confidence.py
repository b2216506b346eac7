"""`Confidence` — drop-in for `oa_reactdiff.dynamics.confidence.Confidence(model=LEFTNet)`, the model the reference ranks generated
transition states with (wrapped by `ConfModule`, oa_reactdiff/trainer/pl_trainer.py:421-669; production widths in
oa_reactdiff/trainer/train_confidence_ts1x.py:42-54).

It is the denoiser's LEFTNet trunk with `for_conf=True` - the node scalars behind the last layer are its output
(model/leftnet.py:875-876) -, a mean over the nodes of every reaction and a `GatedMLP` readout H -> H -> H -> 1
(confidence.py:74-80, 157-163).  One library call, `oard_confidence_forward` (include/oard.h): the trunk's kernels up to the last
EquiUpdate, then `k_conf_readout` (csrc/oard_conf.h).  The module IS an `EGNNDynamics` as far as parameters, weight packing, topology
cache and call buffers go; the twelve `readout.*` tensors are read by the kernel where they lie.

FROZEN BY DEFAULT.  `Confidence(...)` is the inference module: the parameters are created with `requires_grad=False`, and a call with
autograd enabled on a parameter that was switched to require grad by hand raises `NotImplementedError`.  The reference's checkpoints
load here (`checkpoint.load_confidence_checkpoint`).

TRAINING: `Confidence(..., trainable=True)`.  The parameters require grad, and `_forward` / `forward` under autograd run
`oard_confidence_forward_train` - the training-mode trunk with its tape, the same readout kernel - and return logits whose `grad_fn`
is `ConfidenceFunction`.  Its backward is `oard_confidence_tail_backward` (csrc/oard_conf_bwd.h: the adjoint of mean pool + GatedMLP,
float64 behind float32 loads, which seeds the cotangent of the final node scalars and accumulates the twelve readout gradients) and
then the denoiser's own reverse sweep, unchanged: `training.Sweep.layer(l)` for l = L-1 .. 0 and `Sweep.init()`.  The tensors the
reference's autograd leaves without a gradient under for_conf (`CONF_UNUSED_PREFIXES`: the output head, the decoders and the two
modules no forward uses) get none here either.  Under `torch.no_grad()` a trainable module takes the inference entry: the same bits
as a frozen one.  `conf_trainer.ConfidenceTrainer` is the reference's `ConfModule` step on top of this."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from . import _capi
from .dynamics import EGNNDynamics, _TensorKeyCache
from .graph_tools import get_edges_index, get_mask_for_frag, get_n_frag_switch
from .spec import READOUT_NAMES, confidence_state_spec

FEATURE_MAPPING = ["pos", "one_hot", "charge"]                              # confidence.py:18
#: parameters the reference's autograd leaves at `.grad is None` under for_conf (leftnet.py:875-876 returns before the output head;
#: the wrapper's decoders are never called, confidence.py:82-163), besides the two modules no forward uses
CONF_UNUSED_PREFIXES = ("model.embedding_out.", "model.out_pos.", "decoders.", "model.distance_embedding.", "model.last_layer.")


class _Layout:
    """Batch-layout tensors of one set of masks / sizes (what `forward` derives per call in the reference, confidence.py:170-174)."""

    def __init__(self, combined_mask: Tensor, edge_index: Tensor, n_frag_switch: Tensor) -> None:
        self.combined_mask, self.edge_index, self.n_frag_switch = combined_mask, edge_index, n_frag_switch
        self.key_tensors = None


def rank_candidates(scores: Tensor, n_reactions: int) -> Tuple[Tensor, Tensor]:
    """`scores`: [K * n_reactions] scores of K candidates of each of `n_reactions` reactions, candidate-major (K repeats of the
    batch: entry k * n_reactions + r is candidate k of reaction r) -> (best_index [n_reactions], order [n_reactions, K]): the
    candidates of every reaction by descending score, ties by lower candidate index.  Device tensors in, device tensors out, no host
    read."""
    scores = scores.reshape(-1)
    if n_reactions < 1 or scores.numel() % n_reactions:
        raise ValueError(f"{scores.numel()} scores are not K candidates of each of {n_reactions} reactions")
    per_reaction = scores.reshape(-1, n_reactions).t()
    order = torch.argsort(per_reaction, dim=1, descending=True, stable=True)
    return order[:, 0], order


class RankingReport(NamedTuple):
    """Per reaction, `[n_reactions]` device tensors (`ranking_report`)."""
    spearman: Tensor          # float64: rank correlation of the scores with -RMSD over the K candidates (NaN where either is constant)
    top1_rmsd: Tensor         # RMSD of the candidate `rank_candidates` picks
    best_rmsd: Tensor         # the smallest RMSD among the candidates
    hit_at_1: Tensor          # bool: top1_rmsd < threshold
    regret: Tensor            # top1_rmsd - best_rmsd


def ranking_report(scores: Tensor, rmsd: Tensor, n_reactions: int, threshold: float = 0.2) -> RankingReport:
    """How good was the ordering `rank_candidates` gives, against known RMSDs?  `scores`, `rmsd`: [K * n_reactions], candidate-major
    as for `rank_candidates` -> `RankingReport`.  The Spearman correlation is one `oard_rank_metrics` call with one segment of K
    candidates per reaction (ties in the scores get their average rank); a higher score should mean a lower RMSD, hence -RMSD.
    Device tensors in, device tensors out, no host read."""
    from .metrics import rank_metrics
    scores, rmsd = scores.reshape(-1), rmsd.reshape(-1)
    if rmsd.numel() != scores.numel():
        raise ValueError(f"{scores.numel()} scores for {rmsd.numel()} RMSDs")
    best_index, _ = rank_candidates(scores, n_reactions)
    K = scores.numel() // n_reactions
    s_rm = scores.reshape(K, n_reactions).t().contiguous()                 # reaction-major: a reaction's candidates are one segment
    r_rm = rmsd.reshape(K, n_reactions).t().contiguous()
    sizes = torch.full((n_reactions,), K, dtype=torch.int64, device=scores.device)
    spearman = rank_metrics(s_rm, -r_rm, sizes).spearman
    top1 = r_rm.gather(1, best_index.reshape(-1, 1)).reshape(-1)
    best = r_rm.min(dim=1).values
    return RankingReport(spearman, top1, best, top1 < threshold, top1 - best)


class DistinctCandidates(NamedTuple):
    """Per reaction (`distinct_candidates`); K candidates each."""
    label: Tensor             # [n_reactions, K] int64: the candidate index of every candidate's cluster leader (a leader labels itself)
    is_leader: Tensor         # [n_reactions, K] bool
    n_clusters: Tensor        # [n_reactions] int64: how many different structures the K candidates hold
    order: Tensor             # [n_reactions, K] int64: `rank_candidates`' ordering, best score first


def distinct_candidates(scores: Tensor, x: Tensor, sizes, n_reactions: int, threshold: float = 0.1, match_order: bool = True,
                        ignore_chirality: bool = True, exact_limit: int = 10000) -> DistinctCandidates:
    """How many DIFFERENT structures do the K candidates of every reaction hold, and which is the best-scored member of each?  The
    reference's walkthrough answers with two host loops over pymatgen (the all-pairs RMSD matrix, demo.py:401-480, and the greedy
    de-duplication at 0.1, demo.py:544-557); here it is `metrics.pairwise_rmsd` and `metrics.leader_clusters`, on the device.
    Inputs candidate-major like `rank_candidates`: `scores` [K * n_reactions]; `x` the `[n, node_nf]` structures, segment after segment
    (`out_samples[0][1]` of an `inpaint` over K repeats of the batch), the coordinates its first three columns and the species its last
    column truncated to an integer, as `batch_rmsd(match_order=True)` reads it; `sizes` [K * n_reactions] their row counts.
    The candidates of a reaction are visited in `rank_candidates`' order (descending score), so the leader of every cluster is its
    best-scored member; a candidate joins the nearest leader within `threshold`, else it starts a cluster.  `match_order`: like atoms are
    matched first (`matched_rmsd`), otherwise rows are compared in the order given.  A candidate with a non-finite coordinate is a
    cluster of its own.  -> `DistinctCandidates`; `order[is_leader.gather(1, order)]` reads as "the distinct structures, best first".
    Device tensors in, device tensors out, no host read; anything off a ROCm device raises `OardError`."""
    from .metrics import candidate_groups, leader_clusters, pairwise_rmsd
    _, order = rank_candidates(scores, n_reactions)
    if not scores.is_cuda:
        raise _capi.OardError("distinct_candidates needs scores on a ROCm device (there is no CPU fallback)")
    K = scores.numel() // n_reactions
    n_sizes = int(sizes.numel()) if isinstance(sizes, Tensor) else len(sizes)
    if n_sizes != K * n_reactions:
        raise ValueError(f"{n_sizes} sizes for {K * n_reactions} candidates")
    dist = pairwise_rmsd(x, sizes, candidate_groups(n_reactions, K), species=x[:, -1] if match_order else None, match_order=match_order,
                         ignore_chirality=ignore_chirality, exact_limit=exact_limit)
    label, n_clusters = leader_clusters(dist, threshold, order=order.reshape(-1))
    label = label.reshape(n_reactions, K)
    return DistinctCandidates(label, label == torch.arange(K, device=label.device), n_clusters, order)


class ConfidenceFunction(torch.autograd.Function):
    """logits = Confidence._forward(...) with the HIP training-mode forward and the reverse sweep as backward.  Inputs after the fixed
    arguments: the xh tensors, then every parameter the forward uses (`Confidence._train_params`), so that autograd routes their
    gradients.  `conf.grad_inplace` as for `training.DynamicsFunction`: the sweep accumulates into the existing `.grad` tensors and
    autograd receives None."""

    @staticmethod
    def forward(ctx, conf, run_forward, n_obj, *tensors):
        logits, state = run_forward()
        ctx.conf, ctx.state, ctx.n_obj = conf, state, n_obj
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        from . import training
        conf, st = ctx.conf, ctx.state
        dev = st.xh[0].device
        P = conf._train_params()
        if conf.grad_inplace:
            out, dests = {}, training.inplace_gradients(P)
        else:
            out, dests = training.fresh_gradients(P, dev)
        with torch.cuda.device(dev), torch.no_grad():
            conf.backward_sweep(st, dlogits, dests, torch.cuda.current_stream(dev).cuda_stream)
        ctx.state = None
        return (None, None, None) + (None,) * ctx.n_obj + tuple(out.get(n) for n in P)


class Confidence(EGNNDynamics):
    _for_conf = True

    def __init__(
        self,
        model_config: Dict,
        fragment_names: List[str],
        node_nfs: List[int],
        edge_nf: int,
        condition_nf: int = 0,
        pos_dim: int = 3,
        edge_cutoff: Optional[float] = None,
        model=None,
        device: torch.device = torch.device("cuda"),
        enforce_same_encoding: Optional[List] = None,
        source: Optional[Dict] = None,
        trainable: bool = False,
        **kwargs,
    ) -> None:
        model_config.update({"for_conf": True})                             # confidence.py:54-56
        super().__init__(model_config, fragment_names, node_nfs, edge_nf, condition_nf, pos_dim, True, True, edge_cutoff, model,
                         device, enforce_same_encoding, source=source)
        full = confidence_state_spec(model_config, node_nfs, condition_nf, pos_dim, True)
        self._create_tensors({name: full[name] for name in READOUT_NAMES}, device)      # confidence.py:73-80
        self.trainable = bool(trainable)
        for p in self.parameters():                                         # frozen unless built to be trained (module docstring)
            p.requires_grad_(self.trainable)
        self.nan_check = "async"                                            # no host read in a call; the flag stays in `last_status`
        self._readout_slots = None
        self._layout_cache = _TensorKeyCache(8)                             # by the identity of the masks / sizes (forward)
        self._size_layouts: Dict[tuple, _Layout] = {}                       # by the atom counts (score_samples), as DiffusionSampler
        self._t0: Optional[Tensor] = None

    # ------------------------------------------------------------------------------------------
    def _readout_slot_list(self) -> list:
        """The (owning module, attribute) pair of every readout tensor, in READOUT_NAMES order (resolved once)."""
        if self._readout_slots is None:
            slots = []
            for name in READOUT_NAMES:
                mod = self
                for p in name.split(".")[:-1]:
                    mod = mod[int(p)] if p.isdigit() and isinstance(mod, torch.nn.ModuleList) else getattr(mod, p)
                slots.append((mod, name.rsplit(".", 1)[1]))
            self._readout_slots = slots
        return self._readout_slots

    def _readout_tensors(self, dev) -> List[Tensor]:
        out = [mod._parameters[attr] for mod, attr in self._readout_slot_list()]
        for t in out:
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise _capi.OardError("the readout parameters must be contiguous float32 tensors on the call's device")
        return out

    def _forward(
        self,
        xh: List[Tensor],
        edge_index: Tensor,
        t: Tensor,
        conditions: Tensor,
        n_frag_switch: Tensor,
        combined_mask: Tensor,
        edge_attr: Optional[Tensor] = None,
    ) -> Tensor:
        """confidence.py:82-163 -> [B] float32 logits, squeezed like the reference's (0-d for B = 1).  Row b belongs to the reaction
        whose `combined_mask` value is b."""
        if edge_attr is not None:
            raise NotImplementedError("edge attributes are not part of the LEFTNet path")
        train = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if train and not self.trainable:
            raise NotImplementedError("the MI355X Confidence model is inference only: a parameter requires grad and autograd is enabled, but "
                                      "this module was built frozen (call under torch.no_grad(), or build it with trainable=True)")
        dev = xh[0].device
        if dev.type != "cuda":
            raise _capi.OardError("Confidence needs tensors on a ROCm device (no CPU fallback)")
        L = _capi.lib()
        cfg = self._config()
        if L.oard_supported(C.byref(cfg)) != _capi.OARD_OK:
            raise NotImplementedError(f"hidden_channels={int(cfg.hidden)}, num_radial={int(cfg.num_radial)} is not a width pair the production "
                                      "kernels were built for, and the confidence readout runs behind those only - rebuild: "
                                      f"OARD_DIMS=\"196x96,{int(cfg.hidden)}x{int(cfg.num_radial)}\" python -m oareactdiff_amd.build")
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            packed = self._get_packed(cfg, stream)
            if train:
                return self._forward_train_conf(cfg, packed, xh, edge_index, t, conditions, n_frag_switch, combined_mask, stream)
            topo = self._get_topology(cfg, edge_index, n_frag_switch, combined_mask, stream)
            if topo.handle is None:
                raise NotImplementedError("edge_index is not the complete graph per reaction (get_edges_index(combined_mask, "
                                          "remove_self_edge=True)): the confidence model runs on the production kernels only, not on the "
                                          "general-edge-list path")
            if topo.max_sample_id != topo.n_samples - 1:
                raise _capi.OardError(f"combined_mask must name the reactions 0 .. B-1 with none missing: {topo.n_samples} reactions, "
                                      f"largest id {topo.max_sample_id}")
            xs, tt, t_scalar, cond = self._inputs(topo, xh, t, conditions, dev)
            conf = torch.empty(topo.n_samples, dtype=torch.float32, device=dev)
            buffers = self._call_buffers
            ws = buffers.workspace(L.oard_workspace_bytes(C.byref(cfg), topo.handle), dev)
            status = torch.zeros(2, dtype=torch.int32, device=dev)
            rc = L.oard_confidence_forward(C.byref(cfg), topo.handle, packed.data_ptr(), _capi.ptr_array(self._readout_tensors(dev)),
                                           _capi.ptr_array(xs), tt.data_ptr(), t_scalar, cond.data_ptr() if cond is not None else None,
                                           conf.data_ptr(), ws.data_ptr(), ws.numel(), status.data_ptr(), stream)
            _capi.check(rc, "oard_confidence_forward")
            self._last_topo = topo
            self.last_status = status
            buffers.note(status)
        return conf.squeeze()

    # ---- training (trainable=True) ------------------------------------------------------------------
    def _train_params(self) -> Dict[str, Tensor]:
        """Canonical name -> parameter for every distinct tensor the confidence forward uses, in state-dict order: the trunk without
        `CONF_UNUSED_PREFIXES`, then the twelve readout tensors."""
        P = {n: p for n, p in self._param_dict().items() if not n.startswith(CONF_UNUSED_PREFIXES)}
        dev = next(iter(P.values())).device
        P.update(zip(READOUT_NAMES, self._readout_tensors(dev)))
        return P

    def _check_train_topology(self, topo) -> None:
        if topo.max_sample_id != topo.B - 1:
            raise _capi.OardError(f"combined_mask must name the reactions 0 .. B-1 with none missing: {topo.B} reactions, "
                                  f"largest id {topo.max_sample_id}")

    def _run_forward_train_conf(self, cfg, topo, packed: Tensor, xs: List[Tensor], tt: Tensor, t_scalar: int, cond: Optional[Tensor],
                                stream: int, reuse_tape: bool = False):
        """oard_confidence_forward_train on prepared inputs -> (logits [B], TrainState); no autograd involved (ConfidenceTrainer calls
        this directly and feeds the closed-form loss gradient to `backward_sweep`)."""
        from . import training
        L = _capi.lib()
        dev = xs[0].device
        buffers = self._call_buffers
        conf = torch.empty(topo.B, dtype=torch.float32, device=dev)
        ws = buffers.workspace(L.oard_workspace_bytes(C.byref(cfg), topo.handle), dev)
        tape_bytes = L.oard_tape_bytes(C.byref(cfg), topo.handle)
        tape = buffers.tape(tape_bytes, dev) if reuse_tape else torch.empty(tape_bytes, dtype=torch.uint8, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        rc = L.oard_confidence_forward_train(C.byref(cfg), topo.handle, packed.data_ptr(), _capi.ptr_array(self._readout_tensors(dev)),
                                             _capi.ptr_array(xs), tt.data_ptr(), t_scalar, cond.data_ptr() if cond is not None else None,
                                             conf.data_ptr(), ws.data_ptr(), ws.numel(), tape.data_ptr(), tape.numel(),
                                             status.data_ptr(), stream)
        _capi.check(rc, "oard_confidence_forward_train")
        self.last_status = status
        buffers.note(status)
        return conf, training.TrainState(cfg, topo, training.Tape(cfg, topo, tape), xs, tt, bool(t_scalar), cond)

    def backward_sweep(self, st, dlogits: Tensor, dests: Dict[int, Tensor], stream: int) -> None:
        """The reverse sweep of one `_run_forward_train_conf`: d loss / d logit ([B], by reaction id) -> parameter gradients ACCUMULATED
        into `dests` (id(param) -> tensor) for every parameter of `_train_params` that has an entry."""
        from . import training
        dev = st.xh[0].device
        dconf = dlogits.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
        if dconf.numel() != st.topo.B:
            raise _capi.OardError(f"{dconf.numel()} logit cotangents for {st.topo.B} reactions")
        readout = self._readout_tensors(dev)
        training.backward_sweep(self, st, [], stream, dests, conf_tail=(readout, dconf, [dests.get(id(p)) for p in readout]))

    def _forward_train_conf(self, cfg, packed: Tensor, xh: List[Tensor], edge_index: Tensor, t: Tensor, conditions: Tensor,
                            n_frag_switch: Tensor, combined_mask: Tensor, stream: int) -> Tensor:
        """Forward under autograd: the training-mode HIP forward (tape) wrapped in `ConfidenceFunction`.  An edge list that is not the
        complete graph per reaction is refused when the topology is built (training.TrainTopology), as for the denoiser."""
        dev = xh[0].device
        topo = self._get_train_topology(cfg, edge_index, n_frag_switch, combined_mask, stream)
        self._check_train_topology(topo)
        xs, tt, t_scalar, cond = self._inputs(topo, xh, t, conditions, dev, detach=True)

        def run_forward():
            return self._run_forward_train_conf(cfg, topo, packed, xs, tt, t_scalar, cond, stream)

        logits = ConfidenceFunction.apply(self, run_forward, len(self.node_nfs), *xs, *self._train_params().values())
        return logits.squeeze()

    def _zero_time(self, dev) -> Tensor:
        if self._t0 is None or self._t0.device != dev:
            self._t0 = torch.zeros(1, dtype=torch.float32, device=dev)       # confidence.py:187: t = torch.tensor([0])
        return self._t0

    def forward(self, representations: List[Dict], conditions: Tensor) -> Tensor:
        """confidence.py:165-193.  The layout tensors are cached by the identity of the representations' masks and sizes: a caller that
        scores batch after batch of one layout pays for the edge list and the index tables once."""
        masks = [r["mask"] for r in representations]
        sizes = [r["size"] for r in representations]

        dev = representations[0]["pos"].device

        def build():
            combined_mask = torch.cat(masks).to(dev)
            return _Layout(combined_mask, get_edges_index(combined_mask, remove_self_edge=True),
                           get_n_frag_switch([s.to(dev) for s in sizes]))
        lay = self._layout_cache.lookup(tuple(masks) + tuple(sizes), (str(dev),), build)
        xh = [torch.cat([r[f] for f in FEATURE_MAPPING], dim=1) for r in representations]
        return self._forward(xh=xh, edge_index=lay.edge_index, t=self._zero_time(dev), conditions=conditions,
                             n_frag_switch=lay.n_frag_switch, combined_mask=lay.combined_mask, edge_attr=None)

    # ------------------------------------------------------------------------------------------
    def _layout_of_sizes(self, fragments_nodes: List[Tensor], dev) -> _Layout:
        key = tuple(tuple(int(v) for v in f.tolist()) for f in fragments_nodes)
        hit = self._size_layouts.get(key)
        if hit is None or hit.combined_mask.device != dev:
            fn = [f.to(dev) for f in fragments_nodes]
            combined_mask = torch.cat([get_mask_for_frag(f) for f in fn])
            hit = _Layout(combined_mask, get_edges_index(combined_mask, remove_self_edge=True), get_n_frag_switch(fn))
            if len(self._size_layouts) >= 4:
                self._size_layouts.pop(next(iter(self._size_layouts)))
            self._size_layouts[key] = hit
        return hit

    @torch.no_grad()
    def score_samples(self, fragments_nodes: List[Tensor], samples: List[Tensor], conditions: Optional[Tensor] = None,
                      probability: bool = True) -> Tensor:
        """Scores what `DiffusionSampler.sample` / `inpaint` return: `samples` = `out_samples[0]`, one [n_k, node_nf_k] tensor
        [pos | one_hot | charge] per object, laid out by `fragments_nodes` (atoms per reaction, per object).  -> [B] scores;
        `probability`: the sigmoid of the logits, as `ConfModule` applies it (pl_trainer.py:565).  The samples stay on the device."""
        dev = next(self.parameters()).device
        lay = self._layout_of_sizes(fragments_nodes, dev)
        if conditions is None:
            conditions = torch.zeros(int(fragments_nodes[0].numel()), max(self.condition_nf, 1), device=dev)
        xh = [x.to(device=dev, dtype=torch.float32) for x in samples]
        logits = self._forward(xh, lay.edge_index, self._zero_time(dev), conditions.to(dev), lay.n_frag_switch, lay.combined_mask)
        logits = logits.reshape(-1)
        return torch.sigmoid(logits) if probability else logits

    rank_candidates = staticmethod(rank_candidates)
    ranking_report = staticmethod(ranking_report)

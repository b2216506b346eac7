"""One training step of the diffusion model around the HIP denoiser (BASELINE config 4).

`DDPMTrainer.training_step` mirrors `DDPMModule.training_step` + `configure_optimizers` + `configure_gradient_clipping`
(oa_reactdiff/trainer/pl_trainer.py:327-347, :150-160, :391-418) and the data-parallel strategy of
oa_reactdiff/trainer/train_ts1x.py:197-203 (Lightning `DDPStrategy`):

    nll, info = compute_loss(batch);  loss = nll.mean(0)            pl_trainer.py:328-329
    loss.backward()                                                  HIP backward (oareactdiff_amd/training.py)
    gradients averaged over the ranks                                DDP: here ONE all-reduce of one flat bucket
    adaptive gradient clipping (queue of recent norms)               pl_trainer.py:391-418
    AdamW(amsgrad=True) step                                         pl_trainer.py:150, train_ts1x.py:66-71

Multi-GPU: one process per GPU (`torch.distributed`, backend "nccl" = RCCL over xGMI on ROCm), every rank holds a
replica and its own shard of the batch.  All trainable gradients live in ONE contiguous fp32 buffer (`flat_grad`,
42.6 MB for the production model): `param.grad` are views into it, so the backward pass accumulates in place and the
step needs exactly one `all_reduce` — sized for xGMI's per-link bound rather than bucketed for overlap (the backward
of this model takes tens of ms, the all-reduce of 42.6 MB over 7 links well under 1 ms).  The two modules the forward
never uses (`model.distance_embedding`, `model.last_layer`; Lightning needs `find_unused_parameters=True` for them) are
left out of the bucket and never get a gradient, as in the reference.
"""
from __future__ import annotations

import copy
import ctypes as C
import math
import os
import warnings
from collections import OrderedDict
from collections.abc import Mapping
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist
from torch import Tensor, nn

from . import _capi, training
from .dynamics import _CallBuffers
from .flat_state import FlatLayout, FlatTrainerState, Queue, bind_to_average, clip_decision  # noqa: F401  (Queue: this module's public name for it)
from .loss import DiffusionLoss

UNUSED_PREFIXES = ("model.distance_embedding.", "model.last_layer.")
DEFAULT_OPTIMIZER = dict(lr=2.5e-4, betas=(0.9, 0.999), weight_decay=0, amsgrad=True)      # train_ts1x.py:66-71


def vlb_snr_table(schedule) -> Tensor:
    """SNR_weight of every time step, float32 [T + 1]: entry t = 1 - exp(-(gamma[t - 1] - gamma[t])) (en_diffusion.py:139-140 with
    s = t - 1/T), evaluated in float64 on the schedule's gamma table widened to float64 - what the reference's float64 run sees - and
    rounded once.  In float32 most digits of the ~1e-3 difference cancel.  Entry 0 is 0 and is never read for valid input: in
    evaluation t_int lies in [1, T] (the reference's own lookup at t = 0 would wrap around to gamma[T])."""
    g = schedule.gamma.double().numpy()
    out = np.zeros(g.shape[0], dtype=np.float64)
    out[1:] = -np.expm1(-(g[:-1] - g[1:]))
    return torch.from_numpy(out.astype(np.float32))


class LazyInfo(Mapping):
    """What `training_step` returns with `host_sync=False`: the same keys as the eager dict (loss, skipped, grad_norm, max_grad_norm,
    error_t_k, unorm_error_t_k), held as two small device tensors and copied to the host the first time any of them is read."""

    def __init__(self, stats: Tensor, out4: Tensor, K: int, scales: List[float], clip: bool):
        self._dev = (stats, out4)
        self._K, self._scales, self._clip = K, scales, clip
        self._d: Optional[Dict[str, float]] = None

    def _get(self) -> Dict[str, float]:
        if self._d is None:
            stats, out4 = (t.tolist() for t in self._dev)
            K, d = self._K, {}
            for k in range(K):
                d[f"error_t_{k}"] = stats[3 + k] / (self._scales[k] + 1e-4)
                d[f"unorm_error_t_{k}"] = stats[3 + K + k]
            if self._clip:
                d["grad_norm"], d["max_grad_norm"] = out4[0], out4[1]
            d["loss"] = stats[2]
            d["skipped"] = int(out4[3] != 0)
            self._d, self._dev = d, None
        return self._d

    def __getitem__(self, key):
        return self._get()[key]

    def __iter__(self):
        return iter(self._get())

    def __len__(self):
        return len(self._get())


class DDPMTrainer(FlatTrainerState):
    CLIP_FACTORS = (1.5, 3.0)                          # pl_trainer.py:391-418: 150 % of the recent mean norm + 3 standard deviations
    SKIP_MESSAGE = "Warning: non-finite loss / gradient / network output on some rank: step skipped on all ranks ({} so far)"

    def __init__(self, dynamics: nn.Module, noise_schedule: str = "polynomial_2", timesteps: int = 1000,
                 precision: float = 1e-5, norm_values: Sequence[float] = (1.0, 1.0, 1.0),
                 norm_biases: Sequence[float] = (0.0, 0.0, 0.0), loss_type: str = "l2", pos_only: bool = False,
                 scales: Sequence[float] = (1.0, 1.0, 1.0), fixed_idx: Optional[List[int]] = None,
                 optimizer_config: Optional[Dict] = None, clip_grad: bool = True,
                 process_group: Optional["dist.ProcessGroup"] = None, fused: Optional[bool] = None, host_sync: bool = True,
                 microbatches: int = 1, ema_decay: Optional[float] = None):
        """`ema_decay=d` (0 <= d <= 1; None: no average, no buffer): an exponential moving average of the trainable weights, updated
        after every optimiser step that is taken - what the reference wires as `EMACallback` (trainer/train_ts1x.py:188-189,
        trainer/ema.py:37-47: timm's `ModelEmaV2.update` after every batch), in float32:
            ema = fl(fl(d32 * ema) + fl(w32 * p_new)),   d32 = float32(d), w32 = float32(1.0 - d)
        i.e. bit for bit torch's `decay * e + (1. - decay) * m`.  It starts as a copy of the weights (after `sync_replicas`), lives in ONE
        flat buffer `flat_ema` laid out like the gradient bucket, and a skipped step leaves it untouched.  The fused step folds the line
        into the AdamW kernel (`oard_adamw_step_ema` / `oard_adamw_step_dev_ema`: no extra launch); the generic step evaluates the same
        expression per tensor.  NAMING: `d` is timm's decay, the weight of the OLD average.  The reference's `EMACallback(decay=x)` hands
        `1 - x` to timm (ema.py:29) and train_ts1x.py passes `ema_decay=0.999` into it - to reproduce that callback pass `1 - x` here.
        Use the average through `ema_dynamics`, `ema_state_dict()`, `compute_loss(..., weights="ema")` and `copy_ema_to_model()`.

        `microbatches=2` (fused steps on batches that carry their host copies, `to_device`): the step's reactions are dealt to two
        halves that run their forward and their reverse sweep CONCURRENTLY on two streams (the caller's and the library's idle
        sub-batch stream), each with its own tape / workspace / scratch and its own gradient buffer, summed before the all-reduce.
        Same loss, same gradient up to the order of one addition; the low-occupancy node-side launches of one half then run beside
        the other half's edge kernels instead of alone on the chip (round 6).

        `host_sync=False` (fused steps only): the adaptive-clipping decision, the skip decision and AdamW's step-dependent scalars
        are evaluated on the device (`oard_adamw_step_dev`), so a training step contains NO device -> host read; `training_step`
        then returns a `LazyInfo` whose values are fetched when they are first looked at.  Arithmetic and state are the same as with
        `host_sync=True` (the clipping history is summed in numpy's order); the clipping / skip messages are not printed."""
        self.dynamics = dynamics
        self.host_sync = bool(host_sync)
        if int(microbatches) not in (1, 2):
            raise ValueError("microbatches must be 1 or 2")
        self.microbatches = int(microbatches)
        self._mb = None                                # second micro-batch: stream, gradient buffer, its own per-call buffers
        self._clip_state = None                        # device mirror of (history, opt_step, skipped_steps) while host_sync is off
        self.loss = DiffusionLoss(dynamics, noise_schedule, timesteps, precision, norm_values=norm_values,
                                  norm_biases=norm_biases, pos_only=pos_only, fixed_idx=fixed_idx, loss_type=loss_type,
                                  scales=scales)
        # what a DiffusionSampler of this model needs besides the schedule (eval_inpaint_batch builds one per schedule / weights, lazily)
        self._sampler_kw = dict(precision=precision, pos_only=pos_only, norm_values=tuple(norm_values), norm_biases=tuple(norm_biases))
        self._eval_samplers: Dict[Tuple[str, int, str], object] = {}
        self.last_rmsds: Optional[Tensor] = None        # per-reaction RMSDs of the last eval_inpaint_batch (device, [B])
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        self.time_collectives = False                      # True: all_reduce_gradients brackets the collective with timing events (collective_report)
        self._collective_events = []
        # the collectives run with more than one rank - or, for a smoke test of the RCCL path on a one-GPU box, whenever a process
        # group exists and OARD_FORCE_COLLECTIVES is set (a one-rank broadcast / all-reduce is the identity)
        self.collectives = self.world > 1 or (dist.is_available() and dist.is_initialized()
                                              and bool(os.environ.get("OARD_FORCE_COLLECTIVES")))
        # distinct trainable parameters the forward uses, in state-dict order (shared encoders count once)
        seen, self.params, self.names = set(), [], []
        for name, p in dynamics.named_parameters():
            if p.requires_grad and id(p) not in seen and not name.startswith(UNUSED_PREFIXES):
                seen.add(id(p))
                self.params.append(p)
                self.names.append(name)
        self._lay_out(1, ema_decay, clip_grad)         # no alignment padding; p.grad = view into the bucket: backward accumulates in place
        n = self.layout.size
        # one bucket: [gradients (n) | non-finite flag (1)]; the flag rides in the same all-reduce so that every rank takes the
        # same skip / step decision after the collective (a rank that bails out BEFORE it would leave the others hanging)
        self._bucket = torch.zeros(n + 1, dtype=self.params[0].dtype, device=self.params[0].device)
        self._ema_dynamics = None                      # the shadow module, built at the first look at `ema_dynamics`
        self._ema_warned = False
        self._ema_view_list = None
        if self.collectives:
            self.sync_replicas()
        self.opt_config = dict(DEFAULT_OPTIMIZER, **(optimizer_config or {}))
        can_fuse = (hasattr(dynamics, "_get_packed_bwd") and self.params[0].device.type == "cuda" and loss_type == "l2"
                    and self.params[0].dtype == torch.float32)
        if fused and not can_fuse:                     # the fused kernels implement the l2 objective in float32 on the HIP module only
            raise ValueError("fused=True needs the HIP EGNNDynamics on a ROCm device, float32 parameters and loss_type='l2' "
                             f"(got loss_type={loss_type!r}, dtype={self.params[0].dtype}, device={self.params[0].device})")
        self.fused = can_fuse if fused is None else bool(fused)
        if not self.host_sync and not self.fused:
            raise ValueError("host_sync=False is a mode of the fused step (HIP EGNNDynamics on a ROCm device, l2 loss)")
        if self.fused:
            # the HIP module: (1) its backward accumulates straight into the .grad views of the bucket; (2) the parameters
            # themselves become views of ONE flat buffer, so that AdamW is a single kernel over it (oard_adamw_step) and
            # state_dict() / load_state_dict() keep working on the same storage
            dynamics.grad_inplace = True
        self._bind(self._bucket[:n], torch.empty(n, dtype=torch.float32, device=self._bucket.device) if self.fused else None)
        # `trainer.optimizer` is what the reference's configure_optimizers returns (pl_trainer.py:149-151): the generic path steps it;
        # the fused path runs oard_adamw_step on the flat buffers but reads lr / betas / eps / weight_decay / amsgrad from
        # `optimizer.param_groups[0]` at EVERY step, so an LR scheduler attached to it (or an edit of the group) takes effect in
        # both modes.  The fused moments live in `exp_avg` / `exp_avg_sq` / `max_exp_avg_sq` / `opt_step`: see state_dict().
        self.optimizer = torch.optim.AdamW(self.params, **self.opt_config)
        self._gamma_dev = None
        self._snr_dev = None                           # SNR_weight per time step (vlb_snr_table), uploaded at the first eval_loss
        self._val_div: Dict[tuple, Tensor] = {}        # the divisors of validation_step's logged means, per (device, dtype)
        self._val_kept: Dict[str, Tuple[List[Tensor], List[Tensor]]] = {}      # prefix -> (rows, per-reaction nll) since the last epoch end

    # ---- resume: what Lightning's checkpoint keeps of the reference trainer (`optimizer_states`, pl_trainer.py:149-151; the clipping
    # history `gradnorm_queue` is NOT checkpointed by the reference and restarts at [3000], :143-146 - it is kept here) -------------
    def state_dict(self) -> Dict:
        """Everything a bit-identical continuation of the training needs besides the module's own state_dict(): the optimiser state
        (fused: flat AdamW moments + step counter + the hyper-parameters of `optimizer.param_groups`; generic: torch's), the clipping
        history and the skipped-step counter."""
        self._pull_clip_state()
        sd: Dict = {"fused": bool(self.fused), **super().state_dict()}
        if not self.fused:
            sd["optimizer"] = copy.deepcopy(self.optimizer.state_dict())     # a snapshot: torch hands out the live moment tensors
        return sd

    def load_state_dict(self, sd: Dict) -> None:
        if list(sd["names"]) == list(self.names) and bool(sd["fused"]) != bool(self.fused):      # (other names: the error below)
            raise ValueError(f"trainer state was saved with fused={sd['fused']}, this trainer runs fused={self.fused}")
        super().load_state_dict(sd)
        self._clip_state = None                        # rebuilt from the host copies at the next sync-free step
        if not self.fused:
            self.optimizer.load_state_dict(sd["optimizer"])
        if self.flat_ema is not None:
            if sd.get("ema") is None:                  # the run that wrote this state kept no average: start one from the weights it resumes
                if not self._ema_warned:
                    self._ema_warned = True
                    warnings.warn("trainer state holds no EMA: the average restarts from the current weights")
                with torch.no_grad():
                    self.flat_ema.copy_(self._flat_weights())
            if self._ema_dynamics is not None:
                self._ema_dynamics.invalidate_packed()

    # ---- host_sync=False: history / step counter / skip counter live on the device between reads ------------------------------------------
    CLIP_CAPACITY = 50                                 # utils/training_tools.py:9 (Queue(max_len=50))

    def _push_clip_state(self) -> Tensor:
        """Device copy of the host-side clipping history, optimiser step count and skip count (layout: include/oard.h, oard_adamw_step_dev)."""
        cap = self.CLIP_CAPACITY
        items = list(self.gradnorm_queue.items) if self.clip_grad else []
        host = torch.zeros(4 + cap + 8, dtype=torch.float64)
        host[0], host[1], host[2] = len(items), self.opt_step, self.skipped_steps
        if items:
            host[4: 4 + len(items)] = torch.tensor(items, dtype=torch.float64)
        self._clip_state = host.to(self.flat_grad.device)
        return self._clip_state

    def _pull_clip_state(self) -> None:
        """Refresh `gradnorm_queue`, `opt_step`, `skipped_steps` from the device (one host sync; no-op while host_sync is on)."""
        if self._clip_state is None:
            return
        host = self._clip_state.cpu()
        n = int(host[0])
        self.opt_step, self.skipped_steps = int(host[1]), int(host[2])
        if self.clip_grad:
            self.gradnorm_queue.items = [float(x) for x in host[4: 4 + n].tolist()]

    @staticmethod
    def to_device(batch, device, non_blocking: bool = True):
        """A host batch (the dataset's collate output: per object {size, pos, one_hot, charge, mask}, conditions) moved to `device`
        with the HOST copies of `mask` / `size` kept beside the device tensors (`mask_host`, `size_host`): the fused step builds the
        batch layout from them, so a never-seen layout - every step of a real training run - costs no device -> host copy.  Batches
        without the host copies work as before (one blocking copy of the masks per new layout).  `data.DeviceLoader` yields batches in
        this layout straight from a device-resident dataset, host copies included: they need no `to_device`."""
        reps, cond = batch
        out = []
        for r in reps:
            d = {k: (v.to(device, non_blocking=non_blocking) if isinstance(v, Tensor) else v) for k, v in r.items()}
            d["mask_host"], d["size_host"] = r["mask"].detach().cpu(), r["size"].detach().cpu()
            out.append(d)
        return out, (cond.to(device, non_blocking=non_blocking) if isinstance(cond, Tensor) else cond)

    # pl_trainer.py:208-282
    def compute_loss(self, batch, training: bool = True, weights: str = "live", **kw) -> Tuple[Tensor, Dict[str, float]]:
        """`weights="ema"` (evaluation only): the loss under the averaged weights, through `ema_dynamics` - the reference's validation
        under EMA weights (ema.py:49-60) without its store / copy / restore of the live ones."""
        representations, conditions = batch
        if weights == "live":
            return self.loss.compute_loss(representations, conditions, training=training, **kw)
        if weights != "ema":
            raise ValueError("weights must be 'live' or 'ema'")
        if training:
            raise ValueError("weights='ema' evaluates (training=False): the average is not what the optimiser steps")
        self.loss.dynamics = self.ema_dynamics
        try:
            with torch.no_grad():
                return self.loss.compute_loss(representations, conditions, training=False, **kw)
        finally:
            self.loss.dynamics = self.dynamics

    # pl_trainer.py:284-325
    def eval_inpaint_batch(self, batch, resamplings: int = 5, jump_length: int = 5, frag_fixed: Sequence[int] = (0, 2), idx: int = 1,
                           weights: str = "live", noise_schedule: str = "polynomial_2", timesteps: Optional[int] = None,
                           cap: Optional[float] = 1.0, noise_fn=None, match_order: bool = False) -> Tuple[float, float]:
        """The validation metric of the reference's `eval_inplaint_batch` (pl_trainer.py:284-325, logged by training_step / _shared_eval):
        object `idx` (the transition state) of every reaction of `batch` is inpainted with the objects `frag_fixed` (reactant, product)
        held fixed, and the (mean, median) RMSD between the generated and the true structure is returned.
            xh_fixed = cat(pos, one_hot, charge) per object;  fragments_nodes = the batch's `size` tensors
            out_samples, _ = DiffusionSampler.inpaint(...)           the fused RePaint loop (sampler.py)
            rmsds = metrics.batch_rmsd(fragments_nodes, out_samples[0], xh_fixed, idx, cap=cap)      one launch, one wavefront per reaction
        `noise_schedule` / `timesteps` stand for the reference's separate `sampling_schedule` (None: the trainer's own timesteps); the
        sampler is built once per (noise_schedule, timesteps, weights) and reused.  `weights="ema"` samples through `ema_dynamics`: no
        weight is copied in either direction (the reference swaps a snapshot in and out, ema.py:49-60).  `cap` is `batch_rmsd`'s: 1.0 as in
        the reference, None for the uncapped numbers; a reaction whose sample is not finite counts `cap` (None: it is left out).
        Mean and median are taken on the device over the finite entries, the median as numpy's (the mean of the two middle values of an
        even count); no finite entry gives (nan, nan).  The per-reaction tensor stays in `self.last_rmsds` ([B], device).
        Host reads: the loop's NaN flag and the two returned scalars - given a batch that carries `size_host` (`to_device`); the batch
        layout is otherwise read from the device `size` tensors once per new layout.  A NaN network output does not raise: the loop
        warns, and the affected reactions are the non-finite ones above.
        The call changes no weight, no optimiser or EMA state, and neither the module's `training` flag nor its `nan_check`.
        RMSD as in `oareactdiff_amd.metrics.batch_rmsd`: `match_order=False` compares atoms in the order given (an inpainted transition
        state keeps the order of the fixed reactant and product); `match_order=True` matches like atoms first, as the reference's
        `rmsd_core` does, in the same one launch and with the same host reads - never a larger number.  A generated atom whose charge
        column does not truncate to the true atomic number makes the species lists differ: that reaction counts `cap`."""
        from .metrics import batch_rmsd
        from .sampler import DiffusionSampler
        if weights not in ("live", "ema"):
            raise ValueError("weights must be 'live' or 'ema'")
        T = int(self.loss.T if timesteps is None else timesteps)
        key = (str(noise_schedule), T, weights)
        smp = self._eval_samplers.get(key)
        if smp is None:
            dyn = self.dynamics if weights == "live" else self.ema_dynamics
            smp = self._eval_samplers[key] = DiffusionSampler(dyn, noise_schedule, T, on_nan="warn", **self._sampler_kw)
        representations, conditions = batch
        xh_fixed = [torch.cat([r["pos"], r["one_hot"], r["charge"]], dim=1) for r in representations]
        fragments_nodes = [r["size"] for r in representations]
        n_samples = int(fragments_nodes[0].numel())
        out_samples, _ = smp.inpaint(n_samples, [r.get("size_host", r["size"]) for r in representations], conditions=conditions,
                                     return_frames=1, resamplings=resamplings, jump_length=jump_length, timesteps=None,
                                     xh_fixed=xh_fixed, frag_fixed=list(frag_fixed), noise_fn=noise_fn)
        dev = out_samples[0][idx].device
        with torch.no_grad():
            r = batch_rmsd([f.to(dev) for f in fragments_nodes], out_samples[0], [x.to(dev) for x in xh_fixed], idx=idx, cap=cap,
                           match_order=match_order)
            self.last_rmsds = r
            fin = torch.isfinite(r)
            cnt = fin.sum()
            r64 = r.double()
            mean = torch.where(fin, r64, torch.zeros_like(r64)).sum() / cnt                      # 0 / 0 = nan without a finite entry
            ordered = torch.sort(torch.where(fin, r64, torch.full_like(r64, float("inf")))).values      # the finite ones first
            mid = torch.stack([(cnt - 1).clamp(min=0) // 2, cnt // 2]).clamp(max=max(n_samples - 1, 0))
            median = ordered[mid].mean() if n_samples else mean
            median = torch.where(cnt > 0, median, torch.full_like(median, float("nan")))
            mean, median = torch.stack([mean, median]).tolist()                                  # the one read of the two scalars
        return mean, median

    # ---- validation: the variational bound of a batch on the device, the epoch's means (pl_trainer.py:349-382, `_shared_eval`) --------------
    def _can_eval_fused(self) -> bool:
        """The two evaluation kernels need what the fused step needs except the l2 objective: the HIP module on a ROCm device, float32."""
        return (hasattr(self.dynamics, "_get_packed_bwd") and self.params[0].device.type == "cuda"
                and self.params[0].dtype == torch.float32)

    def eval_loss(self, batch, weights: str = "live", t_int: Optional[Tensor] = None, draw=None) -> Tuple[Tensor, Tensor]:
        """The evaluation half of `EnVariationalDiffusion.forward` + `DDPMModule.compute_loss` (en_diffusion.py:56-248,
        pl_trainer.py:246-282) -> (nll [B], terms [5 K + 2, B]), both on the device, for K objects:
            rows [0, K) error_t per object, normalised and scaled   [K, 2K) error_t   [2K, 3K) loss_0_x   [3K, 4K) loss_0_cat
            [4K, 5K) loss_0_charge   row 5K SNR_weight   row 5K + 1 neg_log_constants
            nll = sum_k(-T/2 SNR_weight error_t_k) + sum_k(loss_0_x + loss_0_cat + loss_0_charge)_k + neg_log_constants - delta_log_px
        On a ROCm device with the HIP module: `oard_loss_eval_prepare` (ONE launch for z_t and z_0), two inference network calls (at t
        and at 0: the non-taping `oard_forward`, no gradient work) on the layout built from the batch's host copies of mask / size when
        `to_device` kept them, `oard_loss_eval_terms` - no device -> host read.  `t_int` is drawn with randint(1, T + 1) on the device
        and must lie in [1, T]; the noise of both representations is ONE randn.  Injected `draw` follows DiffusionLoss's protocol: per
        object (n, 3) then (n, nf - 3) for z_t, then the same again for z_0.  `weights="ema"` runs `ema_dynamics` (ValueError on a
        trainer without `ema_decay`).  An empty (sample, object) group contributes 0 (DiffusionLoss gives NaN there).
        Anywhere else (CPU, a network that is not the HIP module): the same table from `DiffusionLoss.loss_terms(training=False)`.
        Changes no weight, no optimiser, clip or EMA state, and neither the module's `training` flag nor its `nan_check`."""
        if weights not in ("live", "ema"):
            raise ValueError(f"weights must be 'live' or 'ema' (got {weights!r})")
        if weights == "ema" and self.flat_ema is None:
            raise ValueError("this trainer keeps no average of the weights (DDPMTrainer(ema_decay=...))")
        dyn = self.dynamics if weights == "live" else self.ema_dynamics
        if self._can_eval_fused():
            return self._eval_loss_fused(dyn, batch, t_int, draw)
        reps, cond = batch
        ls = self.loss
        ls.dynamics = dyn
        try:
            lt = ls.loss_terms(reps, cond, training=False, t_int=t_int, draw=draw)
        finally:
            ls.dynamics = self.dynamics
        nll, _ = ls.nll_and_info(lt, reps, training=False, lazy_info=True)
        K = len(reps)
        width = [ls.pos_dim if ls.pos_only else ls.pos_dim + ls.node_nfs[k] for k in range(K)]
        err_n = [lt["error_t"][k] / (width[k] * reps[k]["size"]) * ls.scales[k] for k in range(K)]
        rows = err_n + [lt[key][k] for key in ("error_t", "loss_0_x", "loss_0_cat", "loss_0_charge") for k in range(K)]
        return nll, torch.stack(rows + [lt["SNR_weight"], lt["neg_log_constants"]])

    def _infer(self, dyn, cfg, topo, packed: Tensor, xh: List[Tensor], t: Tensor, cond, stream: int) -> List[Tensor]:
        """One inference network call (`oard_forward`: no tape) on the single-sub-batch topology the loss kernels share."""
        L = _capi.lib()
        dev = xh[0].device
        xs, tt, t_scalar, cnd = dyn._inputs(topo, xh, t, cond, dev, detach=True)
        outs = [torch.empty_like(x) for x in xs]
        ws = dyn._call_buffers.workspace(L.oard_workspace_bytes(C.byref(cfg), topo.handle), dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        _capi.check(L.oard_forward(C.byref(cfg), topo.handle, packed.data_ptr(), _capi.ptr_array(xs), tt.data_ptr(), t_scalar,
                                   cnd.data_ptr() if cnd is not None else None, _capi.ptr_array(outs), ws.data_ptr(), ws.numel(),
                                   status.data_ptr(), stream), "oard_forward")
        return outs

    def _eval_loss_fused(self, dyn, batch, t_int: Optional[Tensor], draw) -> Tuple[Tensor, Tensor]:
        reps, cond = batch
        ls = self.loss
        dev = self.flat_grad.device
        K = len(reps)
        L = _capi.lib()
        masks, sizes = [r["mask"] for r in reps], [r["size"] for r in reps]
        have_host = all("mask_host" in r and "size_host" in r for r in reps)
        B = int(sizes[0].numel())
        with torch.cuda.device(dev), torch.no_grad():
            stream = torch.cuda.current_stream(dev).cuda_stream
            cfg = dyn._config()
            _capi.check(L.oard_supported(C.byref(cfg)), "oard_supported (hidden_channels/num_radial not built)")
            packed = dyn._get_packed(cfg, stream)
            nfs = list(dyn.node_nfs)
            if t_int is None:
                t_int = torch.randint(1, ls.T + 1, size=(B,), device=dev).float()
            t_int = t_int.detach().to(device=dev, dtype=torch.float32).reshape(B).contiguous()
            counts = [int(m.numel()) for m in masks]
            noise = self._noise_blocks(counts, nfs, draw, 2, dev)          # z_t's block, then z_0's
            hm = [r["mask_host"] for r in reps] if have_host else masks
            hs = [r["size_host"] for r in reps] if have_host else sizes
            combined_mask, _, n_frag_switch = ls._layout(hm, hs, need_edges=False)
            topo = dyn._get_train_topology(cfg, None, n_frag_switch, combined_mask, stream, device=dev)
            gamma, snr = self._eval_tables(dev)
            pos, one_hot, charge, nv, nb, sc = self._loss_operands(reps)
            z_t, eps_t, z_0, eps_0 = ([torch.empty(counts[k], nfs[k], device=dev) for k in range(K)] for _ in range(4))
            arr = _capi.ptr_array
            pos_only = 1 if ls.pos_only else 0
            _capi.check(L.oard_loss_eval_prepare(C.byref(cfg), topo.handle, arr(pos), arr(one_hot), arr(charge), arr(noise[0]), arr(noise[1]),
                                                 t_int.data_ptr(), gamma.data_ptr(), ls.T, nv, nb, pos_only,
                                                 sum(1 << int(k) for k in ls.fixed_idx), arr(z_t), arr(eps_t), arr(z_0), arr(eps_0), stream),
                        "oard_loss_eval_prepare")
            net_t = self._infer(dyn, cfg, topo, packed, z_t, (t_int / ls.T).view(B, 1), cond, stream)
            net_0 = self._infer(dyn, cfg, topo, packed, z_0, torch.zeros(B, 1, device=dev), cond, stream)
            nll = torch.empty(B, device=dev)
            terms = torch.empty(5 * K + 2, B, device=dev)
            delta_log_px = -((sum(counts) - 1) * ls.pos_dim) * math.log(ls.norm_values[0])      # loss.py:153, from the host sizes
            _capi.check(L.oard_loss_eval_terms(C.byref(cfg), topo.handle, arr(eps_t), arr(net_t), arr(eps_0), arr(net_0), arr(z_0),
                                               arr(one_hot), arr(charge), t_int.data_ptr(), gamma.data_ptr(), snr.data_ptr(), ls.T, nv, nb,
                                               sc, pos_only, float(delta_log_px), B, nll.data_ptr(), terms.data_ptr(), stream),
                        "oard_loss_eval_terms")
        return nll, terms

    def _eval_tables(self, dev) -> Tuple[Tensor, Tensor]:
        """The gamma table and the SNR_weight table of `oard_loss_eval_terms` on the device, uploaded once."""
        if self._gamma_dev is None or self._gamma_dev.device != dev:
            self._gamma_dev = self.loss.schedule.gamma.to(device=dev, dtype=torch.float32).contiguous()
        if self._snr_dev is None or self._snr_dev.device != dev:
            self._snr_dev = vlb_snr_table(self.loss.schedule).to(dev)
        return self._gamma_dev, self._snr_dev

    @torch.no_grad()
    def validation_step(self, batch, weights: str = "live", prefix: str = "val", rmsd: bool = False, **kw) -> Tensor:
        """`DDPMModule.validation_step` (`_shared_eval`, pl_trainer.py:349-382) without a host read: -> the device row
        [totloss, error_t_0 .., unorm_error_t_0 .., rmsd, rmsd-median], totloss = nll.mean() of `eval_loss(batch, weights, **kw)` and
        the `info` means as pl_trainer.py:265-269 (error_t_k: the mean of the normalised, scaled error / (scales[k] + 1e-4)).
        `rmsd=True` runs `eval_inpaint_batch(batch, weights=weights)` (that call reads the host); otherwise both RMSD entries are NaN,
        as the reference logs on the epochs it does not sample.  The row and the per-reaction nll are remembered under `prefix` for
        `validation_epoch_end`.  Same API on a trainer that cannot fuse (see `eval_loss`).  `kw`: t_int=, draw= (tests)."""
        nll, terms = self.eval_loss(batch, weights=weights, **kw)
        K = (int(terms.shape[0]) - 2) // 5
        means = terms[: 2 * K].mean(dim=1)
        div = self._val_div.get((means.device, means.dtype))
        if div is None:
            div = self._val_div[(means.device, means.dtype)] = torch.tensor(
                [float(s) + 1e-4 for s in self.loss.scales[:K]] + [1.0] * K, dtype=means.dtype, device=means.device)
        if rmsd:
            tail = torch.tensor(self.eval_inpaint_batch(batch, weights=weights), dtype=means.dtype, device=means.device)
        else:
            tail = torch.full((2,), float("nan"), dtype=means.dtype, device=means.device)
        row = torch.cat([nll.mean().reshape(1).to(means.dtype), means / div, tail])
        kept = self._val_kept.setdefault(prefix, ([], []))
        kept[0].append(row)
        kept[1].append(nll)
        return row

    def test_step(self, batch, weights: str = "live", rmsd: bool = False, **kw) -> Tensor:
        """`DDPMModule.test_step`: `validation_step` logged under the prefix `test`."""
        return self.validation_step(batch, weights=weights, prefix="test", rmsd=rmsd, **kw)

    def validation_epoch_end(self) -> Dict[str, float]:
        """`DDPMModule.validation_epoch_end` (pl_trainer.py:376-382) over the `validation_step` / `test_step` calls since the last one, in
        ONE host read: `<prefix>-<key>` for totloss, error_t_k, unorm_error_t_k, rmsd and rmsd-median, the mean over the batches that
        gave a number (nanmean; the first-batch quirk of the reference's `average_over_batch_metrics` is not reproduced, as in
        `ConfidenceTrainer.validation_epoch_end`), and `<prefix>-pooled-totloss`: the mean nll over ALL remembered reactions, which
        differs from the mean of batch means when the batches are of unequal size.  With collectives on, the sums and counts go through
        one small all-reduce first, so every rank returns the same dict (the reference's `sync_dist=True`); every rank then has to have
        logged under the same prefixes.  Forgets the batches.  No step since the last call: an empty dict."""
        if not self._val_kept:
            return {}
        prefixes = sorted(self._val_kept)
        parts = []
        for p in prefixes:
            rows_list, nlls = self._val_kept[p]
            rows = torch.stack(rows_list).double()
            ok = ~torch.isnan(rows)
            every = torch.cat(nlls).double()
            parts += [torch.where(ok, rows, torch.zeros_like(rows)).sum(dim=0), ok.sum(dim=0).double(), every.sum().reshape(1),
                      torch.full((1,), float(every.numel()), dtype=torch.float64, device=rows.device)]
        width = int(parts[0].numel())
        flat = torch.cat(parts)
        if self.collectives:
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
        per = 2 * width + 2
        flat = flat.view(len(prefixes), per)
        stats = torch.cat([flat[:, :width] / flat[:, width: 2 * width], flat[:, 2 * width: 2 * width + 1] / flat[:, 2 * width + 1:]],
                          dim=1).tolist()                                      # the one host read
        K = (width - 3) // 2
        names = ["totloss"] + [f"error_t_{k}" for k in range(K)] + [f"unorm_error_t_{k}" for k in range(K)] + ["rmsd", "rmsd-median"]
        out: Dict[str, float] = {}
        for p, vals in zip(prefixes, stats):
            out.update({f"{p}-{k}": v for k, v in zip(names, vals)})
            out[f"{p}-pooled-totloss"] = vals[width]
        self._val_kept = {}
        return out

    # ---- the moving average of the weights (trainer/ema.py; see `ema_decay` in __init__) ---------------------------------------------------
    def _need_ema(self) -> Tensor:
        if self.flat_ema is None:
            raise RuntimeError("this trainer keeps no EMA of the weights (DDPMTrainer(ema_decay=...))")
        return self.flat_ema

    def _ema_views(self) -> List[Tensor]:
        """`flat_ema` as one view per trainable tensor (made once: the buffer is only ever written in place)."""
        if self._ema_view_list is None:
            self._ema_view_list = self.layout.views(self.flat_ema)
        return self._ema_view_list

    def _ema_step_generic(self) -> None:
        """The generic step's update, after `optimizer.step()`.  float32 weights on a ROCm device: `oard_ema_update` on views of the flat
        average that copy nothing - ONE call where the weights are one flat buffer too (a fused trainer stepped with `generic=True`), one
        per tensor otherwise (the generic trainer's parameters are not views of one buffer).  Anywhere else (CPU, other dtypes):
        `ModelEmaV2.update`'s expression per tensor as a `mul_` / `add_` pair with the two float32 scalars - the same bits."""
        d = float(np.float32(self.ema_decay))
        w = float(np.float32(1.0 - self.ema_decay))
        ema = self.flat_ema
        with torch.no_grad():
            if ema.is_cuda and ema.dtype == torch.float32:
                L = _capi.lib()
                stream = torch.cuda.current_stream(ema.device).cuda_stream
                pairs = [(ema, self.flat_param)] if self.fused else zip(self._ema_views(), self.params)
                with torch.cuda.device(ema.device):
                    for e, p in pairs:
                        if not p.is_contiguous():
                            raise _capi.OardError("the EMA update needs contiguous parameters")
                        _capi.check(L.oard_ema_update(e.data_ptr(), p.data_ptr(), p.numel(), self.ema_decay, stream), "oard_ema_update")
            else:
                for e, p in zip(self._ema_views(), self.params):
                    e.mul_(d).add_(p.detach() * w)
        if self._ema_dynamics is not None:
            self._ema_dynamics.invalidate_packed()

    def ema_state_dict(self) -> "OrderedDict[str, Tensor]":
        """The module's `state_dict()` with the averaged tensors in place of the trainable ones (copies; buffers and the parameters the
        forward never uses equal their average).  Names and shapes are the reference's: it loads with strict=True into the reference's
        EGNNDynamics or into a fresh one here."""
        ema = self._need_ema()
        where = self.layout.offsets()
        out = OrderedDict()
        for name, t in self.dynamics.state_dict(keep_vars=True).items():
            o = where.get(id(t))
            out[name] = (t.detach() if o is None else ema[o: o + t.numel()].view_as(t)).clone()
        return out

    def copy_ema_to_model(self) -> None:
        """The averaged weights become the model's (EMACallback.on_train_end, ema.py:62-65): one device-to-device copy of the flat buffer,
        or one copy per tensor on the generic path."""
        ema = self._need_ema()
        with torch.no_grad():
            if self.fused:
                self.flat_param.copy_(ema)
            else:
                for e, p in zip(self._ema_views(), self.params):
                    p.copy_(e)
        if hasattr(self.dynamics, "invalidate_packed"):
            self.dynamics.invalidate_packed()

    @property
    def ema_dynamics(self) -> nn.Module:
        """A second module of the live one's class and configuration whose trainable parameters are VIEWS into `flat_ema`; every other
        tensor (buffers, the parameters the forward never uses) shares storage with the live module's.  Built at the first look from the
        live module's constructor arguments; its per-call buffers and its packed weights are its own and appear at its first call, so
        nothing is allocated for a run that never samples from the average.  Hand it to `DiffusionSampler`, `inpaint` or
        `compute_loss(weights="ema")` while training continues: no copy is made, the live weights and their packed blob are not touched,
        and every taken step marks its packed weights stale, so that its next call repacks them.  requires_grad is False throughout;
        `edge_precision` and `nan_check` are the live module's at the time it is built.
        Like any module it serves one stream at a time, and `flat_ema` is written on the stream the training step runs on: a caller
        on another stream orders itself behind the step (`stream.wait_stream(...)`) before it calls the shadow."""
        if self._ema_dynamics is None:
            ema = self._need_ema()
            live = self.dynamics
            args = getattr(live, "_ctor_args", None)
            if args is None:
                raise RuntimeError("ema_dynamics needs a module that keeps its constructor arguments (oareactdiff_amd.EGNNDynamics)")
            args = dict(args, model_config=dict(args["model_config"]), device=torch.device("meta"))     # nothing allocated: every tensor is replaced
            shadow = type(live)(**args)
            shadow.device = live.device
            shadow._ordered_tensors()                  # resolves the (owning module, attribute) pair of every state-dict entry
            bind_to_average(shadow._slots[1], live._ordered_tensors(), ema, self.layout.offsets())
            shadow.edge_precision, shadow.train_edge_precision = live.edge_precision, live.train_edge_precision
            shadow.nan_check, shadow.edge_list_path = live.nan_check, live.edge_list_path
            shadow.eval()
            self._ema_dynamics = shadow
        return self._ema_dynamics

    def sync_replicas(self, check: bool = True) -> None:
        """What torch DDP does when it wraps a module (Lightning `DDPStrategy`, train_ts1x.py:197-203): rank 0's parameters
        and buffers are broadcast to every rank, so replicas built from different RNG states - or with a checkpoint loaded
        on rank 0 only - start identical.  One flat broadcast for the parameters, one for the floating-point buffers."""
        if not self.collectives:
            return
        with torch.no_grad():
            for tensors in (list(self.dynamics.parameters()),
                            [b for b in self.dynamics.buffers() if b.is_floating_point()]):
                uniq, seen = [], set()
                for t in tensors:                          # shared encoders appear once
                    if id(t) not in seen:
                        seen.add(id(t))
                        uniq.append(t)
                if not uniq:
                    continue
                flat = torch.cat([t.reshape(-1).to(torch.float64 if t.dtype == torch.float64 else torch.float32) for t in uniq])
                dist.broadcast(flat, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0, group=self.group)
                for t, received in zip(uniq, FlatLayout(uniq).views(flat)):
                    t.copy_(received)                      # in place: bumps the version -> weights are repacked
                if check:                                  # cheap invariant: every rank now holds the same bytes
                    cs = flat.double().abs().sum().reshape(1)
                    lo, hi = cs.clone(), cs.clone()
                    dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=self.group)
                    dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=self.group)
                    assert float(lo) == float(hi), "replicas differ after the initial broadcast"
            if self.flat_ema is not None:                  # the average travels with the weights (at construction it does not exist yet:
                src = dist.get_global_rank(self.group, 0) if self.group is not None else 0      # it is then copied from the synchronised ones)
                dist.broadcast(self.flat_ema, src=src, group=self.group)
                if self._ema_dynamics is not None:
                    self._ema_dynamics.invalidate_packed()
                if check:
                    cs = self.flat_ema.double().abs().sum().reshape(1)
                    lo, hi = cs.clone(), cs.clone()
                    dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=self.group)
                    dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=self.group)
                    assert float(lo) == float(hi), "EMA buffers differ after the broadcast"

    def all_reduce_gradients(self) -> None:
        """DDP's gradient averaging as one collective over the flat bucket (sum, then / world).  The last element of the
        bucket is the step's non-finite flag: summed with the gradients, > 0 on every rank if any rank raised it."""
        if self.collectives:
            ev = None
            if self.time_collectives and self._bucket.is_cuda:      # bench.py: the collective's own device time, events on the step's stream
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            dist.all_reduce(self._bucket, op=dist.ReduceOp.SUM, group=self.group)
            if ev is not None:
                ev[1].record()
                self._collective_events.append(ev)
            if self.world > 1:
                self.flat_grad.div_(self.world)

    def collective_report(self, reset: bool = True) -> Dict[str, float]:
        """Mean device time of the gradient all-reduce over the steps since the last report (`time_collectives = True`; synchronises)."""
        ms = []
        for a, b in self._collective_events:
            b.synchronize()
            ms.append(a.elapsed_time(b))
        if reset:
            self._collective_events = []
        return {"all_reduce_calls": len(ms), "all_reduce_ms_mean": sum(ms) / len(ms) if ms else None,
                "all_reduce_ms_max": max(ms) if ms else None, "all_reduce_bytes": int(self._bucket.numel() * self._bucket.element_size())}

    def clip_gradients(self, grad_norm: Optional[float] = None) -> Tuple[float, float]:
        """pl_trainer.py:391-418: allow 150 % of the recent mean norm + 3 standard deviations."""
        # get_grad_norm (training_tools.py:29-55): 2-norm of the per-parameter 2-norms == 2-norm of the flat bucket
        if grad_norm is None:
            grad_norm = float(torch.linalg.vector_norm(self.flat_grad, 2.0))
        gscale, max_grad_norm = clip_decision(self.gradnorm_queue, grad_norm, *self.CLIP_FACTORS)
        if math.isfinite(grad_norm) and grad_norm > max_grad_norm:      # (a non-finite norm: nothing scaled, nothing remembered)
            self.flat_grad.mul_(gscale)                # clip_grad_norm_: g *= max_norm / (norm + 1e-6)
        return grad_norm, max_grad_norm

    # ---- what the fused step and the fused evaluation hand to the loss kernels --------------------------------------------------------
    def _loss_operands(self, reps):
        """-> (pos, one_hot, charge: contiguous float32 / int64 / int64 per object; norm_values[3], norm_biases[3], scales[K] as C arrays)."""
        ls, K = self.loss, len(reps)
        pos = [r["pos"].detach().to(torch.float32).contiguous() for r in reps]
        one_hot = [r["one_hot"].detach().to(torch.int64).contiguous() for r in reps]
        charge = [r["charge"].detach().to(torch.int64).contiguous() for r in reps]
        f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])              # noqa: E731
        return pos, one_hot, charge, f3(ls.norm_values), f3(ls.norm_biases), (C.c_float * K)(*[float(x) for x in ls.scales[:K]])

    @staticmethod
    def _noise_blocks(counts: List[int], nfs: List[int], draw, blocks: int, dev) -> List[List[Tensor]]:
        """`blocks` sets of raw N(0,1) draws, each one [n_k, nf_k] tensor per object.  Injected draws (`draw`) follow DiffusionLoss's
        protocol, block after block (per object: randn(n, 3) then randn(n, nf - 3)); the default is ONE device randn for all of it,
        viewed per block and object (same distribution, one launch)."""
        if draw is not None:
            return [[torch.cat([draw((c, 3)).float(), draw((c, f - 3)).float()], dim=1).contiguous() for c, f in zip(counts, nfs)]
                    for _ in range(blocks)]
        flat = torch.randn(blocks * sum(c * f for c, f in zip(counts, nfs)), device=dev)
        out, off = [], 0
        for _ in range(blocks):
            block = []
            for c, f in zip(counts, nfs):
                block.append(flat[off: off + c * f].view(c, f))
                off += c * f
            out.append(block)
        return out

    # ---- fused step (HIP module): no autograd graph, ~20 launches around the network call ----------------------------------------
    def _fused_part(self, cfg, packed, reps, cond, t_int: Tensor, noise: List[Tensor], counts: List[int], host_masks, host_sizes,
                    terms: Tensor, col0: int, buffers: Optional[_CallBuffers] = None):
        """One (micro-)batch on the CURRENT stream: oard_loss_prepare -> oard_forward_train -> oard_loss_terms.  `terms` [2K, B_total]: the
        step's logged terms; this part owns columns [col0, col0 + B) (oard_loss_terms takes B_total both as the row stride of `terms` and
        as the 1 / B of the mean nll).  `buffers`: the per-call buffers of the network call (None: the module's own).
        -> (nll [B], d(mean nll)/d(net), TrainState)."""
        dyn, ls = self.dynamics, self.loss
        dev = self.flat_grad.device
        K = len(reps)
        L = _capi.lib()
        # the layout: from the batch's HOST copies of mask / size when the loader kept them (to_device) - no device -> host copy, i.e. no
        # wait for the work queued on the stream; otherwise from the device tensors.  No edge list either way (the kernels walk the
        # implicit complete graph; a caller-supplied edge_index only exists on dynamics.forward's path, where it is verified).
        combined_mask, _, n_frag_switch = ls._layout(host_masks, host_sizes, need_edges=False)
        B = int(t_int.numel())
        stream = torch.cuda.current_stream(dev).cuda_stream
        topo = dyn._get_train_topology(cfg, None, n_frag_switch, combined_mask, stream, device=dev)
        nfs = list(dyn.node_nfs)
        gamma = self._gamma_dev
        if gamma is None or gamma.device != dev:
            gamma = self._gamma_dev = ls.schedule.gamma.to(device=dev, dtype=torch.float32).contiguous()
        pos, one_hot, charge, nv, nb, sc = self._loss_operands(reps)
        z = [torch.empty(counts[k], nfs[k], device=dev) for k in range(K)]
        eps = [torch.empty_like(x) for x in z]
        arr = _capi.ptr_array
        fixed_mask = sum(1 << int(k) for k in ls.fixed_idx)
        _capi.check(L.oard_loss_prepare(C.byref(cfg), topo.handle, arr(pos), arr(one_hot), arr(charge), arr(noise), t_int.data_ptr(),
                                        gamma.data_ptr(), ls.T, nv, nb, 1 if ls.pos_only else 0, fixed_mask, arr(z), arr(eps), stream),
                    "oard_loss_prepare")
        t = (t_int / ls.T).view(B, 1)
        xs, tt, t_scalar, cnd = dyn._inputs(topo, z, t, cond, dev, detach=True)
        net, state = dyn._run_forward_train(cfg, topo, packed, xs, tt, t_scalar, cnd, stream, reuse_tape=True, buffers=buffers)
        nll = torch.empty(B, device=dev)
        dnet = [torch.empty_like(o) for o in net]
        B_total = int(terms.shape[1])
        _capi.check(L.oard_loss_terms(C.byref(cfg), topo.handle, arr(eps), arr(net), arr(z), arr(one_hot), arr(charge), t_int.data_ptr(),
                                      gamma.data_ptr(), ls.T, nv, nb, sc, 1 if ls.pos_only else 0, B_total, nll.data_ptr(),
                                      terms.data_ptr() + 4 * col0, arr(dnet), stream), "oard_loss_terms")
        state.keep_inputs = (pos, one_hot, charge, z, eps, net, t_int, noise)      # the launches above are asynchronous
        return nll, dnet, state

    def _second_slot(self, dev):
        """State of the second micro-batch: the library's idle sub-batch stream (no fifth stream in the process: the runtime serves a
        process's streams from 4 hardware queues), a gradient buffer with the bucket's layout, and per-call buffers of its own (workspace,
        tape, sweep scratch, NaN flag: the module's set serves the first half)."""
        if self._mb is None or self._mb["device"] != dev:
            h = C.c_void_p()
            with torch.cuda.device(dev):
                _capi.check(_capi.lib().oard_library_stream(1, C.byref(h)), "oard_library_stream")
            grad2 = torch.zeros_like(self.flat_grad)
            self._mb = {"device": dev, "stream": torch.cuda.ExternalStream(h.value, device=dev), "grad": grad2,
                        "dests": self.layout.dests(grad2), "buffers": _CallBuffers()}
        return self._mb

    def _fused_forward_backward(self, batch, t_int: Optional[Tensor] = None, draw=None):
        """loss terms + gradients into the bucket: oard_loss_prepare -> oard_forward_train -> oard_loss_terms -> the backward sweep
        (training.Sweep) fed with the closed-form d(mean nll)/d(net).  Returns (nll [B], terms [2K, B]) on the device.
        Injected draws (`draw`) follow DiffusionLoss's protocol (per object: randn(n, 3) then randn(n, nf - 3)); the default is ONE
        device randn for the whole step's noise (same distribution, one launch instead of nine)."""
        reps, cond = batch
        dyn, ls = self.dynamics, self.loss
        dev = self.flat_grad.device
        K = len(reps)
        L = _capi.lib()
        masks, sizes = [r["mask"] for r in reps], [r["size"] for r in reps]
        have_host = all("mask_host" in r and "size_host" in r for r in reps)
        B = int(sizes[0].numel())
        with torch.cuda.device(dev), torch.no_grad():
            main = torch.cuda.current_stream(dev)
            cfg = dyn._config()
            _capi.check(L.oard_supported(C.byref(cfg)), "oard_supported (hidden_channels/num_radial not built)")
            packed = dyn._get_packed(cfg, main.cuda_stream)
            nfs = list(dyn.node_nfs)
            if t_int is None:
                t_int = torch.randint(0, ls.T + 1, size=(B, 1), device=dev).float()
            t_int = t_int.detach().to(device=dev, dtype=torch.float32).reshape(B).contiguous()
            counts = [int(m.numel()) for m in masks]
            noise = self._noise_blocks(counts, nfs, draw, 1, dev)[0]
            dests = {id(p): p.grad for p in self.params}
            terms = torch.empty(2 * K, B, device=dev)
            if self.microbatches == 2 and have_host and B >= 2:
                return self._fused_two(cfg, packed, reps, cond, t_int, noise, B, dests, main, terms)
            hm = [r["mask_host"] for r in reps] if have_host else masks
            hs = [r["size_host"] for r in reps] if have_host else sizes
            nll, dnet, state = self._fused_part(cfg, packed, reps, cond, t_int, noise, counts, hm, hs, terms, 0)
            training.backward_sweep(dyn, state, dnet, main.cuda_stream, dests)
        return nll, terms

    def _fused_two(self, cfg, packed, reps, cond, t_int, noise, B: int, dests, main, terms):
        """The step as two micro-batches (reactions [0, h) and [h, B)) on two streams; see `microbatches` in __init__."""
        dyn = self.dynamics
        dev = self.flat_grad.device
        mb = self._second_slot(dev)
        side, buf1 = mb["stream"], mb["buffers"]
        K = len(reps)
        h = B // 2
        n0 = [int(r["size_host"][:h].sum()) for r in reps]                 # rows of the first half per object (host arithmetic)
        halves = []
        for lo, hi, first in ((0, h, True), (h, B, False)):
            rp, hm, hs, cn = [], [], [], []
            for k, r in enumerate(reps):
                a, b = (0, n0[k]) if first else (n0[k], int(r["mask_host"].numel()))
                rp.append({"pos": r["pos"][a:b], "one_hot": r["one_hot"][a:b], "charge": r["charge"][a:b]})
                hm.append(r["mask_host"][a:b] - lo)
                hs.append(r["size_host"][lo:hi])
                cn.append(b - a)
            nz = [x[(0 if first else n0[k]): (n0[k] if first else x.shape[0])] for k, x in enumerate(noise)]
            cd = cond[lo:hi] if isinstance(cond, Tensor) else cond
            halves.append((rp, cd, t_int[lo:hi], nz, cn, hm, hs, terms, lo))
        dyn._get_packed_bwd(cfg, main.cuda_stream)             # both packs on the caller's stream BEFORE the fork (the second half reads them)
        mb["grad"].zero_()
        buf1.reset()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            nll1, dnet1, st1 = self._fused_part(cfg, packed, *halves[1], buffers=buf1)
        nll0, dnet0, st0 = self._fused_part(cfg, packed, *halves[0])
        with torch.cuda.stream(side):
            sw1 = training.Sweep(dyn, st1, dnet1, side.cuda_stream, mb["dests"], buf1)
        sw0 = training.Sweep(dyn, st0, dnet0, main.cuda_stream, dests)
        # the two sweeps step by step: the library's gradient stream then sees their weight-gradient work alternately
        steps = [("tail",)] + [("layer", l) for l in reversed(range(sw0.NL))] + [("init",)]
        for st in steps:
            with torch.cuda.stream(side):
                getattr(sw1, st[0])(*st[1:])
            getattr(sw0, st[0])(*st[1:])
        main.wait_stream(side)
        self.flat_grad.add_(mb["grad"])
        if buf1.nan_seen is not None and dyn.nan_seen is not None:
            dyn.nan_seen.bitwise_or_(buf1.nan_seen)       # the second half's flag reaches the module's, which the step reads
        return torch.cat([nll0, nll1]), terms

    def _weight_readers(self):
        return self.dynamics, self._ema_dynamics

    def _fused_step(self, batch, **kw) -> Dict[str, float]:
        dyn = self.dynamics
        prev = dyn.nan_check
        dyn.nan_check = "async"
        dyn.reset_nan_seen()
        self._bucket.zero_()
        try:
            nll, terms = self._fused_forward_backward(batch, **kw)
        finally:
            dyn.nan_check = prev
        K = terms.shape[0] // 2
        means = torch.cat([nll.unsqueeze(0), terms]).mean(dim=1)                  # loss, err_n[k], err_t[k]
        # non-finite anywhere (loss, local gradient, the network's device-side flag) -> the bucket's last element, summed by the all-reduce
        norm = torch.linalg.vector_norm(self.flat_grad, 2.0)
        bad = (~torch.isfinite(norm + means[0])).to(torch.float32)
        if dyn.nan_seen is not None:
            bad = bad + (dyn.nan_seen[0] != 0).to(torch.float32)
        self._bucket[-1] = bad
        if self.collectives:
            self.all_reduce_gradients()
            norm = torch.linalg.vector_norm(self.flat_grad, 2.0)
        if not self.host_sync:
            # no host read: one device thread takes the clip / skip decision, AdamW reads its scalars from device memory
            stats_dev = torch.cat([norm.reshape(1), self._bucket[-1:], means])
            state = self._clip_state if self._clip_state is not None else self._push_clip_state()
            out4 = torch.empty(4, dtype=torch.float32, device=stats_dev.device)
            # the two launches; with an average, the AdamW kernel updates it (not at all if the step is skipped)
            self._adamw("oard_adamw_step_dev", (), (1 if self.clip_grad else 0, state.data_ptr(), self.CLIP_CAPACITY, stats_dev.data_ptr(),
                                                    stats_dev.data_ptr() + 4, out4.data_ptr()))
            return LazyInfo(stats_dev, out4, K, [float(x) for x in self.loss.scales], self.clip_grad)
        if self._clip_state is not None:               # host_sync was switched on again: the host copies become the truth
            self._pull_clip_state()
            self._clip_state = None
        stats = torch.cat([norm.reshape(1), self._bucket[-1:], means]).tolist()        # the one host sync
        grad_norm, flag = stats[0], stats[1]
        info: Dict[str, float] = {}
        for k in range(K):
            info[f"error_t_{k}"] = stats[3 + k] / (self.loss.scales[k] + 1e-4)
            info[f"unorm_error_t_{k}"] = stats[3 + K + k]
        skipped = flag != 0 or not math.isfinite(grad_norm)
        gscale = 1.0
        if skipped:
            self._count_skip(info, grad_norm)
        else:
            if self.clip_grad:                        # pl_trainer.py:391-418, with the factor folded into the optimiser kernel
                gscale, max_norm = clip_decision(self.gradnorm_queue, grad_norm, *self.CLIP_FACTORS)
                info["grad_norm"], info["max_grad_norm"] = grad_norm, max_norm
            self.opt_step += 1
            self._adamw("oard_adamw_step", (self.opt_step,), (float(gscale),))
        info["loss"] = stats[2]
        info["skipped"] = int(skipped)
        return info

    def training_step(self, batch, **kw) -> Dict[str, float]:
        """`kw` (t_int=, draw=) injects the step's randomness for tests; by default it is drawn like the reference does.
        With the HIP module on a ROCm device and the l2 loss this is the fused step (`_fused_step`: no autograd graph, the loss
        terms, their gradient and AdamW as HIP kernels); otherwise the generic autograd formulation below.

        Non-finite values (the reference replaces a NaN network output by randn and trains on, egnn_dynamics.py:138-143 - every
        DDP rank in lock-step): here the network's device-side NaN flag and the finiteness of the local loss / gradient travel
        in the gradient bucket's last element through the SAME all-reduce; if any rank raised it, every rank skips the
        optimiser step (weights, AdamW state and the clipping history untouched), counts it in `skipped_steps` and reports
        `info["skipped"] = 1`.  No rank leaves the step before the collective, and the only host sync is the one read of
        [gradient norm, flag, loss] after it."""
        if self.fused and not kw.get("generic", False):
            return self._fused_step(batch, **{k: v for k, v in kw.items() if k != "generic"})
        kw.pop("generic", None)
        dyn = self.dynamics
        prev = getattr(dyn, "nan_check", None)
        if prev is not None:
            dyn.nan_check = "async"                    # no host sync between forward and backward; the flag is read below
            if hasattr(dyn, "reset_nan_seen"):
                dyn.reset_nan_seen()
        self._bucket.zero_()
        try:
            nll, info = self.compute_loss(batch, training=True, lazy_info=True, **kw)   # logged means stay on the device until the end
            loss = nll.mean(0)                         # pl_trainer.py:329
            loss.backward()
        finally:
            if prev is not None:
                dyn.nan_check = prev
        bad = (~torch.isfinite(loss.detach())).to(self._bucket.dtype).reshape(())
        seen = getattr(dyn, "nan_seen", None)
        if seen is not None:
            bad = bad + (seen[0] != 0).to(self._bucket.dtype)
        # a non-finite local gradient must not reach the sum as NaN only (the flag element would survive, but be explicit)
        self._bucket[-1] = bad + (~torch.isfinite(self.flat_grad.sum())).to(self._bucket.dtype)
        self.all_reduce_gradients()
        stats = torch.stack([torch.linalg.vector_norm(self.flat_grad, 2.0).to(torch.float64), self._bucket[-1].to(torch.float64),
                             loss.detach().to(torch.float64)]).tolist()            # the step's one host sync
        grad_norm, flag, loss_value = stats
        skipped = flag != 0 or not math.isfinite(grad_norm)
        if skipped:
            self._count_skip(info, grad_norm)
        else:
            if self.clip_grad:
                info["grad_norm"], info["max_grad_norm"] = self.clip_gradients(grad_norm)
            self.optimizer.step()
            if self.flat_ema is not None:
                self._ema_step_generic()
        info["loss"] = loss_value
        info["skipped"] = int(skipped)
        return {k: (float(v) if isinstance(v, Tensor) else v) for k, v in info.items()}

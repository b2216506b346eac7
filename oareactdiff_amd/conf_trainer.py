"""One training step of the confidence model around the HIP `Confidence` module.

`ConfidenceTrainer.training_step` mirrors `ConfModule.training_step` + `compute_loss` + `configure_optimizers` +
`configure_gradient_clipping` (oa_reactdiff/trainer/pl_trainer.py:421-669, driven by trainer/train_confidence_ts1x.py):

    preds = confidence.forward(representations, conditions)          pl_trainer.py:559-562
    loss  = BCELoss(sigmoid(preds), target.float())                  :564-565, 584   (classification)
          | MSELoss(preds, target.float())                           :584            (regression)
    loss.backward()                                                  HIP: oard_confidence_tail_backward + the denoiser's sweep
    adaptive gradient clipping, 2.5 mean + 3 std of the norm history :642-669        (the denoiser's trainer uses 1.5)
    AdamW step                                                       :488-499

The step builds no autograd graph: the training-mode forward (`oard_confidence_forward_train`), the closed-form cotangent of the loss,
(sigmoid(x) - y) / B or 2 (x - y) / B - a few element-wise torch ops on [B] -, the reverse sweep straight into ONE flat gradient bucket and
`oard_adamw_step` on ONE flat parameter buffer, as in `DDPMTrainer`'s fused step.  One host read per step: [gradient norm, non-finite
flag, loss, logged metrics].

Logged (`info`): classification `acc`, `precision`, `F1` at threshold 0.5 and `mean` (the share of predictions that round to 1);
regression `MAE` and `mean` - torch ops on the device.  The reference also logs `AUC` (classification), `Pearson` and `Spearman`
(regression) through torchmetrics (pl_trainer.py:568, 579, 581), which this package does not depend on: `ConfidenceTrainer(...,
rank_metrics=True)` adds them under the reference's names from `metrics.rank_metrics` (`oard_rank_metrics`, csrc/oard_rank.h) - AUC of the
float32 `sigmoid(preds)` the reference feeds to torchmetrics, positives `target >= 0.5`, ties counted half.  They travel in the same host
read, which is float64 on that path.  Off by default: the logged keys and every bit of a step are then what they were without it.

VALIDATION: `validation_step(batch)` is `_shared_eval` (pl_trainer.py:619-629) without a host read - an inference-mode forward on the
live weights or on the average, the row [totloss, metrics...] on the device, predictions and targets remembered on the device -, and
`validation_epoch_end()` is `average_over_batch_metrics` (trainer/_metrics.py:6-22) in ONE host read, plus the pooled AUC / Pearson /
Spearman over every remembered prediction as one segment: a mean of per-batch AUCs is not the AUC of the set.

Host-sync step on one device only: no `host_sync=False`, no micro-batches, no process group (out of scope).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import _capi
from .confidence import FEATURE_MAPPING, Confidence, _Layout
from .graph_tools import get_n_frag_switch
from .metrics import rank_metrics
from .flat_state import FlatTrainerState, bind_to_average, clip_decision

DEFAULT_OPTIMIZER = dict(lr=5e-4, betas=(0.9, 0.999), weight_decay=0, amsgrad=True)       # train_confidence_ts1x.py:82-87
CLIP_MEAN_FACTOR, CLIP_STD_FACTOR = 2.5, 3.0                                                # pl_trainer.py:649


class ConfidenceTrainer(FlatTrainerState):
    SKIP_MESSAGE = "Warning: non-finite loss / gradient / network output: step skipped ({} so far)"

    def __init__(self, confidence: Confidence, optimizer_config: Optional[Dict] = None, clip_grad: bool = True,
                 classification: bool = True, target_key: str = "rmsd", ema_decay: Optional[float] = None, rank_metrics: bool = False):
        """`confidence`: a `Confidence(..., trainable=True)` on a ROCm device.  A batch is `(representations, res)` with
        `res["condition"]` and the targets `res[target_key]` ([B], by reaction id), as `ConfModule.compute_loss` takes it.
        `ema_decay=d`: a float32 moving average of the trained weights in `flat_ema`, updated inside the AdamW kernel after every step
        that is taken (`oard_adamw_step_ema`; `d` is the weight of the old average, as in `DDPMTrainer`).
        `rank_metrics=True`: `AUC` (classification) or `Pearson` and `Spearman` (regression) join the logged metrics (module docstring)."""
        if not isinstance(confidence, Confidence) or not confidence.trainable:
            raise ValueError("ConfidenceTrainer needs a Confidence module built with trainable=True")
        self.confidence = confidence
        self.classification, self.target_key = bool(classification), target_key
        self.rank_metrics = bool(rank_metrics)
        P = confidence._train_params()
        self.names: List[str] = list(P)
        self.params: List[Tensor] = list(P.values())
        dev = self.params[0].device
        if dev.type != "cuda" or any(p.dtype != torch.float32 or p.device != dev for p in self.params):
            raise ValueError("ConfidenceTrainer needs float32 parameters on one ROCm device")
        self.n_params = sum(p.numel() for p in self.params)
        # the parameters the confidence forward uses become views of ONE flat buffer, their gradients views of ONE flat bucket; the
        # tensors the forward never uses (confidence.CONF_UNUSED_PREFIXES) stay outside: no gradient, no weight decay, no step.
        # Every view starts on a 16-byte boundary - the readout kernels read the weight rows four floats at a time -; the up to three
        # floats in front of it are zero in every buffer and stay zero (AdamW of a zero weight under a zero gradient)
        self._lay_out(4, ema_decay, bool(clip_grad))
        n = self.layout.size
        self._bind(torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev))
        confidence.grad_inplace = True                         # compute_loss(...)[0].backward() lands in the bucket as well
        self._dests = {id(p): p.grad for p in self.params}
        self._ema_confidence: Optional[Confidence] = None
        # validation: rows [totloss, metrics...] of the batches seen, their predictions / targets in grow-only device buffers
        self._val_rows: List[Tensor] = []
        self._val_names: List[str] = []
        self._val_pred: Optional[Tensor] = None
        self._val_target: Optional[Tensor] = None
        self._val_n = 0
        self.opt_config = dict(DEFAULT_OPTIMIZER, **(optimizer_config or {}))
        # what configure_optimizers returns (pl_trainer.py:488-499): its param_groups[0] is read at EVERY step, so a scheduler attached
        # to it takes effect; the moments live in the flat buffers here (state_dict)
        self.optimizer = torch.optim.AdamW(self.params, **self.opt_config)

    # ---- resume: `state_dict()` / `load_state_dict()` are FlatTrainerState's ----------------------------------------------------------

    # ---- loss -----------------------------------------------------------------------------------------------------------------------
    def _targets(self, res, dev) -> Tensor:
        return res[self.target_key].detach().to(device=dev, dtype=torch.float32).reshape(-1)

    def _ranked(self, names: List[str], vals: Tensor, pred: Tensor, y: Tensor) -> Tuple[List[str], Tensor]:
        """The logged metrics with the ranking ones behind them (`rank_metrics=True`): one kernel call on the batch as one segment."""
        if not self.rank_metrics:
            return names, vals
        m = rank_metrics(pred, y)
        if self.classification:
            return names + ["AUC"], torch.cat([vals.double(), m.auroc])
        return names + ["Pearson", "Spearman"], torch.cat([vals.double(), m.pearson, m.spearman])

    def _loss_and_metrics(self, logits: Tensor, y: Tensor) -> Tuple[Tensor, List[str], Tensor, Tensor]:
        """-> (loss, metric names, metric values [len(names)], the predictions they are computed on: sigmoid(preds) or preds) on the
        device; pl_trainer.py:564-584.  The values are float32, or float64 with `rank_metrics`."""
        x = logits.reshape(-1)
        if self.classification:
            p = torch.sigmoid(x)
            # nn.BCELoss's expression (log terms clamped at -100) from element-wise ops: torch's own BCE kernel asserts 0 <= p <= 1 on
            # the device, which a NaN prediction fails - and the step has to SKIP on a NaN, not abort the process
            loss = -(y * torch.log(p).clamp(min=-100.0) + (1.0 - y) * torch.log(1.0 - p).clamp(min=-100.0)).mean()
            hit, pos = p >= 0.5, y >= 0.5
            tp = (hit & pos).sum().float()
            fp, fn = (hit & ~pos).sum().float(), (~hit & pos).sum().float()
            zero = torch.zeros((), device=x.device)
            prec = torch.where(tp + fp > 0, tp / (tp + fp).clamp(min=1), zero)              # torchmetrics: 0 where undefined
            f1 = torch.where(2 * tp + fp + fn > 0, 2 * tp / (2 * tp + fp + fn).clamp(min=1), zero)
            names, vals = self._ranked(["acc", "precision", "F1", "mean"],
                                       torch.stack([(hit == pos).float().mean(), prec, f1, p.round().mean()]), p, y)
            return loss, names, vals, p
        loss = torch.nn.functional.mse_loss(x, y)
        names, vals = self._ranked(["MAE", "mean"], torch.stack([(x - y).abs().mean(), x.mean()]), x, y)
        return loss, names, vals, x

    def compute_loss(self, batch) -> Tuple[Tensor, Dict[str, float]]:
        """`ConfModule.compute_loss` (pl_trainer.py:554-585) -> (loss, info).  Under autograd the loss carries the module's
        `ConfidenceFunction`; the logged metrics cost one host read."""
        representations, res = batch
        logits = self.confidence.forward(representations, res["condition"])
        loss, names, vals, _ = self._loss_and_metrics(logits, self._targets(res, logits.device))
        return loss, dict(zip(names, vals.detach().tolist()))

    # ---- the step -------------------------------------------------------------------------------------------------------------------
    def _forward_backward(self, batch) -> Tuple[Tensor, List[str], Tensor]:
        """Training-mode forward, closed-form cotangent, reverse sweep into the bucket -> (loss, metric names, metric values)."""
        representations, res = batch
        conf = self.confidence
        dev = self.flat_grad.device
        L = _capi.lib()
        masks, sizes = [r["mask"] for r in representations], [r["size"] for r in representations]

        def build():          # no edge list: the kernels walk the implicit complete graph, and there is no caller's list to verify
            return _Layout(torch.cat(masks).to(dev), None, get_n_frag_switch([s.to(dev) for s in sizes]))
        lay = conf._layout_cache.lookup(tuple(masks) + tuple(sizes), (str(dev), "train"), build)
        xh = [torch.cat([r[f] for f in FEATURE_MAPPING], dim=1) for r in representations]
        with torch.cuda.device(dev), torch.no_grad():
            stream = torch.cuda.current_stream(dev).cuda_stream
            cfg = conf._config()
            _capi.check(L.oard_supported(C.byref(cfg)), "oard_supported (hidden_channels/num_radial not built)")
            packed = conf._get_packed(cfg, stream)
            topo = conf._get_train_topology(cfg, None, lay.n_frag_switch, lay.combined_mask, stream)
            conf._check_train_topology(topo)
            xs, tt, t_scalar, cond = conf._inputs(topo, xh, conf._zero_time(dev), res["condition"], dev, detach=True)
            logits, state = conf._run_forward_train_conf(cfg, topo, packed, xs, tt, t_scalar, cond, stream, reuse_tape=True)
            y = self._targets(res, dev)
            if y.numel() != logits.numel():
                raise _capi.OardError(f"{y.numel()} targets for {logits.numel()} reactions")
            loss, names, vals, _ = self._loss_and_metrics(logits, y)
            B = logits.numel()
            dlogits = (torch.sigmoid(logits) - y) / B if self.classification else 2.0 * (logits - y) / B
            conf.backward_sweep(state, dlogits, self._dests, stream)
        return loss, names, vals

    def _weight_readers(self):
        return self.confidence, self._ema_confidence

    def training_step(self, batch) -> Dict[str, float]:
        """One step; -> info: `loss`, `skipped`, the logged metrics of `compute_loss`, and with clipping `grad_norm` / `max_grad_norm`.
        A non-finite loss, gradient or network output skips the step as `DDPMTrainer.training_step` does: weights, moments, step
        count and clipping history untouched, `skipped_steps` counts it, `info["skipped"] = 1`."""
        conf = self.confidence
        conf.reset_nan_seen()
        self.flat_grad.zero_()
        loss, names, vals = self._forward_backward(batch)
        norm = torch.linalg.vector_norm(self.flat_grad, 2.0)
        bad = (~torch.isfinite(norm + loss)).to(torch.float32)
        if conf.nan_seen is not None:
            bad = bad + (conf.nan_seen[0] != 0).to(torch.float32)
        head = [norm.reshape(1), bad.reshape(1), loss.reshape(1)]
        if self.rank_metrics:                                  # the ranking metrics are float64: widen the rest, which is exact
            head = [h.double() for h in head]
        stats = torch.cat(head + [vals]).tolist()              # the one host sync
        grad_norm, flag = stats[0], stats[1]
        info: Dict[str, float] = dict(zip(names, stats[3:]))
        skipped = flag != 0 or not math.isfinite(grad_norm)
        if skipped:
            self._count_skip(info, grad_norm)
        else:
            gscale = 1.0
            if self.clip_grad:                                 # pl_trainer.py:642-669, the factor folded into the optimiser kernel
                gscale, max_norm = clip_decision(self.gradnorm_queue, grad_norm, CLIP_MEAN_FACTOR, CLIP_STD_FACTOR)
                info["grad_norm"], info["max_grad_norm"] = grad_norm, max_norm
            self.opt_step += 1
            self._adamw("oard_adamw_step", (self.opt_step,), (float(gscale),))
        info["loss"] = stats[2]
        info["skipped"] = int(skipped)
        return info

    # ---- validation -----------------------------------------------------------------------------------------------------------------
    @property
    def ema_confidence(self) -> Confidence:
        """A second, frozen `Confidence` of the live one's configuration whose trained tensors are VIEWS into `flat_ema` (every other
        tensor shares storage with the live module's), as `DDPMTrainer.ema_dynamics`: built at the first look, with packed weights
        and call buffers of its own, so a call on the average touches neither the live weights nor their packed blob; every taken step
        marks its packed weights stale."""
        if self._ema_confidence is None:
            if self.flat_ema is None:
                raise ValueError("this trainer keeps no average of the weights (ConfidenceTrainer(ema_decay=...))")
            live = self.confidence
            args = dict(live._ctor_args, model_config=dict(live._ctor_args["model_config"]), device=torch.device("meta"))
            for k in ("update_pocket_coords", "condition_time"):          # fixed by Confidence itself
                args.pop(k, None)
            shadow = Confidence(**args)
            shadow.device = live.device
            shadow._ordered_tensors()                      # resolves the (owning module, attribute) pair of every state-dict entry
            bind_to_average(shadow._slots[1] + shadow._readout_slot_list(),
                            live._ordered_tensors() + live._readout_tensors(self.flat_ema.device), self.flat_ema, self.layout.offsets())
            shadow.edge_precision, shadow.train_edge_precision = live.edge_precision, live.train_edge_precision
            shadow.eval()
            self._ema_confidence = shadow
        return self._ema_confidence

    def _remember(self, pred: Tensor, y: Tensor) -> None:
        n, B = self._val_n, int(pred.numel())
        if self._val_pred is None or self._val_pred.numel() < n + B:
            cap = max(2 * (n + B), 1024)
            grown = [torch.empty(cap, dtype=torch.float32, device=pred.device) for _ in range(2)]
            if n:
                grown[0][:n].copy_(self._val_pred[:n])
                grown[1][:n].copy_(self._val_target[:n])
            self._val_pred, self._val_target = grown
        self._val_pred[n: n + B].copy_(pred)
        self._val_target[n: n + B].copy_(y)
        self._val_n = n + B

    @torch.no_grad()
    def validation_step(self, batch, weights: str = "live") -> Tensor:
        """`ConfModule.validation_step` (`_shared_eval`, pl_trainer.py:619-629) without a host read: an inference-mode forward - no tape,
        no gradient work - on the live weights, or with `weights="ema"` on the average (`ema_confidence`; ValueError for a trainer
        without `ema_decay`), which leaves the live weights and their packed blob alone.  -> the device row [totloss, metrics...] in the
        order of `compute_loss`'s `info` (float64 with `rank_metrics`).  The batch's predictions (sigmoid(preds) or preds) and targets
        are appended to device buffers that only grow, for `validation_epoch_end`."""
        if weights not in ("live", "ema"):
            raise ValueError(f"weights must be 'live' or 'ema' (got {weights!r})")
        conf = self.confidence if weights == "live" else self.ema_confidence
        representations, res = batch
        logits = conf.forward(representations, res["condition"]).reshape(-1)
        y = self._targets(res, logits.device)
        if y.numel() != logits.numel():
            raise _capi.OardError(f"{y.numel()} targets for {logits.numel()} reactions")
        loss, names, vals, pred = self._loss_and_metrics(logits, y)
        row = torch.cat([loss.reshape(1).to(vals.dtype), vals])
        self._remember(pred, y)
        self._val_rows.append(row)
        self._val_names = ["totloss"] + names
        return row

    def validation_epoch_end(self) -> Dict[str, float]:
        """`ConfModule.validation_epoch_end` (pl_trainer.py:634-640) over the `validation_step` calls since the last one, in ONE host
        read: `val-<k>` for `totloss` and every logged metric, the mean over the batches that gave a number (`nanmean`).  The reference's
        `average_over_batch_metrics` (trainer/_metrics.py:6-22) skips NaN batches too - except the first, whose NaN poisons its mean;
        that quirk is not reproduced.  And what a ranking model is judged by: `val-pooled-AUC` (classification) or `val-pooled-Pearson`
        and `val-pooled-Spearman` (regression) over ALL remembered predictions as one segment - not a mean of per-batch numbers.
        Forgets the batches (the buffers stay allocated).  No `validation_step` since the last call: an empty dict."""
        if not self._val_rows:
            return {}
        names = self._val_names
        means = torch.nanmean(torch.stack(self._val_rows).double(), dim=0)
        m = rank_metrics(self._val_pred[:self._val_n], self._val_target[:self._val_n])
        pooled = {"AUC": m.auroc} if self.classification else {"Pearson": m.pearson, "Spearman": m.spearman}
        stats = torch.cat([means] + list(pooled.values())).tolist()          # the one host read
        out = {f"val-{k}": v for k, v in zip(names, stats)}
        out.update({f"val-pooled-{k}": v for k, v in zip(pooled, stats[len(names):])})
        self._val_rows, self._val_n = [], 0
        return out

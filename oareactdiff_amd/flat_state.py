"""What `DDPMTrainer` and `ConfidenceTrainer` own in common: trainable tensors as views of flat buffers (`FlatLayout`), and on top of
them (`FlatTrainerState`) the flat AdamW state, the one caller of the `oard_adamw_step*` entry points, the resumable state that goes
with them, and the host side of the adaptive clipping rule (`clip_decision`).

    flat_param   the weights: `p.data` are views of it, so AdamW is ONE kernel over it            (not in DDPMTrainer's generic mode)
    flat_grad    the gradients: `p.grad` are views of it, so the backward accumulates in place and the norm is one reduction
    exp_avg, exp_avg_sq, max_exp_avg_sq, opt_step       AdamW's moments and step count            (not in the generic mode)
    flat_ema     the moving average of the weights, updated inside the AdamW kernel               (only with `ema_decay`)
All share one layout; the padding an aligned layout leaves is zero in every buffer and stays zero (AdamW of a zero weight, zero gradient)."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from . import _capi


class FlatLayout:
    """Where each of an ordered list of distinct tensors lies in one flat buffer: tensor k at `starts[k]`, every start a multiple of
    `align` elements, `size` elements in all (a multiple of `align` too).  `align=1` packs them back to back."""

    def __init__(self, tensors: Sequence[Tensor], align: int = 1):
        self.tensors = list(tensors)
        self.starts: List[int] = []
        n = 0
        for p in self.tensors:
            self.starts.append(n)
            n = (n + p.numel() + align - 1) // align * align
        self.size = n

    def offsets(self) -> Dict[int, int]:
        """id(tensor) -> start: the `where` of `bind_to_average`."""
        return {id(p): o for p, o in zip(self.tensors, self.starts)}

    def views(self, flat: Tensor) -> List[Tensor]:
        """`flat` as one view per tensor, of that tensor's shape."""
        return [flat[o: o + p.numel()].view_as(p) for p, o in zip(self.tensors, self.starts)]

    def dests(self, flat: Tensor) -> Dict[int, Tensor]:
        """id(tensor) -> its view of `flat`: the gradient destinations of `training.Sweep`."""
        return {id(p): v for p, v in zip(self.tensors, self.views(flat))}


def bind_to_average(slots, tensors, flat_ema: Tensor, where: Dict[int, int]) -> None:
    """Fills a shadow module (`DDPMTrainer.ema_dynamics`, `ConfidenceTrainer.ema_confidence`): slot k, an (owning module, attribute)
    pair of the shadow, receives the live module's `tensors[k]` - as a VIEW into `flat_ema` at offset `where[id(tensor)]` if it is a
    trained tensor, else the live tensor itself (shared storage).  A tensor that sits in several slots stays one object;
    requires_grad is False throughout."""
    made: Dict[int, Tensor] = {}
    for (mod, attr), t in zip(slots, tensors):
        new = made.get(id(t))
        if new is None:
            o = where.get(id(t))
            data = t.detach() if o is None else flat_ema[o: o + t.numel()].view_as(t)
            new = made[id(t)] = nn.Parameter(data, requires_grad=False) if isinstance(t, nn.Parameter) else data
        if attr in mod._parameters:
            mod._parameters[attr] = new
        else:
            mod._buffers[attr] = new


class Queue:
    """oa_reactdiff/utils/training_tools.py:6-23."""

    def __init__(self, max_len: int = 50):
        self.items: List[float] = []
        self.max_len = max_len

    def __len__(self):
        return len(self.items)

    def add(self, item: float) -> None:
        self.items.insert(0, item)
        if len(self) > self.max_len:
            self.items.pop()

    def mean(self) -> float:
        return float(np.mean(self.items))

    def std(self) -> float:
        return float(np.std(self.items))


def clip_decision(queue: Queue, grad_norm: float, mean_factor: float, std_factor: float) -> Tuple[float, float]:
    """The reference's adaptive clipping (pl_trainer.py:391-418, :642-669) as a decision: allow `mean_factor` times the mean of the recent
    norms plus `std_factor` standard deviations -> (the factor the gradient is to be multiplied by, that allowance).  A norm above the
    allowance is scaled as clip_grad_norm_ does, g *= max_norm / (norm + 1e-6), and the allowance is remembered; otherwise the factor is
    1 and the norm is remembered.  A non-finite norm never poisons the history (nan > max is False: clipping would stay off): factor 1,
    nothing remembered."""
    max_norm = mean_factor * queue.mean() + std_factor * queue.std()
    if not math.isfinite(grad_norm):
        return 1.0, max_norm
    if grad_norm > max_norm:
        queue.add(float(max_norm))
        print(f"Clipped gradient with value {grad_norm:.1f} while allowed {max_norm:.1f}")
        return max_norm / (grad_norm + 1e-6), max_norm
    queue.add(grad_norm)
    return 1.0, max_norm


class FlatTrainerState:
    """Base of the two trainers.  A subclass sets `params` / `names` (distinct trainable tensors and their state-dict names) and
    `optimizer` (its `param_groups[0]` holds the hyper-parameters of every step), calls `_lay_out` and then `_bind` with the buffers it
    allocated, and defines `_weight_readers()` -> (the live module, the shadow module on `flat_ema` or None if none was built): the
    modules whose packed weights a step makes stale.  `SKIP_MESSAGE`: what a skipped step prints, with a place for their count."""

    fused = True          # the weights are views of `flat_param` and AdamW runs here (False: DDPMTrainer's generic mode)

    def _lay_out(self, align: int, ema_decay: Optional[float], clip_grad) -> None:
        """The part of construction that allocates nothing on the device: layout, counters, the clipping history (pl_trainer.py:143-146,
        :465-468), `ema_decay` checked."""
        self.layout = FlatLayout(self.params, align)
        self.skipped_steps = 0
        if ema_decay is not None and not 0.0 <= float(ema_decay) <= 1.0:
            raise ValueError(f"ema_decay must lie in [0, 1] (got {ema_decay!r})")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.flat_ema: Optional[Tensor] = None
        self.clip_grad = clip_grad
        if clip_grad:
            self.gradnorm_queue = Queue()
            self.gradnorm_queue.add(3000)

    def _bind(self, flat_grad: Tensor, flat_param: Optional[Tensor] = None) -> None:
        """`p.grad` become views of `flat_grad`.  With `flat_param` (None in the generic mode) the weights are copied into it, `p.data`
        become views of it and AdamW's state is created beside it.  Then the average, if one is kept, starts as a copy of the weights
        (ModelEmaV2.__init__)."""
        self.flat_grad = flat_grad
        for p, g in zip(self.params, self.layout.views(flat_grad)):
            p.grad = g
        if flat_param is not None:
            self.flat_param = flat_param
            with torch.no_grad():
                for p, w in zip(self.params, self.layout.views(flat_param)):
                    w.copy_(p)
                    p.data = w
            self.exp_avg = torch.zeros_like(flat_param)
            self.exp_avg_sq = torch.zeros_like(flat_param)
            self.max_exp_avg_sq = torch.zeros_like(flat_param)
            self.opt_step = 0
        if self.ema_decay is not None:
            self.flat_ema = self._flat_weights()

    def _flat_weights(self) -> Tensor:
        """A fresh flat copy of the trainable weights in the layout's order."""
        if self.fused:
            return self.flat_param.detach().clone()
        return torch.cat([p.detach().reshape(-1) for p in self.params])

    def _adamw(self, entry: str, before, after) -> None:
        """One call of the AdamW entry point `entry` - its `_ema` form when the trainer keeps an average - on the flat buffers with the
        optimiser's hyper-parameters.  `before` / `after`: the entry point's own arguments on either side of `amsgrad`.  The weights
        change behind torch's version counters (unless the device skipped the step: repacking is harmless)."""
        o = self.optimizer.param_groups[0]
        dev = self.flat_grad.device
        args = (self.flat_param.data_ptr(), self.flat_grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                self.max_exp_avg_sq.data_ptr(), self.flat_param.numel(), float(o["lr"]), float(o["betas"][0]), float(o["betas"][1]),
                float(o.get("eps", 1e-8)), float(o.get("weight_decay", 0.0)), *before, 1 if o.get("amsgrad", False) else 0, *after)
        if self.flat_ema is not None:
            entry, args = entry + "_ema", args + (self.flat_ema.data_ptr(), self.ema_decay)
        with torch.cuda.device(dev):
            _capi.check(getattr(_capi.lib(), entry)(*args, torch.cuda.current_stream(dev).cuda_stream), entry)
        live, shadow = self._weight_readers()
        live.invalidate_packed()
        if shadow is not None:
            shadow.invalidate_packed()

    def _count_skip(self, info: Dict, grad_norm: float) -> None:
        """A step that is not taken (non-finite loss, gradient or network output): counted, announced, logged without an allowance."""
        self.skipped_steps += 1
        print(self.SKIP_MESSAGE.format(self.skipped_steps))
        if self.clip_grad:
            info["grad_norm"], info["max_grad_norm"] = grad_norm, float("nan")

    # ---- resume ---------------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict:
        """What a bit-identical continuation needs besides the module's own state_dict(): parameter names, skipped-step counter, clipping
        history; the flat AdamW moments, step counter and the hyper-parameters of `optimizer.param_groups` (not in the generic mode); the
        average if one is kept (no key at all without: states of earlier versions and of EMA-less runs are the same)."""
        sd: Dict = {"names": list(self.names), "skipped_steps": int(self.skipped_steps),
                    "gradnorm_queue": list(self.gradnorm_queue.items) if self.clip_grad else None}
        if self.fused:
            sd["opt_step"] = int(self.opt_step)
            sd["param_groups"] = [{k: v for k, v in g.items() if k != "params"} for g in self.optimizer.param_groups]
            for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
                sd[k] = getattr(self, k).detach().clone()
        if self.flat_ema is not None:
            sd["ema_decay"] = float(self.ema_decay)
            sd["ema"] = self.flat_ema.detach().clone()
        return sd

    def load_state_dict(self, sd: Dict) -> None:
        """Takes over what `state_dict` wrote.  A saved average is ignored by a trainer that keeps none; a trainer that keeps one is left
        with its own if the state holds none."""
        if list(sd["names"]) != list(self.names):
            raise ValueError("trainer state belongs to a different parameter list")
        self.skipped_steps = int(sd["skipped_steps"])
        if self.clip_grad and sd.get("gradnorm_queue") is not None:
            self.gradnorm_queue.items = [float(x) for x in sd["gradnorm_queue"]]
        with torch.no_grad():
            if self.fused:
                self.opt_step = int(sd["opt_step"])
                for g, saved in zip(self.optimizer.param_groups, sd["param_groups"]):
                    g.update(saved)
                for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
                    getattr(self, k).copy_(sd[k].to(self.flat_param.device))
            if self.flat_ema is not None and sd.get("ema") is not None:
                self.ema_decay = float(sd.get("ema_decay", self.ema_decay))
                self.flat_ema.copy_(sd["ema"].to(device=self.flat_ema.device, dtype=self.flat_ema.dtype))

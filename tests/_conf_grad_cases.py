"""Shared helpers of the Confidence training tests: one recorded training step of the reference's `ConfModule` per c*_conf_* fixture
(tests/golden/cg_*.npz, tools/make_goldens_confidence_grad.py) - targets, the reference's float64 loss / logits / autograd gradients -
and the restatement of that step on the CPU (oracle trunk + pooled gated readout + BCE / MSE) in either precision."""
import json
import os

import numpy as np
import torch

import leftnet_oracle as oracle
from _cases import GOLDEN
from _conf_cases import ConfCase, readout64
from _grad_cases import GradCase

#: fixture -> (the c*_conf_* fixture whose inputs, configuration and entry it takes, loss)
CG_CASES = {
    "cg_wrapper_small": ("ca_conf_wrapper_small", "bce"),
    "cg_ragged_h32": ("cb_conf_ragged_h32", "bce"),
    "cg_prod_b1_n5": ("cc_conf_prod_b1_n5", "bce"),
    "cg_prod_b2_n23": ("cd_conf_prod_b2_n23", "bce"),
    "cg_h32_r32_t": ("ce_conf_h32_r32_t", "mse"),
}


def conf_loss(logits, y, kind):
    """ConfModule.compute_loss's last lines (pl_trainer.py:564-565, 584): BCELoss(sigmoid(preds), y) or MSELoss(preds, y)."""
    logits = logits.reshape(-1)
    if kind == "bce":
        return torch.nn.functional.binary_cross_entropy(torch.sigmoid(logits), y.to(logits.dtype))
    return torch.nn.functional.mse_loss(logits, y.to(logits.dtype))


def restated_step(c: ConfCase, y, kind, dtype, nodeframe):
    """One training step of the restatement under torch autograd on the CPU: `_conf_cases.restate64`'s arithmetic with every operand in
    `dtype` -> ({name: gradient or None}, loss, logits)."""
    sd = c.state_dict(dtype)
    for k, v in sd.items():
        if v.is_floating_point() and "radial_emb" not in k:
            v.requires_grad_(True)
    st = {}
    oracle.dynamics_forward(sd, c.cfg, [x.to(dtype) for x in c.xh], c.edge_index, c.t.to(dtype), c.conditions.to(dtype),
                            c.n_frag_switch, c.combined_mask, c.cnf, nodeframe=nodeframe, stages=st)
    s = st[f"l{c.cfg['num_layers'] - 1}.s"]
    logits = readout64(sd, oracle._scatter_mean(s, c.combined_mask, c.B))
    loss = conf_loss(logits, y, kind)
    loss.backward()
    return {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.requires_grad}, float(loss.detach()), logits.detach()


def conf_module(c: ConfCase, dev, trainable=True, state=None):
    """The Confidence module of a c*_conf_* fixture with its synthetic weights (or `state`)."""
    from oareactdiff_amd.confidence import Confidence
    m = Confidence(model_config=dict(c.cfg), fragment_names=[f"o{k}" for k in range(c.n_obj)], node_nfs=c.node_nfs, edge_nf=0,
                   condition_nf=c.cnf, device=dev, trainable=trainable)
    m.load_state_dict(c.state_dict() if state is None else state, strict=True)
    return m


class ConfGradCase:
    """A cg_* fixture with `GradCase.compare`'s arithmetic on its gradients (same gnorm / gfull / grow / gcol / gidx / gval layout)."""
    compare = GradCase.compare

    def __init__(self, name):
        self.name = name
        self.z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.meta = json.loads(str(self.z["meta"]))
        self.kind = self.meta["loss"]
        self.inputs = ConfCase(self.meta["inputs_of"])
        self.names = [k[len("gnorm."):] for k in self.z.files if k.startswith("gnorm.")]
        self.none_names = set(self.meta["grad_none"])
        self.y = torch.from_numpy(self.z["target"])
        self.loss64 = float(self.z["f64_loss"])
        self.logits64 = torch.from_numpy(self.z["f64_logits"])
        self.ref_gap, self.torch32 = self.meta["ref_f32_vs_f64"], self.meta["torch32_vs_f64"]

    def module(self, dev, trainable=True, state=None):
        return conf_module(self.inputs, dev, trainable, state)

    def batch(self, dev):
        """(representations, res) as ConfModule.compute_loss takes it."""
        c = self.inputs
        return c.representations(dev), {"condition": c.conditions.to(dev), "rmsd": self.y.to(dev)}

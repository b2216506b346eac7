"""Shared helpers of the Confidence tests: load a c*_conf_* fixture, rebuild its weights, restate the model on the CPU in float64."""
import json
import os

import numpy as np
import torch

import leftnet_oracle as oracle
from _cases import GOLDEN
from oareactdiff_amd.graph_tools import get_edges_index
from oareactdiff_amd.spec import confidence_state_spec, synthetic_state_dict

CONF_CASES = ["ca_conf_wrapper_small", "cb_conf_ragged_h32", "cc_conf_prod_b1_n5", "cd_conf_prod_b2_n23", "ce_conf_h32_r32_t"]
GATE = 1e-5          # the project's parity bar: max|d| / max|ref64| over the batch (`rel` of _cases.py)


def readout64(sd, g):
    """GatedMLP H -> H -> H -> 1 (model/core.py:95-131): mlp(g) * sigmoid(gmlp(g)), SiLU behind layers 0 and 1 only."""
    def branch(name, x):
        for layer in range(3):
            x = x @ sd[f"readout.{name}.mlp.{layer}.linear.weight"].t() + sd[f"readout.{name}.mlp.{layer}.linear.bias"]
            if layer < 2:
                x = x * torch.sigmoid(x)
        return x
    return (branch("mlp", g) * torch.sigmoid(branch("gmlp", g))).squeeze(-1)


def restate64(sd64, cfg, xh, edge_index, t, conditions, n_frag_switch, combined_mask, cnf, n_reactions, nodeframe="literal"):
    """Confidence._forward (confidence.py:82-163) in float64: the oracle's trunk up to the node scalars behind the last layer
    (for_conf, leftnet.py:875-876), the mean over every reaction's nodes, the gated readout.  -> [n_reactions]"""
    st = {}
    oracle.dynamics_forward(sd64, cfg, [x.double() for x in xh], edge_index, t.double(), conditions.double(), n_frag_switch,
                            combined_mask, cnf, nodeframe=nodeframe, stages=st)
    s = st[f"l{cfg['num_layers'] - 1}.s"]
    return readout64(sd64, oracle._scatter_mean(s, combined_mask, n_reactions))


class ConfCase:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.name = name
        self.meta = json.loads(str(z["meta"]))
        self.cfg = dict(self.meta["model_config"])
        self.node_nfs, self.cnf = self.meta["node_nfs"], self.meta["condition_nf"]
        self.entry = self.meta["entry"]
        self.n_obj = len(self.node_nfs)
        self.sizes = [torch.tensor(f, dtype=torch.long) for f in self.meta["fragments_nodes"]]
        self.B = int(self.sizes[0].numel())
        self.xh = [torch.from_numpy(z[f"xh{k}"]) for k in range(self.n_obj)]
        self.conditions = torch.from_numpy(z["conditions"])
        self.combined_mask = torch.from_numpy(z["combined_mask"])
        self.n_frag_switch = torch.from_numpy(z["n_frag_switch"])
        self.t = torch.from_numpy(z["t"])
        self.ref64, self.ref32 = torch.from_numpy(z["ref64"]), torch.from_numpy(z["ref32"])
        self.edge_index = get_edges_index(self.combined_mask, remove_self_edge=True)
        self.spec = confidence_state_spec(self.cfg, self.node_nfs, self.cnf)

    def state_dict(self, dtype=torch.float32):
        return synthetic_state_dict(self.spec, self.cfg, seed=42, dtype=dtype)

    def representations(self, dev="cpu"):
        starts = np.concatenate([[0], np.cumsum([x.shape[0] for x in self.xh])])
        return [{"mask": self.combined_mask[starts[k]: starts[k + 1]].to(dev), "size": self.sizes[k].to(dev),
                 "pos": self.xh[k][:, :3].to(dev), "one_hot": self.xh[k][:, 3:-1].to(dev), "charge": self.xh[k][:, -1:].to(dev)}
                for k in range(self.n_obj)]

    def module(self, dev, **attrs):
        from oareactdiff_amd.confidence import Confidence
        m = Confidence(model_config=dict(self.cfg), fragment_names=[f"o{k}" for k in range(self.n_obj)], node_nfs=self.node_nfs,
                       edge_nf=0, condition_nf=self.cnf, device=dev)
        m.load_state_dict(self.state_dict(), strict=True)
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    def restated(self):
        return restate64(self.state_dict(torch.float64), self.cfg, self.xh, self.edge_index, self.t, self.conditions,
                         self.n_frag_switch, self.combined_mask, self.cnf, self.B)

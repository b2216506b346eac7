"""The Confidence model's boundary, without a GPU: state-dict layout, exported symbol, checkpoint file, fixtures against the float64
restatement, ranking helper."""
import os
import re
import sys
import types

import pytest
import torch

from _cases import rel
from _conf_cases import CONF_CASES, ConfCase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def test_state_dict_layout_is_the_references():
    """Keys and shapes equal `confidence_state_spec` (pinned when the fixtures were generated: the reference's Confidence loaded
    this spec's tensors with strict=True): EGNNDynamics' layout plus the twelve readout tensors, in the reference's order."""
    from oareactdiff_amd.confidence import Confidence
    from oareactdiff_amd.dynamics import EGNNDynamics
    from oareactdiff_amd.spec import READOUT_NAMES, confidence_state_spec
    for name in ("ca_conf_wrapper_small", "cd_conf_prod_b2_n23"):
        c = ConfCase(name)
        cfg = dict(c.cfg)
        m = Confidence(model_config=cfg, fragment_names=[f"o{k}" for k in range(c.n_obj)], node_nfs=c.node_nfs, edge_nf=0,
                       condition_nf=c.cnf, device=CPU, update_pocket_coords=False, condition_time=False)     # swallowed **kwargs
        assert cfg["for_conf"] is True                                      # confidence.py:54 mutates the caller's dict
        spec = confidence_state_spec(c.cfg, c.node_nfs, c.cnf)
        sd = m.state_dict()
        assert list(sd.keys()) == list(spec.keys())
        assert all(tuple(sd[k].shape) == spec[k][0] for k in spec)
        d = EGNNDynamics(model_config=dict(c.cfg), fragment_names=[f"o{k}" for k in range(c.n_obj)], node_nfs=c.node_nfs,
                         edge_nf=0, condition_nf=c.cnf, device=CPU)
        assert len(sd) == len(d.state_dict()) + 12
        assert list(sd.keys())[:len(d.state_dict())] == list(d.state_dict().keys()) and tuple(list(sd.keys())[-12:]) == READOUT_NAMES
        H = c.cfg["hidden_channels"]
        assert sd["readout.mlp.mlp.0.linear.weight"].shape == (H, H) and sd["readout.gmlp.mlp.2.linear.weight"].shape == (1, H)
        assert sd["readout.gmlp.mlp.2.linear.bias"].shape == (1,)
        assert not any(p.requires_grad for p in m.parameters())             # inference only
        m.load_state_dict(c.state_dict(), strict=True)
        assert m.update_pocket_coords is True and m.condition_time is True
        # the trunk the library packs is still EGNNDynamics': the readout tensors are not part of the packed parameter list
        assert len(m._ordered_tensors()) == len(d._ordered_tensors())
    # the denoiser still refuses the switch
    with pytest.raises(NotImplementedError):
        EGNNDynamics(model_config=dict(c.cfg, for_conf=True), fragment_names=["a", "b", "c"], node_nfs=c.node_nfs, edge_nf=0,
                     condition_nf=c.cnf, device=CPU)


def test_entry_point_is_declared_exported_and_versioned():
    from oareactdiff_amd import _capi
    from oareactdiff_amd.build import build
    build()
    L = _capi.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oard.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+oard_confidence_forward\s*\(", header)
    assert "oard_confidence_forward" in _capi.EXPORTS and hasattr(L, "oard_confidence_forward")
    assert L.oard_version() == _capi.ABI_VERSION >= 2043
    src = open(os.path.join(ROOT, "oareactdiff_amd", "csrc", "oard_hip.hip")).read()
    assert re.search(r"#define OARD_VERSION %d\b" % _capi.ABI_VERSION, src)


def _write_confmodule_ckpt(path, c):
    """A file as Lightning leaves it for `ConfModule` (pl_trainer.py:421-469: `save_hyperparameters()` pickles the class object
    `model=LEFTNet` and wraps dicts in AttributeDict), written with stand-in classes under the reference's module paths that are
    removed again before loading - the way tests/test_checkpoint.py builds its DDPMModule file."""
    created = []

    def module(name):
        parts = name.split(".")
        for i in range(1, len(parts) + 1):
            n = ".".join(parts[:i])
            if n not in sys.modules:
                sys.modules[n] = types.ModuleType(n)
                created.append(n)
        return sys.modules[name]

    leftnet = module("oa_reactdiff.model.leftnet")

    class LEFTNet(torch.nn.Module):
        pass
    LEFTNet.__module__, LEFTNet.__qualname__ = "oa_reactdiff.model.leftnet", "LEFTNet"
    leftnet.LEFTNet = LEFTNet
    parsing = module("pytorch_lightning.utilities.parsing")

    class AttributeDict(dict):
        pass
    AttributeDict.__module__, AttributeDict.__qualname__ = "pytorch_lightning.utilities.parsing", "AttributeDict"
    parsing.AttributeDict = AttributeDict

    sd = c.state_dict()
    state = {"confidence." + k: v for k, v in sd.items()}
    ckpt = {
        "epoch": 199, "global_step": 4321, "pytorch-lightning_version": "2.0.4", "state_dict": state,
        "loops": {"fit_loop": {"state_dict": {}, "epoch_progress": AttributeDict(total=AttributeDict(ready=3))}},
        "callbacks": {}, "optimizer_states": [{"state": {0: {"step": torch.tensor(7.0)}}, "param_groups": [{"lr": 5e-4}]}],
        "lr_schedulers": [], "hparams_name": "kwargs",
        "hyper_parameters": dict(
            model_config=AttributeDict(dict(c.cfg, for_conf=True)), optimizer_config=dict(lr=5e-4, betas=[0.9, 0.999], weight_decay=0, amsgrad=True),
            training_config=dict(remove_h=False, clip_grad=True, bz=32, datadir="data"), node_nfs=list(c.node_nfs), edge_nf=0,
            condition_nf=c.cnf, fragment_names=["R", "TS", "P"], pos_dim=3, edge_cutoff=None, process_type="TS1x", model=LEFTNet,
            enforce_same_encoding=None, source=None, classification=True, name_temp="conf_hold", target_key="rmsd"),
    }
    torch.save(ckpt, path)
    for n in created:
        del sys.modules[n]


def test_confmodule_checkpoint_file_loads_strict_and_bit_equal(tmp_path):
    from oareactdiff_amd.checkpoint import confidence_from_checkpoint, extract_confidence_state, load_confidence_checkpoint
    from oareactdiff_amd.confidence import Confidence
    c = ConfCase("cd_conf_prod_b2_n23")
    path = os.path.join(tmp_path, "confidence-like.ckpt")
    _write_confmodule_ckpt(path, c)
    assert "oa_reactdiff" not in sys.modules
    conf, hp = load_confidence_checkpoint(path, device=CPU)
    assert isinstance(conf, Confidence)
    sd, got = c.state_dict(), conf.state_dict()
    assert list(got.keys()) == list(sd.keys()) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert hp["classification"] is True and hp["target_key"] == "rmsd" and hp["model_config"]["hidden_channels"] == 196
    assert conf.fragment_names == ["R", "TS", "P"] and conf.condition_nf == c.cnf
    assert "oa_reactdiff" not in sys.modules and "pytorch_lightning" not in sys.modules
    # strict: a file without the readout, or with a tensor too many, is refused
    with pytest.raises(KeyError):
        extract_confidence_state({"confidence." + k: v for k, v in sd.items() if not k.startswith("readout.")})
    hp_min = dict(model_config=dict(c.cfg), node_nfs=c.node_nfs, edge_nf=0, condition_nf=c.cnf)
    with pytest.raises(RuntimeError):
        confidence_from_checkpoint({"state_dict": {**{"confidence." + k: v for k, v in sd.items()},
                                                   "confidence.readout.mlp.mlp.3.linear.weight": torch.zeros(1)},
                                    "hyper_parameters": hp_min}, device=CPU)

    class EGNN:
        pass
    with pytest.raises(NotImplementedError):                                # like dynamics_from_checkpoint
        confidence_from_checkpoint({"state_dict": {}, "hyper_parameters": dict(hp_min, model=EGNN)}, device=CPU)


@pytest.mark.parametrize("name", CONF_CASES)
def test_fixture_is_the_float64_restatement(name):
    """ref64 (the reference's Confidence in float64) == oracle trunk + float64 mean per reaction + gated readout, to 1e-12."""
    c = ConfCase(name)
    assert c.ref64.dtype == torch.float64 and c.ref64.shape == (c.B,) and c.ref32.shape == (c.B,)
    assert (c.entry == "_forward") == (c.t.dim() == 2)
    if c.entry == "forward":
        assert c.t.tolist() == [0]                                          # confidence.py:187
    got = c.restated()
    print(f"{name}: restatement vs ref64 {rel(got, c.ref64):.2e}, reference f32 vs f64 {rel(c.ref32, c.ref64):.2e}")
    assert rel(got, c.ref64) <= 1e-12


def test_rank_candidates_on_hand_made_scores():
    from oareactdiff_amd.confidence import Confidence, rank_candidates
    # K = 3 candidates of 4 reactions, candidate-major: entry k * 4 + r
    scores = torch.tensor([0.1, 0.9, 0.5, 0.3,
                           0.1, 0.2, 0.7, 0.3,
                           0.3, 0.9, 0.7, 0.3])
    best, order = rank_candidates(scores, 4)
    assert best.tolist() == [2, 0, 1, 0]                                    # ties (reactions 1, 2, 3): the lower candidate index
    assert order.tolist() == [[2, 0, 1], [0, 2, 1], [1, 2, 0], [0, 1, 2]]
    assert best.dtype == torch.int64 and order.shape == (4, 3)
    b1, o1 = rank_candidates(torch.tensor([0.2, 0.4]), 2)                   # K = 1
    assert b1.tolist() == [0, 0] and o1.tolist() == [[0], [0]]
    b2, o2 = Confidence.rank_candidates(torch.tensor([0.2, 0.4, 0.4]), 1)   # one reaction, also reachable from the class
    assert b2.tolist() == [1] and o2.tolist() == [[1, 2, 0]]
    with pytest.raises(ValueError):
        rank_candidates(torch.zeros(7), 3)


def test_no_cpu_fallback_and_inference_only():
    from oareactdiff_amd._capi import OardError
    c = ConfCase("ca_conf_wrapper_small")
    m = c.module(CPU)
    with torch.no_grad(), pytest.raises(OardError):
        m(c.representations(), c.conditions)
    getattr(m.readout.mlp.mlp, "0").linear.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="inference only"):
        m(c.representations(), c.conditions)

"""Training the Confidence model, without a GPU: the cg_* fixtures against the restatement's autograd, the set of tensors that get no
gradient, the `trainable` switch, the two library entries."""
import os
import re

import pytest
import torch

from _conf_cases import ConfCase
from _conf_grad_cases import CG_CASES, ConfGradCase, restated_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.mark.parametrize("name", ["cg_ragged_h32", "cg_wrapper_small"])
def test_restatement_autograd_matches_reference_gradients(name):
    """Pins the restatement's backward (torch autograd through oracle trunk + pool + gated readout + loss, float64, literal node frame)
    on the reference's recorded gradients: the bars of test_grad.py::test_oracle_autograd_matches_reference_gradients."""
    g = ConfGradCase(name)
    grads, loss, logits = restated_step(g.inputs, g.y, g.kind, torch.float64, "literal")
    errs, flat = g.compare({k: v for k, v in grads.items() if v is not None})
    assert abs(loss - g.loss64) <= 1e-10 * abs(g.loss64)
    assert float((logits - g.logits64).abs().max()) <= 1e-12 * float(g.logits64.abs().max())
    assert flat <= 1e-8 and max(errs.values()) <= 1e-6, (flat, max(errs.items(), key=lambda kv: kv[1]))
    assert {k for k, v in grads.items() if v is None} == g.none_names


@pytest.mark.parametrize("name", list(CG_CASES))
def test_fixture_records_the_none_set_and_both_noise_floors(name):
    from oareactdiff_amd.confidence import CONF_UNUSED_PREFIXES
    g = ConfGradCase(name)
    assert g.meta["inputs_of"] == CG_CASES[name][0] and g.kind == CG_CASES[name][1]
    names = list(g.inputs.spec)
    params = [n for n in names if "radial_emb" not in n]
    assert g.none_names == {n for n in params if n.startswith(CONF_UNUSED_PREFIXES)}          # what the reference's autograd leaves None
    assert set(g.names) == set(params) - g.none_names                                         # a gradient for every other parameter
    assert set(g.ref_gap) == set(g.names) == set(g.torch32)
    assert g.y.shape == (g.inputs.B,) and g.logits64.shape == (g.inputs.B,)
    if g.kind == "bce":
        assert set(g.y.tolist()) <= {0.0, 1.0} and (g.inputs.B == 1 or len(set(g.y.tolist())) == 2)     # mixed labels
    assert float((g.logits64 - g.inputs.ref64).abs().max()) <= 1e-12          # train() and eval() logits of the reference agree


def test_default_module_is_frozen_and_trainable_switch_sets_requires_grad():
    from oareactdiff_amd.confidence import CONF_UNUSED_PREFIXES, Confidence
    from oareactdiff_amd.spec import READOUT_NAMES
    c = ConfCase("ca_conf_wrapper_small")
    kw = dict(fragment_names=[f"o{k}" for k in range(c.n_obj)], node_nfs=c.node_nfs, edge_nf=0, condition_nf=c.cnf, device=CPU)
    frozen = Confidence(model_config=dict(c.cfg), **kw)
    assert frozen.trainable is False and not any(p.requires_grad for p in frozen.parameters())
    m = Confidence(model_config=dict(c.cfg), trainable=True, **kw)
    assert m.trainable is True and all(p.requires_grad for p in m.parameters())
    assert not any(b.requires_grad for b in m.buffers())
    assert list(m.state_dict().keys()) == list(frozen.state_dict().keys())
    # the tensors a training step reaches: the trunk without the output head / decoders / unused modules, then the readout
    used = m._train_params()
    trunk = [n for n, _ in m.named_parameters() if not n.startswith("readout.")]
    assert list(used)[:-12] == [n for n in trunk if not n.startswith(CONF_UNUSED_PREFIXES)]
    assert tuple(list(used)[-12:]) == READOUT_NAMES
    assert all(used[n] is dict(m.named_parameters())[n] for n in used)
    # no CPU fallback in training mode either
    from oareactdiff_amd._capi import OardError
    with pytest.raises(OardError):
        m(c.representations(), c.conditions)


def test_trainer_refuses_a_frozen_module():
    from oareactdiff_amd import ConfidenceTrainer
    c = ConfCase("ca_conf_wrapper_small")
    with pytest.raises(ValueError, match="trainable=True"):
        ConfidenceTrainer(c.module(CPU))


def test_training_entries_are_declared_exported_and_versioned():
    from oareactdiff_amd import _capi
    from oareactdiff_amd.build import build
    build()
    L = _capi.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oard.h")).read(), flags=re.S)
    for entry in ("oard_confidence_forward_train", "oard_confidence_tail_backward"):
        assert re.search(r"\bint\s+%s\s*\(" % entry, header), entry
        assert entry in _capi.EXPORTS and hasattr(L, entry), entry
    assert L.oard_version() == _capi.ABI_VERSION >= 2044

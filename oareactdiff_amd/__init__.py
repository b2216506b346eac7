"""oareactdiff_amd — MI355X (gfx950) backend for OA-ReactDiff's per-timestep denoising call.

    from oareactdiff_amd import EGNNDynamics        # drop-in for oa_reactdiff.dynamics.EGNNDynamics(model=LEFTNet)
    from oareactdiff_amd import Confidence          # drop-in for oa_reactdiff.dynamics.confidence.Confidence(model=LEFTNet)
    from oareactdiff_amd import ConfidenceTrainer   # ConfModule's training step for Confidence(..., trainable=True)
    from oareactdiff_amd import ReactionStore, DeviceLoader   # ProcessedTS1x + DataLoader on the device, one launch per batch

See DESIGN.md (path, kernels, measurement) and INTEGRATION.md (binding)."""
from .dynamics import EGNNDynamics  # noqa: F401
from .confidence import Confidence, distinct_candidates, rank_candidates, ranking_report  # noqa: F401
from .metrics import binary_auroc, midrank, pearson_corrcoef, rank_metrics, spearman_corrcoef  # noqa: F401
from .sampler import DiffusionSampler  # noqa: F401
from .loss import DiffusionLoss  # noqa: F401
from .trainer import DDPMTrainer  # noqa: F401
from .conf_trainer import ConfidenceTrainer  # noqa: F401
from .data import DeviceLoader, ReactionStore  # noqa: F401
from .graph_tools import get_edges_index, get_mask_for_frag, get_n_frag_switch, get_subgraph_mask  # noqa: F401

__all__ = ["EGNNDynamics", "Confidence", "rank_candidates", "ranking_report", "distinct_candidates", "midrank", "rank_metrics", "binary_auroc", "pearson_corrcoef", "spearman_corrcoef", "DiffusionSampler", "DiffusionLoss", "DDPMTrainer", "ConfidenceTrainer", "ReactionStore", "DeviceLoader", "get_edges_index", "get_mask_for_frag", "get_n_frag_switch", "get_subgraph_mask"]

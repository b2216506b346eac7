"""A ragged 5-reaction batch whose sampling / inpainting trajectories stay inside the cutoff, and its float64 replays (pure host code;
the GPU tests of tests/test_sampler_loops.py compare the device loops with them).

The golden sampler fixtures have the same atom counts in R, TS and P and - with untrained weights and no prior term - inflate to
hundreds of Angstrom, so most of their network calls run on an empty radius graph.  Here the three objects have different counts per
reaction, and both the device loop (`gaussian_prior_std=1`) and the replay (the same term added in its `dynamics` callback, as
tests/test_configs.py does for config 1) follow the reverse process of N(0, 1) data: |pos| stays at a few Angstrom and every same-object
edge is inside the cutoff in every call.  The replay evaluates the network on the float32 rounding of its float64 state, i.e. where
the device evaluates it.  A replay costs about 1.6 s of CPU per network call; they are cached per process."""
import functools

import torch

import leftnet_oracle as oracle
import sampler_oracle as so
from oareactdiff_amd.graph_tools import get_edges_index, get_mask_for_frag, get_n_frag_switch
from oareactdiff_amd.spec import PRODUCTION_LEFTNET_CONFIG, state_spec, synthetic_state_dict

#        atoms per reaction of   R                   TS                  P             N = 183, 9 294 edges, 3 160 of them same-object
FRAGS = ([7, 23, 12, 1, 16], [9, 20, 5, 3, 16], [4, 23, 12, 2, 30])
FRAGS_12 = ([3, 11, 7, 1, 16, 9, 2, 23, 5, 8, 4, 13], [5, 9, 7, 2, 12, 9, 3, 20, 6, 8, 1, 10], [2, 14, 7, 4, 16, 3, 6, 23, 5, 11, 4, 9])
NODE_NFS = [9, 9, 9]
CFG = dict(PRODUCTION_LEFTNET_CONFIG, num_layers=2)
HEAD_SCALE = 0.05                # the untrained output head, tamed as in config 1 / the g4 fixtures
PRECISION = 1e-5
POS = 3


class Batch:
    def __init__(self, frags=FRAGS):
        self.frag = [torch.tensor(f) for f in frags]
        self.masks = [get_mask_for_frag(f) for f in self.frag]
        self.cm = torch.cat(self.masks)
        self.ei = get_edges_index(self.cm, remove_self_edge=True)
        self.nfs = get_n_frag_switch(self.frag)
        self.B = len(frags[0])
        self.cond = torch.zeros(self.B, 1)
        self.inner = int((self.nfs[self.ei[0]] == self.nfs[self.ei[1]]).sum())
        self.sizes = [int(m.numel()) for m in self.masks]
        g = torch.Generator().manual_seed(5)
        self.h0, self.xh_fixed = [], []
        for n in self.sizes:                               # atom types H C N O as one-hot (5 columns) + the atomic number
            typ = torch.multinomial(torch.tensor([0.5, 0.3, 0.1, 0.1]), n, replacement=True, generator=g)
            feat = torch.zeros(n, 6)
            feat[torch.arange(n), typ] = 1.0
            feat[:, 5] = torch.tensor([1.0, 6.0, 7.0, 8.0])[typ]
            self.h0.append(feat)
            self.xh_fixed.append(torch.cat([torch.randn(n, POS, generator=g) + 0.3, feat], dim=1))      # inpaint removes the CoM itself
        self._noise = {}

    def noise(self, i):
        """The i-th set of raw N(0,1) draws, one [n_k, 9] tensor per object, from a CPU generator seeded with the call index."""
        if i not in self._noise:
            g = torch.Generator().manual_seed(1000 + i)
            self._noise[i] = [torch.randn(n, nf, generator=g) for n, nf in zip(self.sizes, NODE_NFS)]
        return self._noise[i]


@functools.lru_cache(maxsize=None)
def batch(n=5):
    return Batch(FRAGS if n == 5 else FRAGS_12)


@functools.lru_cache(maxsize=None)
def weights():
    sd = synthetic_state_dict(state_spec(CFG, NODE_NFS, 1), CFG, seed=42)
    for k in list(sd):
        if "out_pos" in k and "update_net.2" in k:
            sd[k] = sd[k] * HEAD_SCALE
    return sd


def prior_coefficients(table):
    """sigma_t / (alpha_t^2 + sigma_t^2) per entry of a gamma table, float32: E[eps | z_t] = coefficient * z_t for x0 ~ N(0, 1)."""
    out = []
    for g in table.float():
        a, sg = float(torch.sqrt(torch.sigmoid(-g))), float(torch.sqrt(torch.sigmoid(g)))
        out.append(float(torch.tensor(sg / (a * a + sg * sg), dtype=torch.float32)))
    return out


class Replay:
    """x64: the final [pos | features] per object in float64; calls: per network call (float32 inputs, float32 t, float64 network
    output on them, edges inside the cutoff); trace: the state after every ancestral step (sample only)."""

    def __init__(self):
        self.x64, self.calls, self.trace = None, [], []

    @property
    def min_active(self):
        return min(c[3] for c in self.calls)

    @property
    def max_pos(self):
        return max(float(z[:, :POS].abs().max()) for c in self.calls for z in c[0])


@functools.lru_cache(maxsize=None)
def replay(kind, schedule, T, n_steps, pos_only):
    """kind "sample": `so.sample` with `n_steps` steps on the T-step schedule `schedule` (n_steps < T: the gamma table sub-sampled at
    round(k / n_steps * T), en_diffusion.py:471 with _schedule.py:127-129).  kind "inpaint": `so.inpaint`, 2 resamplings, jump length 3,
    objects 0 and 2 fixed.  Both with the Gaussian-prior term."""
    b = batch()
    sd64 = {k: v.double() for k, v in weights().items()}
    full = so.gamma_table(schedule, T, PRECISION)
    assert T % n_steps == 0
    table = full[:: T // n_steps].clone()                 # entry k = gamma at time k / n_steps
    assert table.numel() == n_steps + 1
    pc = prior_coefficients(table)
    r = Replay()

    def dyn64(zt, t):
        z32 = [z.float() for z in zt]
        t32 = t.float()
        st = {}
        o = oracle.dynamics_forward(sd64, CFG, [z.double() for z in z32], b.ei, t32.double(), b.cond.double(), b.nfs, b.cm, 1,
                                    nodeframe="exact", stages=st)
        r.calls.append((z32, t32, o, int(st["edge_mask"].sum())))
        c = pc[int(round(float(t.reshape(-1)[0]) * n_steps))]
        return [torch.cat([x[:, :POS] + c * z[:, :POS], x[:, POS:]], dim=1) for x, z in zip(o, zt)]

    noise = lambda i: [n.double() for n in b.noise(i)]
    torch.set_default_dtype(torch.float64)
    try:
        if kind == "sample":
            r.x64 = so.sample(dyn64, table.double(), n_steps, b.masks, b.B, noise, b.cond.double(), pos_only,
                              [h.double() for h in b.h0] if pos_only else None, trace=r.trace)
        else:
            assert kind == "inpaint" and pos_only
            r.x64 = so.inpaint(dyn64, table.double(), n_steps, b.masks, b.B, noise, b.cond.double(), True,
                               [x.double() for x in b.xh_fixed], [0, 2], 2, 3)
    finally:
        torch.set_default_dtype(torch.float32)
    return r

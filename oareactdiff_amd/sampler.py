"""On-device ancestral sampler around the HIP denoising call.

`DiffusionSampler.sample` mirrors `EnVariationalDiffusion.sample`
(oa_reactdiff/diffusion/en_diffusion.py:459-560): same arguments, same return value
`(out_samples, fragments_masks)`.  Per step it issues one `oard_forward` and the step kernel `oard_sampler_step`
(mu, CoM-free noise, CoM projection, pos_only feature reset fused; launched a second time as a bare projection after the steps
that project, `_project_again`); the schedule scalars come from a host
table, the NaN flag stays on the device, and the reference's four `.item()` asserts per step are gone, so
the loop never synchronises the host with the GPU.

`DiffusionSampler.inpaint` (row N3) runs the RePaint loop the same way on the fused step kernel `oard_inpaint_step`: one launch per
step for the known branch, the denoised branch and the forward jump, group sums in float64."""
from __future__ import annotations

import contextlib
import ctypes as C
import itertools
from typing import Callable, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _capi
from .dynamics import EGNNDynamics
from .graph_tools import get_edges_index, get_mask_for_frag, get_n_frag_switch
from .schedule import Schedule, get_repaint_schedule, repaint_steps


class DiffusionSampler:
    def __init__(self, dynamics: EGNNDynamics, noise_schedule: str = "polynomial_2", timesteps: int = 1000,
                 precision: float = 1e-5, pos_only: bool = False,
                 norm_values: Sequence[float] = (1.0, 1.0, 1.0), norm_biases: Sequence[float] = (0.0, 0.0, 0.0),
                 on_nan: str = "raise", gaussian_prior_std: Optional[float] = None):
        """`gaussian_prior_std` (measurement aid, default off): add to every network prediction the ideal denoiser of a Gaussian data
        prior x0 ~ N(0, s^2) per coordinate, eps = sigma_t z_t / (alpha_t^2 s^2 + sigma_t^2), on the position columns.  An UNTRAINED
        network predicts eps ~ 0, and the ancestral sampler then scales its state by 1 / alpha_t|s every step (en_diffusion.py:614-618):
        positions reach hundreds of Angstrom within a few calls, every pair leaves the cutoff and the remaining calls run on an empty
        radius graph.  With the prior term the chain is the exact reverse process of N(0, s^2) data: the state keeps the marginal
        alpha_t^2 s^2 + sigma_t^2 (= 1 for s = 1, the distribution of the headline's inputs) and every network call sees a
        molecule-sized cloud, as a trained model's would.  One in-place axpy per object and step on the loop's stream; the network
        call itself is untouched.  Used by bench.py's T = 1000 line and tests/test_configs.py (the float64 replay adds the same term).
        The term applies after EVERY network call of `sample` and of `inpaint` (the denoising calls at time (s + 1) / T and the final call
        at time 0; in `inpaint` the objects of `frag_fixed` receive it too, and their denoised branch is discarded as before).

        `on_nan`: what to do when any network call of a run predicted a NaN displacement.  The reference replaces that
        step's velocity by randn, prints a warning and keeps sampling (egnn_dynamics.py:138-143) - one host sync per
        step.  Here the loop never syncs: every call ORs its NaN flag into a device-side sticky flag which is read ONCE
        after the loop; "raise" (default) raises FloatingPointError, "warn" warns and returns the (NaN) samples,
        "replace" reproduces the reference: the step's velocity becomes CoM-free randn ON THE DEVICE (oard_nan_replace, keyed on the
        call's device-side flag; costs one extra randn draw per object and step, so the noise stream of a seeded run differs from the
        other modes) and a warning is printed once after the loop."""
        assert on_nan in ("raise", "warn", "replace")
        self.on_nan = on_nan
        self.prior_std = None if gaussian_prior_std is None else float(gaussian_prior_std)
        self.dynamics = dynamics
        self.schedule = Schedule(noise_schedule, timesteps, precision)
        self.T = timesteps
        self.pos_only = pos_only
        self.pos_dim = dynamics.pos_dim
        self.node_nfs = dynamics.node_nfs
        self.norm_values = tuple(norm_values)
        self.norm_biases = tuple(norm_biases)
        self._layout_cache = {}
        self.last_x: Optional[List[Tensor]] = None         # final (normalised) state and status of the last run
        self.last_status: Optional[Tensor] = None
        #: upper bound on the pre-drawn noise of the hipGraph-replayed loop (`sample(graph=True)` / small batches)
        self.noise_block_bytes = 64 << 20
        self.last_inpaint_loop: Optional[str] = None       # the loop the last `inpaint` took: "graphed", "fused" or "unfused"
        self.last_inpaint_refills = 0                      # noise-table refills of the last graphed `inpaint`

    def _layout(self, fragments_nodes: List[Tensor], dev):
        """Batch-layout tensors (masks, combined_mask, edge_index, n_frag_switch) on the device, cached by the
        atom counts so that repeated sample()/inpaint() calls reuse the same tensors (and therefore the
        dynamics' cached index tables)."""
        key = tuple(tuple(int(v) for v in f.tolist()) for f in fragments_nodes)
        hit = self._layout_cache.get(key)
        if hit is None:
            fn = [f.to(dev) for f in fragments_nodes]
            masks = [get_mask_for_frag(f) for f in fn]
            combined_mask = torch.cat(masks)
            hit = (masks, combined_mask, get_edges_index(combined_mask, remove_self_edge=True), get_n_frag_switch(fn))
            if len(self._layout_cache) >= 4:
                self._layout_cache.pop(next(iter(self._layout_cache)))
            self._layout_cache[key] = hit
        return hit

    def _check_nan(self, dyn) -> None:
        """The single host read of a sampling run: did any of its network calls produce a NaN displacement?"""
        if dyn.nan_seen is not None and int(dyn.nan_seen[0].item()) != 0:
            if self.on_nan == "replace":
                print("Warning: detected nan in pos, resetting EGNN output to randn.")       # the reference's message (:139)
                return
            msg = ("a network call of this sampling run predicted NaN positions; the reference would have replaced that "
                   "step by randn (egnn_dynamics.py:138-143), this loop does not: the affected samples are NaN")
            if self.on_nan == "raise":
                raise FloatingPointError(msg)
            import warnings
            warnings.warn(msg)

    def prior_coefficient(self, step: int, n_steps: int) -> float:
        """sigma_t / (alpha_t^2 s^2 + sigma_t^2) at time step / n_steps: E[eps | z_t] = coefficient * z_t for x0 ~ N(0, s^2)."""
        a, sg = self.schedule.alpha_sigma(step, n_steps)
        return sg / (a * a * self.prior_std * self.prior_std + sg * sg)

    def _prior_table(self, timesteps: int, dev) -> Tensor:
        """[T + 1] float32 on the device: entry k = the coefficient at time k / T.  Built once per run; both loops read their coefficient
        from it as a [1] device tensor, so the eager loop and the hipGraph replay run the same kernel on the same operands (bit-identical)."""
        return torch.tensor([self.prior_coefficient(k, timesteps) for k in range(timesteps + 1)], dtype=torch.float32, device=dev)

    def _add_prior(self, eps_hat, z, coef: Tensor) -> None:
        """eps_hat[:, :pos_dim] += coef * z[:, :pos_dim] per object; `coef` a [1] device tensor."""
        pd = self.pos_dim
        for e, x in zip(eps_hat, z):
            if e.numel():
                e[:, :pd].addcmul_(x[:, :pd], coef)

    def _denoise(self, z, t, prior_tab, at, edge_index, conditions, n_frag_switch, combined_mask):
        """One network call at time `t` ([1] device tensor) -> eps_hat, with the prior term added when the run has a prior table: its
        entry `at`, a slice (the eager loops: a view) or a [1] device index (the replayed loops: an index_select, issued after the
        network call as the loops always did)."""
        eps_hat, _ = self.dynamics(z, edge_index, t, conditions, n_frag_switch, combined_mask)
        if prior_tab is not None:
            self._add_prior(eps_hat, z, prior_tab[at] if isinstance(at, slice) else prior_tab.index_select(0, at))
        return eps_hat

    def _noise_source(self, noise_fn, sizes, dev):
        """-> draw(i): the i-th set of raw N(0, 1) draws of a run, one [n_k, node_nf_k] float32 tensor per object on the device - from
        `noise_fn(i)` (tests) if given, else torch.randn there."""
        def draw(i):
            if noise_fn is not None:
                return [x.to(device=dev, dtype=torch.float32).contiguous() for x in noise_fn(i)]
            return [torch.randn(n, nf, device=dev) for n, nf in zip(sizes, self.node_nfs)]
        return draw

    # --------------------------------------------------------------------------------------------
    def _launch_step(self, topo, mode, z, eh, noise, h0, scalars, out, stream):
        """One launch of the step kernel, then the second projection for the modes that project (0 and 4).  `scalars`: the three
        schedule scalars as host floats (a, b, c), or a [3] device tensor (the launch a hipGraph replays)."""
        L = _capi.lib()
        cfg = self.dynamics._config()
        arr = _capi.ptr_array
        first = [torch.empty_like(o) for o in out] if mode in (0, 4) else out
        head = (C.byref(cfg), topo.handle, mode, arr(z), arr(eh), arr(noise), arr(h0))
        tail = (1 if self.pos_only else 0, arr(first), stream)
        if isinstance(scalars, Tensor):
            _capi.check(L.oard_sampler_step_dev(*head, scalars.data_ptr(), *tail), "oard_sampler_step_dev")
        else:
            _capi.check(L.oard_sampler_step(*head, *[C.c_float(v) for v in scalars], *tail), "oard_sampler_step")
        if first is not out:
            self._project_again(topo, first, h0, out, stream)

    def _step_kernel(self, topo, mode, z, eh, noise, h0, a, b, c, out, stream):
        self._launch_step(topo, mode, z, eh, noise, h0, (a, b, c), out, stream)

    def _step_kernel_dev(self, topo, mode, z, eh, noise, h0, coef, out, stream):
        """As `_step_kernel` with the schedule scalars in device memory (`coef` [3]): the launch a hipGraph replays."""
        self._launch_step(topo, mode, z, eh, noise, h0, coef, out, stream)

    def _project_again(self, topo, x, h0, out, stream):
        """Second CoM projection of a mode 0 / mode 4 result: out = x - mean_group(x) on the positions, everything else copied (the
        step kernel in mode 4 with a = 1, c = 0; `x` itself stands in for the noise operand, which c = 0 switches off, so nothing
        else is read and a finite x gives a finite out).  The kernel adds a group's rows up in a float32 running sum, so the mean it
        removes carries ~1e-7 of the UN-projected values per row: when those share an offset far above their spread (|mean| ~ 60,
        spread ~ 1) a mean of 3e-6 ... 1e-5 max|out| stays in the output.  The second pass sums values of the size of the output
        and leaves 1e-8.  The loops' own operands are CoM-free, so for them the pass changes last bits only; it is here because the
        wrappers promise a CoM-free result for ANY operands.  (The one-launch form - float64 group sums inside the step kernel - is
        what the inpainting loop's k_inpaint_step does; k_sampler_step and `sample` keep the two passes.)"""
        arr = _capi.ptr_array
        rc = _capi.lib().oard_sampler_step(C.byref(self.dynamics._config()), topo.handle, 4, arr(x), None, arr(x), arr(h0),
                                           C.c_float(1.0), C.c_float(0.0), C.c_float(0.0), 1 if self.pos_only else 0, arr(out), stream)
        _capi.check(rc, "oard_sampler_step (second projection)")

    def _replay(self, dev, n_steps, block, one_step, refill, step_callback=None):
        """The capture-and-replay protocol of the graphed loops: `one_step()` run `n_steps` times on a side stream that waits for the
        caller's - once eagerly (the warm-up torch.cuda.graph requires), then captured once and replayed - and joined back at the end.
        `refill(first, n_rows)` draws the noise rows of steps first .. first + n_rows - 1 into the loop's tables and resets its row
        counter; it is called before the first step and then whenever `block` steps have used a block up.  `step_callback(i)` is
        called with the side stream current after the warm-up step and after every replay."""
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            refill(0, min(block, n_steps))
            one_step()
            done, in_block = 1, 1
            if step_callback is not None:
                step_callback(done)
            if n_steps > 1:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    one_step()
                while done < n_steps:
                    if in_block == block:
                        refill(done, min(block, n_steps - done))
                        in_block = 0
                    g.replay()
                    done += 1
                    in_block += 1
                    if step_callback is not None:
                        step_callback(done)
        torch.cuda.current_stream(dev).wait_stream(side)

    def _graphed_steps(self, topo, timesteps, za, draw, h0d, net, dev, step_callback=None):
        """The T ancestral steps of `sample` as ONE captured hipGraph replayed T times (small batches are launch-bound:
        ~100 kernel launches per step).  The per-step scalars live in device tables indexed by a device-side step counter:
        t, the three schedule coefficients and the step's noise draw; the graph holds [table lookups, oard_forward,
        oard_sampler_step_dev, its second projection (oard_sampler_step with constant scalars), z <- z_new, counter += 1].  Same
        kernels and same arithmetic as the eager loop, so the result is bit-identical.  `_replay` runs it; `net`: the network call's
        (edge_index, conditions, n_frag_switch, combined_mask)."""
        n_obj = len(self.node_nfs)
        steps = list(reversed(range(timesteps)))
        coefs = [self.schedule.step(s, timesteps) for s in steps]
        coef_tab = torch.tensor([[c.alpha_ts, c.c_eps, c.sigma] for c in coefs], dtype=torch.float32, device=dev)      # [T,3]
        # the eager loop's t values, bit for bit: (arange(T + 1) / T)[s + 1]
        t_tab = (torch.arange(timesteps + 1, device=dev, dtype=torch.float32) / timesteps)[torch.tensor([s + 1 for s in steps], device=dev)]
        prior_tab = (self._prior_table(timesteps, dev)[torch.tensor([s + 1 for s in steps], device=dev)]
                     if self.prior_std is not None else None)
        # The noise of the steps is drawn in BLOCKS (not all T draws up front: that would be T x the eager loop's memory -
        # a [T, n, nf] table per object): at most `noise_block_bytes` of draws exist at a time, refilled between replays in
        # the eager loop's draw order (call 1 .. T), so a seeded run consumes the generator exactly like the eager loop.
        per_step = 4 * sum(int(x.numel()) for x in za)
        block = max(1, min(timesteps, self.noise_block_bytes // max(per_step, 1)))
        noise_tab = [torch.empty((block,) + tuple(x.shape), dtype=torch.float32, device=dev) for x in za]              # [block, n_k, nf_k]
        counter = torch.zeros(1, dtype=torch.long, device=dev)           # step index (t / coefficient tables)
        slot = torch.zeros(1, dtype=torch.long, device=dev)              # row of the current block's noise table
        z = [x.clone() for x in za]
        z_new = [torch.empty_like(x) for x in za]

        def refill(first, n_rows):
            for r in range(n_rows):
                d = draw(first + r + 1)                                  # call 0 drew the initial state
                for k in range(n_obj):
                    noise_tab[k][r].copy_(d[k])
            slot.zero_()

        def one_step():
            t_cur = t_tab.index_select(0, counter)                       # [1]: a 1-D t = one value for every node
            coef = coef_tab.index_select(0, counter).view(3)
            noise = [nt.index_select(0, slot)[0] for nt in noise_tab]
            eps_hat = self._denoise(z, t_cur, prior_tab, counter, *net)
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._step_kernel_dev(topo, 0, z, eps_hat, noise, h0d if self.pos_only else None, coef, z_new, stream)
            for a, b in zip(z, z_new):
                a.copy_(b)
            counter.add_(1)
            slot.add_(1)
        self._replay(dev, timesteps, block, one_step, refill, step_callback)
        return z

    @contextlib.contextmanager
    def _run(self, n_samples: int, fragments_nodes: List[Tensor], conditions: Optional[Tensor]):
        """What `sample` and `inpaint` do around their loops -> (dev, (masks, combined_mask, edge_index, n_frag_switch), conditions, topo,
        stream), with the device current: the batch layout, default conditions, the module's NaN check switched to the loop's (no host
        sync; restored on the way out) with a cleared sticky flag, and the production topology.  After a loop that ended normally the
        flag is read - the run's single host read (`_check_nan`)."""
        dyn = self.dynamics
        dev = next(dyn.parameters()).device
        if dev.type != "cuda":
            raise _capi.OardError("DiffusionSampler needs the dynamics on a ROCm device (no CPU fallback)")
        layout = self._layout(fragments_nodes, dev)
        _, combined_mask, edge_index, n_frag_switch = layout
        if conditions is None:
            conditions = torch.zeros(n_samples, max(dyn.condition_nf, 1), device=dev)
        conditions = conditions.to(dev)
        old_nan = dyn.nan_check
        dyn.nan_check = "replace" if self.on_nan == "replace" else "async"
        dyn.reset_nan_seen()
        try:
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                topo = dyn._get_topology(dyn._config(), edge_index, n_frag_switch, combined_mask, stream)
                if topo.handle is None:
                    raise _capi.OardError("the sampling loops run on the production kernels: hidden_channels / num_radial must be a built width "
                                          "pair (OARD_DIMS=... python -m oareactdiff_amd.build) and a (sample, object) group at most 1024 atoms")
                yield dev, layout, conditions, topo, stream
        finally:
            dyn.nan_check = old_nan
        self._check_nan(dyn)

    def _to_samples(self, x: List[Tensor], h0: Optional[List[Tensor]], h0_long: bool) -> List[Tensor]:
        """The final state un-normalised into [pos | one-hot | charge] per object (en_diffusion.py:542-557, :680-683).  `pos_only`: the
        features are `h0`'s, as integers if `h0_long` (inpaint; sample hands them back in h0's dtype)."""
        nv, nb, pd = self.norm_values, self.norm_biases, self.pos_dim
        n_obj = len(self.node_nfs)
        pos = [x[k][:, :pd] * nv[0] + nb[0] for k in range(n_obj)]
        if self.pos_only:
            cat, charge = [h[:, :-1] for h in h0], [h[:, -1:] for h in h0]
            if h0_long:
                cat, charge = [c.long() for c in cat], [c.long() for c in charge]
        else:
            cat = [torch.nn.functional.one_hot(torch.argmax(x[k][:, pd:-1] * nv[1] + nb[1], dim=1),
                                               self.node_nfs[k] - 4).long() for k in range(n_obj)]
            charge = [torch.round(x[k][:, -1:] * nv[2] + nb[2]).long() for k in range(n_obj)]
        return [torch.cat([pos[k], cat[k], charge[k]], dim=1) for k in range(n_obj)]

    @torch.no_grad()
    def sample(self, n_samples: int, fragments_nodes: List[Tensor], conditions: Optional[Tensor] = None,
               return_frames: int = 1, timesteps: Optional[int] = None, h0: Optional[List[Tensor]] = None,
               noise_fn: Optional[Callable[[int], List[Tensor]]] = None, graph: Optional[bool] = None,
               step_callback: Optional[Callable[[int], None]] = None) -> Tuple[list, List[Tensor]]:
        """`noise_fn(i)` (tests) supplies the i-th set of raw N(0,1) draws, one [n_k, node_nf_k] tensor per
        object (i = 0 initial state, 1..T the steps, T+1 the final draw); default: torch.randn on the device.
        `graph`: replay the step as a captured hipGraph (`_graphed_steps`; bit-identical to the eager loop, noise drawn in
        blocks of at most `self.noise_block_bytes`); None = automatically for launch-bound batches (n_samples <= 8, one returned
        frame) unless the caller's stream is itself being captured (then the eager loop runs, which is capturable).
        `step_callback(i)`: called on the host after the i-th network call has been enqueued (i = 1 ... T; progress bars, timing
        events - it must not synchronise if the loop is to stay free of host waits).  The graphed loop calls it after the warm-up step
        and after every replay, with its capture stream current."""
        timesteps = self.T if timesteps is None else timesteps
        assert 0 < return_frames <= timesteps and timesteps % return_frames == 0       # en_diffusion.py:473-475
        assert h0 is not None if self.pos_only else True
        dyn = self.dynamics
        n_obj = len(self.node_nfs)
        with self._run(n_samples, fragments_nodes, conditions) as (dev, layout, conditions, topo, stream):
            masks, combined_mask, edge_index, n_frag_switch = layout
            h0d = [h.to(device=dev, dtype=torch.float32).contiguous() for h in h0] if h0 is not None else None
            net = (edge_index, conditions, n_frag_switch, combined_mask)
            sizes = [int(m.numel()) for m in masks]
            draw = self._noise_source(noise_fn, sizes, dev)
            za = [torch.empty(sizes[k], self.node_nfs[k], device=dev) for k in range(n_obj)]
            zb = [torch.empty_like(z) for z in za]
            self._step_kernel(topo, 2, None, None, draw(0), h0d if self.pos_only else None, 0.0, 0.0, 1.0, za, stream)
            t_table = torch.arange(timesteps + 1, device=dev, dtype=torch.float32) / timesteps
            ptab = self._prior_table(timesteps, dev) if self.prior_std is not None else None
            out_samples = [None] * return_frames
            call = 1
            use_graph = ((n_samples <= 8 and return_frames == 1 and not torch.cuda.is_current_stream_capturing())
                         if graph is None else bool(graph))
            if use_graph:
                assert return_frames == 1, "intermediate frames need the eager loop"
                za = self._graphed_steps(topo, timesteps, za, draw, h0d, net, dev, step_callback)
                call = timesteps + 1
            for s in (reversed(range(timesteps)) if not use_graph else ()):
                co = self.schedule.step(s, timesteps)
                eps_hat = self._denoise(za, t_table[s + 1: s + 2], ptab, slice(s + 1, s + 2), *net)
                self._step_kernel(topo, 0, za, eps_hat, draw(call), h0d if self.pos_only else None,
                                  co.alpha_ts, co.c_eps, co.sigma, zb, stream)
                if step_callback is not None:
                    step_callback(call)
                call += 1
                za, zb = zb, za
                if (s * return_frames) % timesteps == 0 and return_frames > 1:
                    out_samples[(s * return_frames) // timesteps] = self._unnormalize_z([z.clone() for z in za])
            fc = self.schedule.final()
            eps_hat = self._denoise(za, t_table[0:1], ptab, slice(0, 1), *net)
            self._step_kernel(topo, 1, za, eps_hat, draw(call), None, fc.inv_alpha_0, fc.sigma_0, fc.sigma_x, zb, stream)
            x = zb
            self.last_x = x
            self.last_status = dyn.last_status
        out_samples[0] = self._to_samples(x, h0d, h0_long=False)
        return out_samples, masks

    @torch.no_grad()
    def sample_sharded(self, fragments_nodes: List[Tensor], conditions: Optional[Tensor] = None, seed: int = 0,
                       gather: bool = False, h0: Optional[List[Tensor]] = None, **kw):
        """BASELINE configs[2]: a GLOBAL batch (per-object atom counts of all B reactions) sharded over the ranks of the
        default process group, one process per GPU.  Reactions are independent (utils/_graph_tools.py:30), so every rank
        samples its contiguous slice `shard_range(B, rank, world)` with its own RNG stream (`seed + rank`) and NO
        data-path collective.  `gather=True` adds one host-side gather of the final samples on rank 0 (the only
        communication of the whole run).  Returns (samples, masks, (lo, hi)); with `gather` rank 0 gets the samples of the
        whole batch per object (in batch order), the other ranks their own."""
        return self._run_sharded(self.sample, "h0", fragments_nodes, h0, conditions, seed, gather, kw)

    def _run_sharded(self, run, rows_name, fragments_nodes, rows, conditions, seed, gather, kw):
        """`sample_sharded` / `inpaint_sharded`: `run` (`sample` or `inpaint`) on this rank's reactions `shard_range(B, rank, world)` -
        their atom counts, their conditions and, if `rows` (h0 / xh_fixed, passed on as `rows_name`) is given, object k's rows of them
        by its cumulative atom counts -, seeded with `seed + rank`; then, if asked for, the one gather of the samples on rank 0."""
        import torch.distributed as dist
        from .shard import shard_range
        on = dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
        B = int(fragments_nodes[0].numel())
        lo, hi = shard_range(B, rank, world)
        local = [f[lo:hi] for f in fragments_nodes]
        cond = conditions[lo:hi] if conditions is not None else None
        local_rows = None
        if rows is not None:
            local_rows = []
            for f, x in zip(fragments_nodes, rows):
                off = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.long), f.cpu().long()]), 0)
                local_rows.append(x[int(off[lo]): int(off[hi])])
        torch.manual_seed(seed + rank)                     # seeds the device generators too
        out, masks = run(hi - lo, local, conditions=cond, **{rows_name: local_rows}, **kw)
        if gather and world > 1:
            mine = (lo, [o.cpu() for o in out[0]])
            got = [None] * world if rank == 0 else None
            dist.gather_object(mine, got, dst=0)
            if rank == 0:
                got.sort(key=lambda t: t[0])
                out = list(out)
                out[0] = [torch.cat([g[1][k] for g in got], dim=0) for k in range(len(self.node_nfs))]
        return out, masks, (lo, hi)

    def _inpaint_step(self, topo, fixed_mask, z, eh, xf, nk, ns, nj, h0, coef, out, stream):
        """One launch of the fused RePaint step (`oard_inpaint_step`; include/oard.h has the formulas).  `coef`: the eight scalars
        [a_s, sigma_s, alpha_ts, c_eps, sigma, jump, a_j, sigma_j] as host floats, or an [8] device tensor (the launch a hipGraph
        replays: `oard_inpaint_step_dev`).  `nj` may be None for a host `coef` whose jump flag is 0."""
        L = _capi.lib()
        arr = _capi.ptr_array
        head = (C.byref(self.dynamics._config()), topo.handle, fixed_mask, arr(z), arr(eh), arr(xf), arr(nk), arr(ns), arr(nj), arr(h0))
        tail = (1 if self.pos_only else 0, arr(out), stream)
        if isinstance(coef, Tensor):
            _capi.check(L.oard_inpaint_step_dev(*head, coef.data_ptr(), *tail), "oard_inpaint_step_dev")
        else:
            _capi.check(L.oard_inpaint_step(*head, (C.c_float * 8)(*coef), *tail), "oard_inpaint_step")

    def _repaint_coefficients(self, s: int, jump_to: Optional[int], timesteps: int) -> List[float]:
        """The coefficient row of `oard_inpaint_step` for the step to s, re-noised to `jump_to` if that is set."""
        a_s, sig_s = self.schedule.alpha_sigma(s, timesteps)
        co = self.schedule.step(s, timesteps)
        a_j, sig_j = self.schedule.forward_jump(s, jump_to, timesteps) if jump_to is not None else (1.0, 0.0)
        return [a_s, sig_s, co.alpha_ts, co.c_eps, co.sigma, 0.0 if jump_to is None else 1.0, a_j, sig_j]

    def _graphed_repaint(self, topo, timesteps, steps, fixed_mask, za, xf, draw, hsel, net, dev):
        """The RePaint steps of the fused `inpaint` loop as ONE captured hipGraph, replayed once per entry of `steps` by `_replay`, as
        `_graphed_steps`' are.  Per-step device tables indexed by a device-side counter: t, the 8-float coefficient row (jump flag included: the kernel branches on it, so one launch serves both kinds of
        step), the prior coefficient, and three noise tables (known / step / jump) refilled in blocks of at most
        `noise_block_bytes` in the eager loop's draw order - a jump row is drawn only for the steps that jump, so a seeded run
        consumes the generator exactly like the eager loop.  The graph holds [table lookups, oard_forward, the prior axpy,
        oard_inpaint_step_dev, z <- z_new, counters += 1]: the eager loop's kernels on the eager loop's operands."""
        n_obj = len(self.node_nfs)
        n_steps = len(steps)
        coef_tab = torch.tensor([self._repaint_coefficients(s, j, timesteps) for s, j in steps], dtype=torch.float32, device=dev)   # [S,8]
        idx = torch.tensor([s + 1 for s, _ in steps], device=dev)
        t_tab = (torch.arange(timesteps + 1, device=dev, dtype=torch.float32) / timesteps)[idx]      # the eager loop's t, bit for bit
        prior_tab = self._prior_table(timesteps, dev)[idx] if self.prior_std is not None else None
        per_step = 3 * 4 * sum(int(x.numel()) for x in za)
        block = max(1, min(n_steps, self.noise_block_bytes // max(per_step, 1)))
        # known, step, jump; zeros: a jump row is never drawn for a step that does not jump and never read, but stays finite
        tabs = [[torch.zeros((block,) + tuple(x.shape), dtype=torch.float32, device=dev) for x in za] for _ in range(3)]
        counter = torch.zeros(1, dtype=torch.long, device=dev)           # entry of `steps` (t / coefficient / prior tables)
        slot = torch.zeros(1, dtype=torch.long, device=dev)              # row of the current block's noise tables
        z = [x.clone() for x in za]
        z_new = [torch.empty_like(x) for x in za]
        self.last_inpaint_refills = 0

        def refill(first, n_rows):
            for r in range(n_rows):
                for which in range(3 if steps[first + r][1] is not None else 2):
                    d = draw()
                    for k in range(n_obj):
                        tabs[which][k][r].copy_(d[k])
            slot.zero_()
            self.last_inpaint_refills += 1

        def one_step():
            t_cur = t_tab.index_select(0, counter)
            coef = coef_tab.index_select(0, counter).view(8)
            nk, ns, nj = ([nt.index_select(0, slot)[0] for nt in tab] for tab in tabs)
            eps_hat = self._denoise(z, t_cur, prior_tab, counter, *net)
            stream = torch.cuda.current_stream(dev).cuda_stream
            self._inpaint_step(topo, fixed_mask, z, eps_hat, xf, nk, ns, nj, hsel, coef, z_new, stream)
            for a, b in zip(z, z_new):
                a.copy_(b)
            counter.add_(1)
            slot.add_(1)
        self._replay(dev, n_steps, block, one_step, refill)
        return z

    @torch.no_grad()
    def inpaint(self, n_samples: int, fragments_nodes: List[Tensor], conditions: Optional[Tensor] = None,
                return_frames: int = 1, resamplings: int = 1, jump_length: int = 1, timesteps: Optional[int] = None,
                xh_fixed: Optional[List[Tensor]] = None, frag_fixed: Optional[List[int]] = None,
                noise_fn: Optional[Callable[[int], List[Tensor]]] = None, fused: bool = True,
                graph: Optional[bool] = None) -> Tuple[list, List[Tensor]]:
        """RePaint-style conditional generation, mirror of `EnVariationalDiffusion.inpaint`
        (en_diffusion.py:722-883): objects in `frag_fixed` follow q(z_s | x_fixed), the others are denoised,
        with `resamplings` x `jump_length` forward jumps.  Noise draws are consumed in the reference's order
        (per step: known-branch noise, denoising noise, then the jump noise if any).
        `fused` (default): one `oard_inpaint_step` launch per RePaint step and sub-batch on two ping-ponged state lists (float64 group
        sums, one projection).  `fused=False`: the earlier sequence of up to five `oard_sampler_step` launches per step, bit for bit as
        before; the fused loop differs from it in last bits.
        `graph=True`: replay the fused step as a captured hipGraph (`_graphed_repaint`, bit-identical to the fused eager loop; needs
        `fused`, one returned frame and a stream that is not itself being captured).  None = the eager loop: unlike `sample`'s, this
        replay measured SLOWER than the eager loop at 1, 8 and 64 reactions (profiles/inpaint_loop.txt), so nothing selects it
        automatically.  `self.last_inpaint_loop` names the loop the call took: "graphed", "fused" or "unfused"."""
        timesteps = self.T if timesteps is None else timesteps
        assert 0 < return_frames <= timesteps and timesteps % return_frames == 0
        assert xh_fixed is not None and len(xh_fixed)
        frag_fixed = list(frag_fixed or [])
        dyn = self.dynamics
        n_obj = len(self.node_nfs)
        pd = self.pos_dim
        assert all(0 <= int(k) < n_obj for k in frag_fixed)
        assert fused or not graph, "the hipGraph replay is built on the fused step"
        with self._run(n_samples, fragments_nodes, conditions) as (dev, layout, conditions, topo, stream):
            masks, combined_mask, edge_index, n_frag_switch = layout
            xf = [x.to(device=dev, dtype=torch.float32).clone() for x in xh_fixed]
            h0 = [x[:, pd:].long().to(torch.float32).contiguous() for x in xf]                 # :753
            for k in range(n_obj):                                                              # :755-759
                xf[k][:, :pd] = EGNNDynamics.remove_mean_batch(xf[k][:, :pd], masks[k])
            net = (edge_index, conditions, n_frag_switch, combined_mask)
            sizes = [int(m.numel()) for m in masks]
            calls = itertools.count()                          # the draws are numbered in the order the loop asks for them
            draw_call = self._noise_source(noise_fn, sizes, dev)
            draw = lambda: draw_call(next(calls))              # noqa: E731
            new = lambda: [torch.empty(sizes[k], self.node_nfs[k], device=dev) for k in range(n_obj)]
            hsel = h0 if self.pos_only else None
            zt = new()
            self._step_kernel(topo, 2, None, None, draw(), hsel, 0.0, 0.0, 1.0, zt, stream)
            t_table = torch.arange(timesteps + 1, device=dev, dtype=torch.float32) / timesteps
            ptab = self._prior_table(timesteps, dev) if self.prior_std is not None else None
            steps = repaint_steps(resamplings, jump_length, timesteps)
            fixed_mask = sum(1 << k for k in set(int(k) for k in frag_fixed))
            use_graph = fused and bool(graph)                  # None: the eager loop (measured faster at every batch size, see `graph`)
            self.last_inpaint_loop = "graphed" if use_graph else "fused" if fused else "unfused"
            if use_graph:
                assert return_frames == 1, "intermediate frames need the eager loop"
                zt = self._graphed_repaint(topo, timesteps, steps, fixed_mask, zt, xf, draw, hsel, net, dev)
            elif fused:
                spare = new()                                  # the two state lists of the whole loop, ping-ponged
                for s, jump_to in steps:
                    nk = draw()                                                                         # :797-805
                    eps_hat = self._denoise(zt, t_table[s + 1: s + 2], ptab, slice(s + 1, s + 2), *net)
                    ns = draw()
                    nj = draw() if jump_to is not None else None                                        # :833-850
                    self._inpaint_step(topo, fixed_mask, zt, eps_hat, xf, nk, ns, nj, hsel,
                                       self._repaint_coefficients(s, jump_to, timesteps), spare, stream)
                    zt, spare = spare, zt
            # fused=False: the launch sequence from before the fused step, untouched (A/B); the fused loops above leave it nothing to do
            schedule = [] if fused else get_repaint_schedule(resamplings, jump_length, timesteps)
            s = timesteps - 1
            for i, n_denoise in enumerate(schedule):
                for j in range(n_denoise):
                    a_s, sig_s = self.schedule.alpha_sigma(s, timesteps)
                    known = new()
                    self._step_kernel(topo, 3, xf, None, draw(), hsel, a_s, 0.0, sig_s, known, stream)   # :797-805
                    co = self.schedule.step(s, timesteps)
                    eps_hat = self._denoise(zt, t_table[s + 1: s + 2], ptab, slice(s + 1, s + 2), *net)
                    unknown = new()
                    self._step_kernel(topo, 0, zt, eps_hat, draw(), hsel, co.alpha_ts, co.c_eps, co.sigma, unknown, stream)
                    zt = [known[k] if k in frag_fixed else unknown[k] for k in range(n_obj)]            # :827-830
                    if j == n_denoise - 1 and i < len(schedule) - 1:                                   # :833-850
                        t = s + jump_length
                        a_ts, sig_ts = self.schedule.forward_jump(s, t, timesteps)
                        jumped = new()
                        self._step_kernel(topo, 4, zt, None, draw(), None, a_ts, 0.0, sig_ts, jumped, stream)
                        zt = jumped
                        s = t
                    s -= 1
            fc = self.schedule.final()
            eps_hat = self._denoise(zt, t_table[0:1], ptab, slice(0, 1), *net)
            x = new()
            self._step_kernel(topo, 1, zt, eps_hat, draw(), None, fc.inv_alpha_0, fc.sigma_0, fc.sigma_x, x, stream)
            self.last_x = x
            self.last_status = dyn.last_status
        out_samples = [None] * return_frames
        out_samples[0] = self._to_samples(x, h0, h0_long=True)
        return out_samples, masks

    @torch.no_grad()
    def inpaint_sharded(self, fragments_nodes: List[Tensor], xh_fixed: List[Tensor], conditions: Optional[Tensor] = None,
                        seed: int = 0, gather: bool = False, **kw):
        """`inpaint` on a GLOBAL batch sharded over the ranks of the default process group, the mirror of `sample_sharded`: every rank
        takes the reactions `shard_range(B, rank, world)` - their atom counts, conditions and the rows of every `xh_fixed[k]` (by the
        cumulative atom counts of object k) -, seeds with `seed + rank` and runs `inpaint`; no collective inside the loop.
        `gather=True`: one host-side gather of the samples on rank 0, in batch order.  Returns (samples, masks, (lo, hi))."""
        return self._run_sharded(self.inpaint, "xh_fixed", fragments_nodes, xh_fixed, conditions, seed, gather, kw)

    def _unnormalize_z(self, z: List[Tensor]) -> List[Tensor]:
        nv, nb, pd = self.norm_values, self.norm_biases, self.pos_dim
        for k in range(len(z)):
            z[k][:, :pd] = z[k][:, :pd] * nv[0] + nb[0]
            z[k][:, pd:-1] = z[k][:, pd:-1] * nv[1] + nb[1]
            z[k][:, -1:] = z[k][:, -1:] * nv[2] + nb[2]
        return z

/*
 * oard.h — C ABI of liboard_hip.so: the MI355X (gfx950) implementation of OA-ReactDiff's
 * per-timestep denoising call,
 *
 *     EGNNDynamics.forward   oa_reactdiff/dynamics/egnn_dynamics.py:63-168
 *       -> LEFTNet.forward   oa_reactdiff/model/leftnet.py:724-891
 *
 * The reference has no FFI of its own (it is pure Python on torch ops); the interface each
 * entry point replaces is therefore the Python call it stands in for, cited per function.
 * Conventions: every function returns 0 on success or a negative OARD_E* code; nothing here
 * synchronises a stream or the device (oard_topology_create does its work on the host and leaves
 * ONE asynchronous upload behind; the only waits are in oard_topology_check_edge_index, a verification call);
 * all `*_dev` pointers are device pointers on the current HIP device; float tensors are
 * contiguous row-major fp32; the library never touches torch.
 * Threading: calls on DISTINCT (topology, workspace, tape, scratch) objects may run concurrently from several host threads /
 * on several streams: everything a call needs travels in its arguments (oard_config incl. the precision bits, the packed
 * blob, the topology, caller-owned buffers).  Process-global and NOT thread-safe are only the debugging facilities:
 * oard_debug_option / oard_debug_stop_after (A/B switches, read at launch time) and the oard_timing_* event recorder
 * (keep it disabled when calling from several threads).  One process per GPU remains the deployment model
 * (torch.distributed / RCCL).
 */
#ifndef OARD_H
#define OARD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OARD_MAX_OBJECTS 8

#define OARD_OK 0
#define OARD_EINVAL (-1)      /* bad argument / unsupported configuration */
#define OARD_ENOTCOMPLETE (-2)/* topology is not "complete graph per sample" */
#define OARD_EHIP (-3)        /* a HIP runtime call failed */
#define OARD_ENOMEM (-4)      /* workspace too small */

typedef void* oard_stream_t;  /* hipStream_t */

/* Mirrors the constructor arguments of EGNNDynamics / BaseDynamics
 * (oa_reactdiff/dynamics/_base.py:10-80) and the LEFTNet model_config
 * (oa_reactdiff/trainer/train_ts1x.py:43-56) that shape the forward pass. */
typedef struct oard_config {
    int32_t hidden;          /* hidden_channels H                                   */
    int32_t num_radial;      /* num_radial R                                        */
    int32_t num_layers;      /* num_layers L                                        */
    int32_t in_hidden;       /* in_hidden_channels (= embed_dim + time + conditions) */
    int32_t n_obj;           /* len(fragment_names)                                 */
    int32_t node_nf[OARD_MAX_OBJECTS];   /* node_nfs[k] (pos_dim + feature width)   */
    int32_t enc_alias[OARD_MAX_OBJECTS]; /* encoder/decoder index object k uses
                                            (enforce_same_encoding, _base.py:110-113) */
    int32_t condition_nf;
    int32_t condition_time;  /* bool                                                */
    int32_t pos_dim;         /* must be 3                                           */
    float   cutoff;
    int32_t reflect_equiv;   /* LEFTNet reflect_equiv (leftnet.py:268-272, 331, 794-796): 1 = production setting; 0 = the Equi
                                message carries x (x) coord_cross and the edge scalarisation keeps its sign              */
    int32_t precision;       /* OARD_PREC_* bits: arithmetic of the two MFMA edge stages (0 = fp32 everywhere).  A property of
                                the call, not of the process: oard_pack_weights builds the bf16 streams for the bits set, and
                                oard_forward / oard_forward_train must be given the blob packed with the same bits. */
} oard_config;

/* Split precision (csrc/oard_edge_b3.h): every fp32 value as three bf16 terms, six bf16 MFMAs per K block, fp32 accumulation -
 * fp32-grade results (parity <= 1e-5 against the float64 reference like the fp32 kernels).  No counterpart in the reference (which
 * is fp32 torch); the fp32 kernels are the default. */
#define OARD_PREC_GCL_BF16X3 1    /* GCLMessage edge stage of inference calls (throughput launch shape)          */
#define OARD_PREC_EQUI_BF16X3 2   /* EquiMessage edge stage of inference calls                                   */
#define OARD_PREC_TRAIN_BF16X3 4  /* both edge stages of the training-mode forward (the backward stays fp32)      */

/* Library / ABI version (major*1000 + minor). */
int oard_version(void);

/* 0 if this build has kernels for (hidden, num_radial) and the switches in cfg, else OARD_EINVAL. */
int oard_supported(const oard_config* cfg);

/* ---- weights --------------------------------------------------------------------------------
 * Replaces: nn.Module parameter storage of EGNNDynamics (state-dict layout in
 * oareactdiff_amd/spec.py:state_spec == reference state_dict()).  `params_dev[i]` is the device
 * pointer of the i-th tensor in that canonical order (buffers included; unused tensors may be
 * NULL).  Packs every Linear into MFMA-fragment order (16x16 chunks) plus the
 * padded bias / LayerNorm vectors and the constant inter-object edge row.  Call again after
 * any weight update.
 * The blob ends with room for one table per layer of EquiMessage's rbf_proj as a function of exp(-d) (csrc/oard_rbf_table.h;
 * 3 * ceil(H / 16) * 2049 * 32 floats each, 10.2 MB at H = 196).  oard_pack_weights neither writes nor reads that part - a trainer
 * packs after every update -; the first inference-mode oard_forward on the blob that can use the tables builds and checks them
 * there on its stream and synchronises it once (a call being captured into a graph does not, and runs without them unless an
 * earlier call built them).  Do not copy a blob in place of packing it: the library keeps the tables' state by the blob's address. */
size_t oard_param_count(const oard_config* cfg);
size_t oard_packed_bytes(const oard_config* cfg);
int oard_pack_weights(const oard_config* cfg, const float* const* params_dev, size_t n_params,
                      void* packed_dev, size_t packed_bytes, oard_stream_t stream);

/* ---- topology -------------------------------------------------------------------------------
 * Replaces: what get_edges_index / get_subgraph_mask / compute_frag_index derive from
 * (combined_mask, n_frag_switch) (oa_reactdiff/utils/_graph_tools.py:9-59,
 * egnn_dynamics.py:177-182).  Built once per sample() / batch; host arrays in, device index
 * tables out.  Nodes are given in the reference's order (object-major). */
typedef struct oard_topology oard_topology;

int oard_topology_create(const oard_config* cfg, const int64_t* combined_mask_host,
                         const int64_t* n_frag_switch_host, int64_t n_nodes, oard_topology** out);
/* As oard_topology_create with an explicit number of concurrent sub-batches (0 = the library's choice, see
 * "parts" below).  Training needs 1: the tape and the backward kernels work on one sub-batch. */
int oard_topology_create_parts(const oard_config* cfg, const int64_t* combined_mask_host,
                               const int64_t* n_frag_switch_host, int64_t n_nodes, int parts, oard_topology** out);
void oard_topology_destroy(oard_topology* topo);
int64_t oard_topology_num_nodes(const oard_topology* topo);
int64_t oard_topology_num_edges(const oard_topology* topo);        /* sum n_s (n_s - 1)         */
int64_t oard_topology_num_inner_edges(const oard_topology* topo);  /* same-object ordered pairs */
int64_t oard_topology_num_samples(const oard_topology* topo);
/* Writes 1 to *ok_dev iff edge_index_dev ([2,E] int64, row-major, reference node ids) is the edge SET
 * get_edges_index(combined_mask, remove_self_edge=True) would produce for this topology (utils/_graph_tools.py:30-36),
 * in any order: every ordered pair of distinct nodes of one sample exactly once.  EGNNDynamics.forward accepts any edge_index
 * (egnn_dynamics.py:63-72); its outputs are per node, so any ordering of the complete set is the same computation.
 * Synchronises the stream (once per topology). */
int oard_topology_check_edge_index(const oard_topology* topo, const int64_t* edge_index_dev,
                                   int64_t n_edges, int32_t* ok_dev, oard_stream_t stream);

/* ---- forward --------------------------------------------------------------------------------
 * Replaces: EGNNDynamics.forward(xh, edge_index, t, conditions, n_frag_switch, combined_mask)
 * (egnn_dynamics.py:63-168) including LEFTNet.forward, for update_pocket_coords=True,
 * edge_attr=None.  xh_dev[k] / out_dev[k]: [n_k, node_nf[k]].  t_dev: [B] (one per sample) or,
 * if t_is_scalar, [1].  conditions_dev: [B, condition_nf] (may be NULL when condition_nf==0).
 * status_dev[0] is set to 1 if the predicted displacement contains a NaN
 * (egnn_dynamics.py:138-143 — the caller applies the randn replacement). */
size_t oard_workspace_bytes(const oard_config* cfg, const oard_topology* topo);
int oard_forward(const oard_config* cfg, const oard_topology* topo, const void* packed_dev,
                 const float* const* xh_dev, const float* t_dev, int t_is_scalar,
                 const float* conditions_dev, float* const* out_dev,
                 void* workspace_dev, size_t workspace_bytes, int32_t* status_dev,
                 oard_stream_t stream);

/* ---- confidence score ---------------------------------------------------------------------------
 * Replaces: Confidence._forward(xh, edge_index, t, conditions, n_frag_switch, combined_mask)
 * (oa_reactdiff/dynamics/confidence.py:82-163): LEFTNet.forward with for_conf=True, which returns the node scalars s behind
 * the last layer (model/leftnet.py:875-876), scatter_mean over the nodes of every reaction (confidence.py:157-161) and the
 * GatedMLP readout H -> H -> H -> 1 (confidence.py:74-80, 162; model/core.py:95-131): conf = mlp(g) * sigmoid(gmlp(g)), SiLU behind
 * layers 0 and 1 of both branches.  Inference; the training-mode call and its backward: "training the confidence model" below.
 * Arguments as oard_forward (same packed blob - the output head's weights in it are not read -, same workspace size, same sub-batch
 * streams, same precision bits, same poisoning), without out_dev and with
 *   readout_dev[12]  the raw fp32 tensors readout.{mlp,gmlp}.mlp.{0,1,2}.linear.{weight,bias} in that (state-dict) order,
 *                    weights [out][in] as nn.Linear keeps them, 16-byte aligned (rows are read four floats at a time);
 *   conf_dev         [B] fp32: the logit of the reaction whose combined_mask value is id goes to conf_dev[id].
 * The trunk stops behind the last layer's EquiUpdate; one launch of k_conf_readout (csrc/oard_conf.h) per sub-batch follows: fixed
 * summation order, no atomics - a reaction's value is bit-identical run to run and does not depend on the rest of the batch.
 * status_dev[0] is set to 1 if a written value is NaN.
 * OARD_EINVAL: (hidden, num_radial) is not a built pair, or the reactions' combined_mask values are not exactly 0 .. B - 1 (the
 * reference's scatter_mean would produce rows for the missing ids; its own callers never leave one out). */
int oard_confidence_forward(const oard_config* cfg, const oard_topology* topo, const void* packed_dev,
                            const float* const* readout_dev, const float* const* xh_dev, const float* t_dev, int t_is_scalar,
                            const float* conditions_dev, float* conf_dev, void* workspace_dev, size_t workspace_bytes,
                            int32_t* status_dev, oard_stream_t stream);

/* Inner (same-object) edges that were inside the cutoff in the LAST inference-mode oard_forward on this workspace - the rows
 * EquiMessage actually ran (model/leftnet.py:748-753: the others carry an exactly-zero message and are skipped; equal to
 * oard_topology_num_inner_edges while nothing is masked).  A measurement aid (bench.py charges the roofline with it):
 * synchronises the stream and copies one int per sub-batch.  -1 if the forward did not build the list (training mode, debug
 * option equi_skip = 0). */
int oard_active_inner_edges(const oard_config* cfg, const oard_topology* topo, const void* workspace_dev, size_t workspace_bytes,
                            int64_t* n_active_host, oard_stream_t stream);

/* EquiUpdate's frame-scalar MLP (model/leftnet.py:333, lin3: 3 -> 48 -> 8 -> 1 on (x, 0, 0)) is evaluated from a table that
 * oard_pack_weights builds and CHECKS per layer (csrc/oard_layout.h: L3T_*): this copies layer `layer`'s table - OARD_L3T_FLOATS floats:
 * (f, f' h) at the 1025 grid points of [-16, 16], then [flag, worst midpoint deviation, range of f, -] - to out_dev (tests). */
#define OARD_L3T_FLOATS 2054
int oard_debug_lin3u_table(const oard_config* cfg, const void* packed_dev, int layer, float* out_dev, oard_stream_t stream);

/* ---- sampler step (next row N1) ----------------------------------------------------------------
 * Replaces the element-wise part of EnVariationalDiffusion.sample_p_zs_given_zt / sample_normal /
 * sample_p_xh_given_z0 (oa_reactdiff/diffusion/en_diffusion.py:562-702) and the CoM-free noise of
 * sample_combined_position_feature_noise (:278-305), per object k, rows in the reference's order:
 *   eps      = [ noise_pos - mean_group(noise_pos) | zero_feature_noise ? 0 : noise_feat ]
 *   mode 0:  out = z / a - eps_hat * b + c * eps ;  out_pos -= mean_group(out_pos)     (a = alpha_t|s, b, c = sigma)
 *   mode 1:  out = a * (z - b * eps_hat) + c * eps                                     (a = 1/alpha_0, b = sigma_0, c = sigma_x)
 *   mode 2:  out = eps                                                                 (initial z_T)
 *   mode 3:  out = a * z + c * eps                      (q(z_s | x): noised_representation, :269-287; a = alpha_s, c = sigma_s)
 *   mode 4:  out = a * z + c * eps ;  out_pos -= mean_group(out_pos)   (sample_p_zt_given_zs, :1050-1074; a = alpha_t|s, c = sigma_t|s)
 *   h0_dev[k] != NULL: the feature columns of out are overwritten by h0 (pos_only sampling, :526-530).
 * group = nodes of one object in one sample.  The scalars are host values (the schedule is a host table),
 * so a sampling loop built on this and oard_forward never synchronises. */
int oard_sampler_step(const oard_config* cfg, const oard_topology* topo, int mode,
                      const float* const* z_dev, const float* const* eps_hat_dev, const float* const* noise_dev,
                      const float* const* h0_dev, float a, float b, float c, int zero_feature_noise,
                      float* const* out_dev, oard_stream_t stream);

/* As oard_sampler_step with the three scalars (a, b, c) read from device memory (coef_dev[3]): the launch is then
 * identical for every step, so one captured hipGraph of [oard_forward, oard_sampler_step_dev] replays the whole loop
 * (the host only advances a device-side step index that selects the row of the schedule table). */
int oard_sampler_step_dev(const oard_config* cfg, const oard_topology* topo, int mode,
                          const float* const* z_dev, const float* const* eps_hat_dev, const float* const* noise_dev,
                          const float* const* h0_dev, const float* coef_dev, int zero_feature_noise,
                          float* const* out_dev, oard_stream_t stream);

/* ---- fused RePaint step (next row N3) -----------------------------------------------------------
 * One step of EnVariationalDiffusion.inpaint's loop (oa_reactdiff/diffusion/en_diffusion.py:788-853) in ONE launch per
 * sub-batch: one wavefront per (sample, object) group.  Per object k, rows in the reference's order; eps(n) is the noise n with
 * its position columns made CoM-free per group and its feature columns 0 if zero_feature_noise:
 *   k in fixed:     y = a_s * xfix + sigma_s * eps(noise_known)                                  (q(z_s | x), :803-805)
 *   k not fixed:    y = z / alpha_ts - eps_hat * c_eps + sigma * eps(noise_step) ;  y_pos -= mean_group(y_pos)      (:806-815)
 *   h0_dev[k] != NULL:  the feature columns of y := h0                                           (:817-825)
 *   jump != 0:      out = a_j * y + sigma_j * eps(noise_jump) ;  out_pos -= mean_group(out_pos)  (no h0 override; :848)
 *   else:           out = y
 * coef = [a_s, sigma_s, alpha_ts, c_eps, sigma, jump, a_j, sigma_j]; bit k of fixed_mask set = object k is fixed.
 * Every group sum (the CoM of each noise draw, of the un-projected update, of the jump result) is a float64 sum in a fixed order
 * (lane-strided partials, then a fixed 64-lane reduction), removed in float64: a projected block keeps a mean of at most
 * 2^-24 max|out| whatever the operands' offset, and a group's result does not depend on the sub-batch split.
 * Operands of objects that do not use them may be NULL (z / eps_hat / noise_step of a fixed object, xfix / noise_known of a
 * free one; the arrays themselves when no object needs them).  noise_jump_dev may be NULL only here and only with jump == 0.
 * out_dev[k] must not be one of object k's operands (OARD_EINVAL): the kernel reads whole groups while it writes rows. */
int oard_inpaint_step(const oard_config* cfg, const oard_topology* topo, unsigned int fixed_mask,
                      const float* const* z_dev, const float* const* eps_hat_dev, const float* const* xfix_dev,
                      const float* const* noise_known_dev, const float* const* noise_step_dev,
                      const float* const* noise_jump_dev, const float* const* h0_dev, const float coef[8],
                      int zero_feature_noise, float* const* out_dev, oard_stream_t stream);

/* As oard_inpaint_step with the eight scalars read from device memory (coef_dev[8]), the jump flag among them (a wave-uniform
 * branch): ONE captured launch serves the steps that jump and those that do not.  noise_jump_dev is required. */
int oard_inpaint_step_dev(const oard_config* cfg, const oard_topology* topo, unsigned int fixed_mask,
                          const float* const* z_dev, const float* const* eps_hat_dev, const float* const* xfix_dev,
                          const float* const* noise_known_dev, const float* const* noise_step_dev,
                          const float* const* noise_jump_dev, const float* const* h0_dev, const float* coef_dev,
                          int zero_feature_noise, float* const* out_dev, oard_stream_t stream);

/* ---- introspection (tests / profiling) --------------------------------------------------------
 * Copies an intermediate tensor of the LAST oard_forward on this workspace into dst_dev, in the
 * reference's node / edge order, dense [rows, cols] fp32.  `which`: see OARD_TAP_*.  `layer`
 * selects nothing yet (taps hold the state after the final layer) and must be 0. */
#define OARD_TAP_S 1          /* [N, H]      node scalars s after the last layer            */
#define OARD_TAP_VEC 2        /* [N, 3*H]    node vectors after the last layer              */
#define OARD_TAP_EDGE 3       /* [E, 3H+R]   edge state after the last layer                */
#define OARD_TAP_POS_FRAME 4  /* [N, 3]                                                     */
#define OARD_TAP_DPOS 5       /* [N, 3]      LEFTNet displacement before CoM removal        */
#define OARD_TAP_HOUT 6       /* [N, in_hidden]                                             */
#define OARD_TAP_LABELS 7     /* [N, 1]      frame-group label (as float, reference-order id of the group's first node) */
#define OARD_TAP_NE1 8         /* [N, 3*H]    CFConvS2V output (leftnet.py:791)              */
int oard_tap(const oard_config* cfg, const oard_topology* topo, const void* workspace_dev,
             int which, int layer, float* dst_dev, oard_stream_t stream);

/* Debug: make oard_forward return right after a stage so the taps expose intermediate state.
 * 0 = run everything (default); 1 = after the init stages (s = NeighborEmb output, edge state =
 * initial edgeweight); 100 + 10*l + 1 = after layer l's GCL node update; 100 + 10*l + 2 = after
 * layer l's EquiUpdate. */
int oard_debug_stop_after(int code);
/* Process-wide switches for tests and A/B measurements (defaults in brackets; all variants compute the same
 * function and have their own parity test):
 *   "gcl_variant" [2]   GCLMessage edge kernel: 0 = weights straight from L2 (v0, the simple cross-check kernel),
 *                       2 = LDS-streamed, 8 waves x 16 edges, 3 = the same with 4 waves (small launches)
 *                       (oard_edge_v1.h), 6 = latency kernel (oard_edge_small.h)
 *   "equi_variant" [2]  EquiMessage edge kernel: 0 = v0, 2 / 1 = LDS-streamed with 8 / 4 waves, 4 = latency kernel
 *   "node_variant" [1]  0 = one wave per 16 nodes (v0), 1 = one wave per hidden tile (oard_node_v1.h)
 *   "gcl_skip" [1]      skip S1 / S3 of the GCL chain on inter-object rows of the first / last layer
 *   "auto_small" [4], "auto_tiny" [8]  launch-shape heuristics: launches of <= 1024*auto_small (GCL) /
 *                       512*auto_small (Equi) 16-edge tiles use 4-wave workgroups, launches of <= 512*auto_tiny
 *                       tiles the latency kernels; 0 = always the throughput shape
 *   "npb" [0]           real nodes per workgroup of the node stages (0 = ceil(N/256) clamped to 1..16); read by
 *                       oard_topology_create
 *   "parts" [0]         sub-batches per topology (0 = 4 for B >= 32, 2 for B >= 16, else 1); read by
 *                       oard_topology_create;  "sequential" [0] = 1 runs them one after the other
 *   "poison" [0]        1 fills the workspace with NaN bit patterns before every forward (the tests use it to
 *                       prove that nothing depends on workspace contents)
 *   "wgrad_wgs" [512]   workgroups per weight-gradient GEMM (oard_wgrad): row chunks x task groups
 *   "small_split" [128] EquiMessage latency kernel: launches of <= this many 16-edge tiles run one launch per dense stage
 *                       (k_equi_small_s1 / _s2, a tile spread over several CUs); 0 = never */
int oard_debug_option(const char* name, int value);

/* Average duration (ms) and launch count per kernel family since the last reset, measured with
 * HIP events on the launch stream when timing is enabled (bench.py's roofline leg).
 * names: "gcl_edge", "equi_edge", "node", "init", "other" (forward), "gcl_edge_bwd", "equi_edge_bwd", "wgrad" (backward). */
int oard_timing_enable(int on);
int oard_timing_reset(void);
int oard_timing_get(const char* family, double* total_ms, int64_t* launches);

/* ---- training (next row N2): tape, backward of the edge stages ---------------------------------------
 * Replaces: torch autograd through GCLMessage / EquiMessage when DDPMModule.training_step
 * (oa_reactdiff/trainer/pl_trainer.py:327-347) back-propagates the loss of EnVariationalDiffusion.forward
 * (oa_reactdiff/diffusion/en_diffusion.py:56-248).  The reference has no hand-written backward.
 * All of this works on topologies created with parts == 1.
 *
 * oard_forward_train = oard_forward that additionally fills `tape_dev` (oard_tape_bytes) with what the
 * backward pass needs: the edge state entering every layer, the pre-activations of the edge MLPs, the node
 * state at the layer boundaries and the geometry constants.  oard_tape_entry locates one tensor in the tape
 * (byte offset, rows, floats per row); rows are in the library's internal order: nodes sample-major
 * (oard_topology_export NODE_REF maps them to the reference's rows), edges as physical rows (inner edges
 * first, target-sorted == INNER_SRC/INNER_TGT, then inter-object edges; ROW_SRC/ROW_TGT), feature widths
 * padded to multiples of 16 with zero pads (H -> HP, 3H+R -> WP, ...). */
#define OARD_TOPO_NODE_REF 1     /* [N] internal node -> row in the reference's (object-major) order            */
#define OARD_TOPO_NODE_OBJ 2     /* [N] object index                                                          */
#define OARD_TOPO_NODE_ROW 3     /* [N] row inside xh[object]                                                 */
#define OARD_TOPO_NODE_SAMPLE 4  /* [N] dense sample index                                                    */
#define OARD_TOPO_NODE_TIDX 5    /* [N] combined_mask value (row of t / conditions)                           */
#define OARD_TOPO_SAMPLE_PTR 6   /* [B+1] node range of every sample                                          */
#define OARD_TOPO_GROUP_PTR 7    /* [B*n_obj+1] node range of every (sample, object) group                    */
#define OARD_TOPO_INNER_SRC 8    /* [A] source node of inner edge a (rows sorted by target)                   */
#define OARD_TOPO_INNER_TGT 9    /* [A]                                                                       */
#define OARD_TOPO_ROW_SRC 10     /* [E] source node of physical edge row r                                    */
#define OARD_TOPO_ROW_TGT 11     /* [E]                                                                       */
int oard_topology_export(const oard_topology* topo, int which, int32_t* dst_dev, int64_t capacity,
                         oard_stream_t stream);

#define OARD_TAPE_HIN 1      /* [N][16]      encoder output | t | conditions  (LEFTNet input h)              */
#define OARD_TAPE_GEO 2      /* [A+1][12]    per inner edge: d, env, u[3], c[3], v[3], mask                   */
#define OARD_TAPE_RBF 3      /* [A+1][RP]    radial basis                                                     */
#define OARD_TAPE_PP0 4      /* [N][1]       pos_prjt[:, 0]                                                   */
#define OARD_TAPE_X1 5       /* [N][3]       node frame axis x1                                               */
#define OARD_TAPE_S_IN 16    /* [N][HP]      s entering layer l          (l = L: after the last layer)        */
#define OARD_TAPE_VEC_IN 17  /* [N][3][HP]   vec entering layer l        (l = L: after the last layer)        */
#define OARD_TAPE_EW 18      /* [E+1][WP]    edge state entering layer l (l = L: final; inter-object rows of l = 0
                                             are the constant row and are not materialised)                   */
#define OARD_TAPE_AGG 19     /* [N][HP]      mean gated message per source node                               */
#define OARD_TAPE_S_MID 20   /* [N][HP]      s after the GCL node update                                      */
#define OARD_TAPE_Z1 21      /* [E+1][HP]    edge_mlp.0 pre-activation                                        */
#define OARD_TAPE_Z2 22      /* [E+1][HP]    edge_mlp.1 pre-activation                                        */
#define OARD_TAPE_ATT 23     /* [E+1][1]     att_mlp pre-activation                                           */
#define OARD_TAPE_Z3 24      /* [E+1][WP]    edge_out_trans pre-activation                                    */
#define OARD_TAPE_ZD1 25     /* [A+1][D1P]   dir_proj.0 pre-activation                                        */
#define OARD_TAPE_CD 26      /* [A+1][3][HP] dir_proj output (before the product with rbf_proj)               */
#define OARD_TAPE_S_A 27     /* [N][HP]      s after the EquiMessage aggregation, (s + dx)/sqrt2 (EquiUpdate input) */
#define OARD_TAPE_VEC_A 28   /* [N][3][HP]   vec after the EquiMessage aggregation (EquiUpdate input)          */
size_t oard_tape_bytes(const oard_config* cfg, const oard_topology* topo);
int oard_tape_entry(const oard_config* cfg, const oard_topology* topo, int which, int layer,
                    size_t* offset_bytes, int64_t* rows, int64_t* row_floats);
int oard_forward_train(const oard_config* cfg, const oard_topology* topo, const void* packed_dev,
                       const float* const* xh_dev, const float* t_dev, int t_is_scalar,
                       const float* conditions_dev, float* const* out_dev,
                       void* workspace_dev, size_t workspace_bytes, void* tape_dev, size_t tape_bytes,
                       int32_t* status_dev, oard_stream_t stream);

/* Transposed weight streams of the two backward edge kernels (same params_dev convention as
 * oard_pack_weights); call again after any weight update. */
size_t oard_packed_bwd_bytes(const oard_config* cfg);
int oard_pack_weights_bwd(const oard_config* cfg, const float* const* params_dev, size_t n_params,
                          void* packed_bwd_dev, size_t packed_bytes, oard_stream_t stream);

/* Adjoint of layer `layer`'s GCLMessage edge part (leftnet.py:162-170 + the mean aggregation :172-180).
 *   in : dagg_dev [N][HP]    gradient w.r.t. the per-node mean message (pads zero)
 *        dew_dev  [E+1][WP]  gradient w.r.t. the edge state LEAVING the layer (pads and spare row finite)
 *   out: dew_dev             gradient w.r.t. the edge state ENTERING the layer (in place)
 *        dz3_dev [E+1][WP], dz2_dev / dz1_dev [E+1][HP], da_dev [E+1]: gradients w.r.t. the pre-activations
 *        of edge_out_trans, edge_mlp.1, edge_mlp.0, att_mlp;  mout_dev [E+1][HP]: the gated message m,
 *        all in physical row order - the operands of the weight-gradient GEMMs (oard_wgrad).
 *   Last layer: dz3 is produced for the inner rows [0, A) only (the forward skips edge_out_trans on
 *   inter-object rows there). */
int oard_gcl_backward_dx(const oard_config* cfg, const oard_topology* topo, const void* packed_bwd_dev, int layer,
                         const void* tape_dev, const float* dagg_dev, float* dew_dev, float* dz3_dev,
                         float* mout_dev, float* dz2_dev, float* da_dev, float* dz1_dev, oard_stream_t stream);
/* dP[n] / dQ[n] = sum of dz1 over the edges whose source / target is node n (the node halves of edge_mlp.0). */
int oard_edge_node_sums(const oard_config* cfg, const oard_topology* topo, const float* dz1_dev,
                        float* dP_dev, float* dQ_dev, oard_stream_t stream);
/* Adjoint of layer `layer`'s EquiMessage edge part (leftnet.py:247-249, dir_proj):
 *   in : dcd_dev [A+1][3][HP] gradient w.r.t. dir_proj's output;  out: dew_dev rows [0, A) += dir_proj.0^T ...,
 *        dzd1_dev [A+1][D1P] gradient w.r.t. dir_proj.0's pre-activation. */
int oard_equi_backward_dx(const oard_config* cfg, const oard_topology* topo, const void* packed_bwd_dev, int layer,
                          const void* tape_dev, const float* dcd_dev, float* dew_dev, float* dzd1_dev,
                          oard_stream_t stream);
/* Adjoint of EquiMessage's message formation + aggregation (leftnet.py:264-283, the gather half of k_equi_node_v1):
 *   in : xq_dev [N][3][H] x_proj output, cr_dev [A][3][H] rbf_proj(rbf), gx_dev [N][H] / gv_dev [N][3][H] gradients w.r.t. the
 *        aggregated scalar / vector messages (dense, unpadded);  vec_in, dir_proj's output and the edge frames come from the tape
 *   out: dcd_dev / dcr_dev [A+1][3][HP] gradients w.r.t. dir_proj's output / rbf_proj's output (pads untouched: pass zeroed
 *        buffers), dxq_dev [N][3][H], dvec_dev [N][3][H] (gradient w.r.t. vec entering the layer, identity path included). */
int oard_equi_msg_backward(const oard_config* cfg, const oard_topology* topo, const void* tape_dev, int layer,
                           const float* xq_dev, const float* cr_dev, const float* gx_dev, const float* gv_dev,
                           float* dcd_dev, float* dcr_dev, float* dxq_dev, float* dvec_dev, oard_stream_t stream);
/* EquiUpdate's frame-scalar MLP lin3 (leftnet.py:304-310, 333: Linear(3,48) SiLU Linear(48,8) SiLU Linear(8,1) on (x, 0, 0)) as a
 * differentiable op on n = N*H items (training; the inference forward fuses it into k_equi_node_v1).
 *   forward : out[i] = lin3(x[i], 0, 0)
 *   backward: dx[i], and per item the operands of the weight gradients for oard_wgrad:
 *             xa [n][4] = (x, 1, 0, 0), h1 [n][48], dz1 [n][48], dz2 [n][8], h2a [n][12] = dout * (h2[8], 1, 0, 0, 0)
 *             (lin3.0: dz1^T xa -> [48][4] = (d weight[:,0] | d bias);  lin3.2: dz2^T h1, bias = column sums of dz2;
 *              lin3.4: column sums of h2a = (d weight[8] | d bias)). */
int oard_lin3u_forward(const oard_config* cfg, const void* packed_dev, int layer, const float* x_dev, int64_t n,
                       float* out_dev, oard_stream_t stream);
int oard_lin3u_backward(const oard_config* cfg, const void* packed_dev, int layer, const float* x_dev, const float* dout_dev,
                        int64_t n, float* dx_dev, float* xa_dev, float* h1_dev, float* dz1_dev, float* h2a_dev,
                        float* dz2_dev, oard_stream_t stream);
/* Adjoint of the edge scalarisation + lin3 (leftnet.py:792-806, k_scalarize): from the gradient of the initial edge state
 * (dew_dev [E+1][WP], columns [0, 2H) of the inner rows) and NE1 (ne1_dev [N][3][ld], ld >= H, the CFConvS2V output) to
 *   dne1_dev [N][3][ld]     gradient w.r.t. NE1
 *   part_dev [N][5*(H/4)+1] per-node partial sums of the lin3 gradients: lin3.0.weight [H/4][3] | lin3.0.bias [H/4] |
 *                           lin3.2.weight [H/4] | lin3.2.bias [1]  (the caller adds the N rows up)
 * packed_dev: oard_pack_weights blob (lin3 weights), tape_dev: the forward's tape (edge frames). */
int oard_scalarize_backward(const oard_config* cfg, const oard_topology* topo, const void* packed_dev, const void* tape_dev,
                            const float* ne1_dev, int ld, const float* dew_dev, float* dne1_dev, float* part_dev,
                            oard_stream_t stream);
/* Weight gradient of a Linear layer from row-major operands (nn.Linear backward, dW = dY^T X, db = sum dY):
 *   dW[o][i] = sum_{r < rows} dY[r][op(o)] * act(X[r][ip(i)]),   db[o] = sum_r dY[r][op(o)]   (db may be NULL)
 * op(o) = (o / o_len) * o_pad + o % o_len undoes section padding (e.g. three 196-wide thirds stored 208 apart);
 * ncY / ncX = readable floats per row (multiples of 4, <= ld);  x_silu != 0 applies SiLU to X on load.
 * Deterministic: fixed chunking and summation order for a given shape. */
size_t oard_wgrad_scratch_bytes(int ncY, int ncX, int64_t rows);
int oard_wgrad(const float* dY_dev, int ldY, int ncY, int o_len, int o_pad, int MO,
               const float* X_dev, int ldX, int ncX, int x_silu, int i_len, int i_pad, int MI, int64_t rows,
               float* dW_dev, float* db_dev, void* scratch_dev, size_t scratch_bytes, oard_stream_t stream);

/* ---- The whole reverse sweep on the device (round 3) -------------------------------------------------------------------------
 * Replaces torch autograd through the node-side / init / output stages of LEFTNet.forward (oa_reactdiff/model/leftnet.py:
 * EquiUpdate :325-346, GCL node update :172-183, x_proj :245, pos_expansion + LayerNorm + edge_mlp.0 node halves :840-841,158,168,
 * output block :566-576,878-891, init head :744,781-809) and of the wrapper (egnn_dynamics.py:91-119 encoders, :137-160 velocity /
 * CoM / decoders).  Every entry reads the tape of oard_forward_train and ACCUMULATES parameter gradients into `grads_dev`:
 * a table of device pointers in the canonical parameter order of oard_pack_weights (nn.Linear shapes; NULL entries are skipped;
 * encoders / decoders shared by several objects simply appear several times).  `params_dev` is the same table for the weights
 * themselves.  Node cotangents are [N][HP] / [3N][HP] float32 with zero pads, the edge-state cotangent is [E+1][WP].  All scratch
 * is the caller's (`oard_train_scratch_bytes`); nothing synchronises, and the library's own job tables (the grouped weight-gradient
 * launches) travel through a ring of pinned / device slots that is allocated once per device, at its first use.  `packed_bwd_dev` = oard_pack_weights_bwd.
 *   oard_train_tail_backward   grad_out[k] ([n_k][node_nf_k], reference rows; NULL = zero) -> ds, dvec of the final node state
 *   oard_train_layer_backward  one layer: ds / dvec / dew in place (cotangents of the layer's outputs -> of its inputs)
 *   oard_train_init_backward   ds0, dew (cotangents of the state entering layer 0) -> init-head and encoder gradients
 *   oard_train_stage_backward  one stage of a layer in isolation (teacher-forced tests); RECOMPUTE first */
#define OARD_STAGE_RECOMPUTE 0
#define OARD_STAGE_UPDATE 1      /* in: ds, dvec          out: gs_a, gvec_a       */
#define OARD_STAGE_MESSAGE 2     /* in: gs_a, gvec_a      out: gx, dxq, dvec_in   */
#define OARD_STAGE_GCL_NODE 3    /* in: gx, dxq           out: dxh, dagg          */
#define OARD_STAGE_NODE_PRE 4    /* in: dxh, dP, dQ       out: ds_in              */
#define OARD_STAGE_GCL_EDGE 5    /* in: dagg              in/out: dew (out0)      out: dP, dQ   (+ every GCLMessage edge-MLP gradient) */
#define OARD_STAGE_EQUI_EDGE 6   /* in: dcd [A+1][3HP]    in/out: dew (out0)      (+ dir_proj gradients)  */
#define OARD_SCRATCH_XH 1
#define OARD_SCRATCH_XQ 2
#define OARD_SCRATCH_CR 3
#define OARD_SCRATCH_DCD 4
#define OARD_SCRATCH_DCR 5
size_t oard_train_scratch_bytes(const oard_config* cfg, const oard_topology* topo);
int oard_train_scratch_poison(const oard_config* cfg, const oard_topology* topo, void* scratch_dev, size_t scratch_bytes,
                              oard_stream_t stream);
int oard_train_scratch_entry(const oard_config* cfg, const oard_topology* topo, int which, size_t* offset_bytes, int64_t* rows,
                             int64_t* row_floats);
int oard_train_tail_backward(const oard_config* cfg, const oard_topology* topo, const void* packed_dev, const void* packed_bwd_dev,
                             const void* tape_dev, const float* const* grad_out_dev, float* ds_dev, float* dvec_dev,
                             const float* const* params_dev, float* const* grads_dev, void* scratch_dev, size_t scratch_bytes,
                             oard_stream_t stream);
int oard_train_layer_backward(const oard_config* cfg, const oard_topology* topo, const void* packed_dev, const void* packed_bwd_dev,
                              const void* tape_dev, int layer, float* ds_dev, float* dvec_dev, float* dew_dev,
                              const float* const* params_dev, float* const* grads_dev, void* scratch_dev, size_t scratch_bytes,
                              oard_stream_t stream);
int oard_train_init_backward(const oard_config* cfg, const oard_topology* topo, const void* packed_dev, const void* packed_bwd_dev,
                             const void* tape_dev, const float* const* xh_dev, const float* ds0_dev, const float* dew_dev,
                             const float* const* params_dev, float* const* grads_dev, void* scratch_dev, size_t scratch_bytes,
                             oard_stream_t stream);
int oard_train_stage_backward(const oard_config* cfg, const oard_topology* topo, const void* packed_dev, const void* packed_bwd_dev,
                              const void* tape_dev, int layer, int stage, const float* in0, const float* in1, const float* in2,
                              float* out0, float* out1, float* out2, const float* const* params_dev, float* const* grads_dev,
                              void* scratch_dev, size_t scratch_bytes, oard_stream_t stream);

/* The reference's NaN guard (egnn_dynamics.py:138-143) without its host sync: if `status_dev[0]` (written by oard_forward) is set,
 * the velocity columns of every out[k] are replaced by noise[k] ([n_k][3] N(0,1) draws of the caller) minus its per-(sample, object)
 * mean; otherwise nothing is written.  Asynchronous on `stream`. */
int oard_nan_replace(const oard_config* cfg, const oard_topology* topo, const int32_t* status_dev, const float* const* noise_dev,
                     float* const* out_dev, oard_stream_t stream);

/* ---- training the confidence model ---------------------------------------------------------------------------------------------
 * Replaces: torch autograd through Confidence._forward (oa_reactdiff/dynamics/confidence.py:82-163) when ConfModule.training_step
 * (oa_reactdiff/trainer/pl_trainer.py:554-617) back-propagates its BCE / MSE loss.  The reference has no hand-written backward.
 *
 * oard_confidence_forward_train: oard_forward_train's arguments without out_dev, plus readout_dev[12] and conf_dev [B] as in
 * oard_confidence_forward.  The training-mode trunk with the tape written (cfg.precision handed through unchanged) stops behind the last
 * layer's EquiUpdate; k_conf_readout then runs on the tape's S_IN[L].  OARD_EINVAL as for oard_confidence_forward (unbuilt width pair,
 * reaction ids not exactly 0 .. B - 1, a missing or misaligned readout tensor) and, like oard_forward_train, for a topology of more
 * than one sub-batch.
 *
 * oard_confidence_tail_backward: the confidence counterpart of oard_train_tail_backward, the first call of a sweep; then
 * oard_train_layer_backward for l = L-1 .. 0 and oard_train_init_backward as for the denoiser (they take the final edge state's
 * cotangent as zero; the last layer's vec-side adjoints run on dvec = 0).
 *   in : tape_dev           the tape of oard_confidence_forward_train
 *        readout_dev[12]    as above
 *        dconf_dev [B]      fp32, d loss / d logit, indexed by the reaction's combined_mask value like conf_dev
 *   out: ds_dev [N][HP]     cotangent of the final node scalars: dg / n_b in the columns < H of every node of reaction b, exact zeros
 *                           in the pad columns (the buffer may arrive uninitialised)
 *        dvec_dev [3N][HP]  exact zeros (nothing flows into vec under for_conf)
 *        readout_grads_dev[12]  nn.Linear shapes in readout_dev's order; NULL entries are skipped; ACCUMULATED into, like grads_dev
 * Two launches on `stream` (csrc/oard_conf_bwd.h): k_conf_readout_bwd, one workgroup per reaction, recomputes the readout in float64
 * from the taped s (no extra tape entry, pad columns of s never read) and leaves the weight gradients' operands in the scratch;
 * k_conf_wgrad sums them over the reactions in ascending order in float64 and adds once, in float32, into the destination.  No atomics:
 * bit-identical run to run.  scratch_dev: the sweep's scratch (oard_train_scratch_bytes covers the 72 H + 16 bytes per reaction this
 * call uses; OARD_ENOMEM otherwise), poisoned first under the "poison" debug option.  Nothing synchronises. */
int oard_confidence_forward_train(const oard_config* cfg, const oard_topology* topo, const void* packed_dev,
                                  const float* const* readout_dev, const float* const* xh_dev, const float* t_dev, int t_is_scalar,
                                  const float* conditions_dev, float* conf_dev, void* workspace_dev, size_t workspace_bytes,
                                  void* tape_dev, size_t tape_bytes, int32_t* status_dev, oard_stream_t stream);
int oard_confidence_tail_backward(const oard_config* cfg, const oard_topology* topo, const void* tape_dev,
                                  const float* const* readout_dev, const float* dconf_dev, float* ds_dev, float* dvec_dev,
                                  float* const* readout_grads_dev, void* scratch_dev, size_t scratch_bytes, oard_stream_t stream);

/* ---- The training caller around the network call, fused (round 3) --------------------------------------------------------------
 * oard_loss_prepare  EnVariationalDiffusion.forward up to the network call (en_diffusion.py:56-123, noised_representation :250-281,
 *                    sample_combined_position_feature_noise :283-306): normalises the dataset-layout batch (pos float32 [n_k][3],
 *                    one_hot int64 [n_k][nf_k-4], charge int64 [n_k][1]; reference rows), removes the per-(sample, object) CoM of the
 *                    raw N(0,1) position noise, z_t = alpha_t x + sigma_t eps with gamma = gamma_table[t_int[b]].
 * oard_loss_terms    the rest of it + DDPMModule.compute_loss (pl_trainer.py:208-282, l2 training form): per-sample nll [B], logged
 *                    terms [2 n_obj][B] (normalised and un-normalised error per object) and d(mean_b nll)/d(network output).
 *                    An empty (sample, object) group contributes 0 to nll and gets exact zeros in its two `terms` entries (the
 *                    reference divides by the group's size there and yields NaN).
 * oard_adamw_step    torch.optim.AdamW(amsgrad) (pl_trainer.py:150) over one flat bucket, gradient-clipping factor folded in.
 * norm_values / norm_biases [3], scales [n_obj]: host arrays.  t_int [B] float32 (device), gamma table [T+1] (device). */
int oard_loss_prepare(const oard_config* cfg, const oard_topology* topo, const float* const* pos_dev, const int64_t* const* one_hot_dev,
                      const int64_t* const* charge_dev, const float* const* noise_dev, const float* t_int_dev, const float* gamma_dev,
                      int T, const float* norm_values, const float* norm_biases, int pos_only, int fixed_mask, float* const* z_dev,
                      float* const* eps_dev, oard_stream_t stream);
int oard_loss_terms(const oard_config* cfg, const oard_topology* topo, const float* const* eps_dev, const float* const* net_dev,
                    const float* const* z_dev, const int64_t* const* one_hot_dev, const int64_t* const* charge_dev,
                    const float* t_int_dev, const float* gamma_dev, int T, const float* norm_values, const float* norm_biases,
                    const float* scales, int pos_only, int B, float* nll_dev, float* terms_dev, float* const* dnet_dev,
                    oard_stream_t stream);
int oard_adamw_step(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* max_exp_avg_sq_dev,
                    int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, int amsgrad,
                    double grad_scale, oard_stream_t stream);

/* ---- The evaluation half of the loss: the variational bound of a validation batch (csrc/oard_loss_eval.h) ---------------------------
 * oard_loss_prepare / oard_loss_terms above are the l2 training form only.  These two are the `not self.training` branch of
 * EnVariationalDiffusion.forward (en_diffusion.py:56-248: a separate t = 0 call on its own noise, :181-199) and the `vlb` form of
 * DDPMModule.compute_loss (pl_trainer.py:246-282), with TWO inference network calls (at t and at 0) between them.
 * oard_loss_eval_prepare  en_diffusion.py:56-123 and :181-186 (noised_representation :250-281, sample_combined_position_feature_noise
 *                    :283-306, both times) in ONE launch: normalises the dataset-layout batch once, removes the per-(sample, object) CoM
 *                    of each of the two raw N(0,1) noise blocks, z_t = alpha_t x + sigma_t eps_t with gamma_t = gamma_table[t_int[b]],
 *                    z_0 = alpha_0 x + sigma_0 eps_0 with gamma_0 = gamma_table[0].  pos_only / fixed_mask zero the noise exactly as
 *                    oard_loss_prepare does.
 * oard_loss_eval_terms    en_diffusion.py:125-248 (helpers :308-449) + pl_trainer.py:246-282: per-sample
 *                      nll [B] = sum_k(-T/2 SNR_weight error_t_k) + sum_k(loss_0_x + loss_0_cat + loss_0_charge)_k + neg_log_constants
 *                                - delta_log_px                                   (kl_prior = log_pN = 0), summed in double, rounded once
 *                    and terms [5 n_obj + 2][B] with K = n_obj: rows [0, K) error_t per object normalised and scaled (info["error_t_k"]
 *                    is its mean / (scales[k] + 1e-4)), [K, 2K) error_t un-normalised, [2K, 3K) loss_0_x, [3K, 4K) loss_0_cat, [4K, 5K)
 *                    loss_0_charge, row 5K SNR_weight, row 5K + 1 neg_log_constants.  `B` is the row stride of `terms`; a call owns the
 *                    columns its t_int rows name, so a part of a larger table passes terms_dev + col0 (as oard_loss_terms).  error_t is
 *                    not masked and EVERY sample gets the t = 0 likelihood terms on z_0.  An empty (sample, object) group contributes 0
 *                    and gets exact zeros in its five entries; only the normalised row divides by a size.
 * snr_dev [T+1] (device, float32): SNR_weight per time step, 1 - exp(-(gamma[t-1] - gamma[t])) evaluated by the HOST in float64 and
 * rounded once (in float32 most digits of the ~1e-3 difference cancel).  Entry 0 is never read for valid input: in evaluation t_int lies
 * in [1, T].  Every index into the gamma and SNR tables is clamped into [0, T], so an out-of-contract t_int reads no other memory.
 * delta_log_px: the host scalar -(N_atoms_of_the_batch - 1) * 3 * log(norm_values[0]) (en_diffusion.py:87-89: the whole-batch quantity).
 * Returned before any HIP call, with OARD_EINVAL: a null table or pointer list, B < 1, T < 1, n_obj outside [1, OARD_MAX_OBJECTS],
 * node_nf - 4 outside [1, 16], an unbuilt configuration, a topology of more than one sub-batch. */
int oard_loss_eval_prepare(const oard_config* cfg, const oard_topology* topo, const float* const* pos_dev,
                           const int64_t* const* one_hot_dev, const int64_t* const* charge_dev, const float* const* noise_t_dev,
                           const float* const* noise_0_dev, const float* t_int_dev, const float* gamma_dev, int T,
                           const float* norm_values, const float* norm_biases, int pos_only, int fixed_mask, float* const* z_t_dev,
                           float* const* eps_t_dev, float* const* z_0_dev, float* const* eps_0_dev, oard_stream_t stream);
int oard_loss_eval_terms(const oard_config* cfg, const oard_topology* topo, const float* const* eps_t_dev,
                         const float* const* net_t_dev, const float* const* eps_0_dev, const float* const* net_0_dev,
                         const float* const* z_0_dev, const int64_t* const* one_hot_dev, const int64_t* const* charge_dev,
                         const float* t_int_dev, const float* gamma_dev, const float* snr_dev, int T, const float* norm_values,
                         const float* norm_biases, const float* scales, int pos_only, double delta_log_px, int B, float* nll_dev,
                         float* terms_dev, oard_stream_t stream);

/* The optimiser step WITHOUT a host round trip (round 4): the adaptive clipping decision of pl_trainer.py:391-418 (max_norm = 1.5 mean +
 * 3 std of the last <= `capacity` gradient norms, utils/training_tools.py:6-23) taken by one device thread, then AdamW with the scalars it
 * derived.  clip_state (device, doubles, 4 + capacity + 8 entries): [0] entries in the history, [1] optimiser steps taken so far, [2] steps
 * skipped so far, [3] reserved, [4 ..) the history, newest first; the caller initialises [0 .. 4 + capacity) and may read it back at any time.
 * grad_norm / flag (device, float): the gradient's 2-norm and the non-finite flag of the step (flag != 0 or a non-finite norm: the step is
 * skipped - parameters, moments, history and step count untouched, [2] counts it).  clip = 0: no clipping (history untouched).
 * out4 (device, float[4]): grad_norm, max_norm (NaN when not clipping / skipped), the clipping factor applied, 1 if skipped. */
int oard_adamw_step_dev(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* max_exp_avg_sq_dev,
                        int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay, int amsgrad, int clip,
                        double* clip_state_dev, int capacity, const float* grad_norm_dev, const float* flag_dev, float* out4_dev,
                        oard_stream_t stream);

/* The exponential moving average of the weights, updated after every batch (trainer/ema.py:37-47: EMACallback.on_train_batch_end ->
 * timm's ModelEmaV2.update, wired in trainer/train_ts1x.py:188-189), in float32:
 *     ema[i] = fl(fl(d32 ema[i]) + fl(w32 param[i])),  d32 = (float)ema_decay, w32 = (float)(1.0 - ema_decay)
 * - two rounded products and one add, no fused multiply-add: the bits torch gives for `decay * e + (1. - decay) * m`.  `ema_decay` is
 * timm's decay, the weight of the OLD average (the reference's EMACallback(decay=x) passes 1 - x, ema.py:29).  ema_dev: n floats that do
 * not overlap param_dev.  A null ema_dev or a decay outside [0, 1] returns OARD_EINVAL and launches nothing.
 * oard_adamw_step_ema / oard_adamw_step_dev_ema: oard_adamw_step / oard_adamw_step_dev (same arguments, same parameters and moments bit
 * for bit) with the line above applied to the freshly stepped parameter in the same kernel - no extra launch; a skipped step
 * (oard_adamw_step_dev_ema) leaves the average untouched like everything else.
 * oard_ema_update: the line alone, for callers that step the weights by other means.  Asynchronous on `stream`. */
int oard_adamw_step_ema(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* max_exp_avg_sq_dev,
                        int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, int amsgrad,
                        double grad_scale, float* ema_dev, double ema_decay, oard_stream_t stream);
int oard_adamw_step_dev_ema(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* max_exp_avg_sq_dev,
                            int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay, int amsgrad, int clip,
                            double* clip_state_dev, int capacity, const float* grad_norm_dev, const float* flag_dev, float* out4_dev,
                            float* ema_dev, double ema_decay, oard_stream_t stream);
int oard_ema_update(float* ema_dev, const float* param_dev, int64_t n, double ema_decay, oard_stream_t stream);

/* ---- validation metric: optimal-superposition RMSD per molecule ------------------------------------------------------------------
 * Replaces: the same-order Kabsch fit of rmsd_core (oa_reactdiff/analyze/rmsd.py:30-35, pymatgen's KabschMatcher), the chirality
 * handling of pymatgen_rmsd and the per-molecule loop of batch_rmsd (:54-100), which DDPMModule.eval_inplaint_batch logs
 * (trainer/pl_trainer.py:284-325).  Rows are compared in the order given, an upper bound on the order-matched number; the permutation
 * search over like atoms of rmsd_core's other branch (:36-51) is oard_matched_rmsd below.
 * Segment g is rows seg_ptr[g] .. seg_ptr[g + 1] (seg_ptr_dev: n_segments + 1 ascending int32) of a_dev and b_dev: row-major float32
 * with row strides lda / ldb >= 3 in ELEMENTS, coordinates in the first three columns (the other columns are never read, so the
 * [n, node_nf] tensors of the samplers are passed as they are).  One wavefront per segment (csrc/oard_kabsch.h); float64 throughout:
 * fixed-order sums (bitwise reproducible, independent of the other segments of the launch), Horn's quaternion matrix diagonalised by
 * cyclic Jacobi (n = 1, 2, collinear, coplanar and identical structures included), the RMSD as the residual of a second pass,
 *     rmsd[g] = sqrt(sum_rows |R (b - c_b) - (a - c_a)|^2 / n),     R the proper rotation minimising it.
 * flags bit 0 (allow reflection, the reference's ignore_chirality=True): the fit is repeated with the z column of the centred b negated
 * and the smaller RMSD kept, with its improper map.  cap > 0: rmsd = min(rmsd, cap) (the reference's min(rmsd, 1.0)).
 * An empty segment gives NaN; a segment with a non-finite coordinate gives cap if cap > 0, else NaN (the reference's `except: 1.0`);
 * their rot / aligned entries are NaN.
 * rot_dev (or NULL): [n_segments, 9] row-major 3 x 3, the map taking centred b onto centred a (reflection folded in when chosen).
 * aligned_dev (or NULL): [rows, 3], row r = rot (b_r - c_b) + c_a with rot as returned (rounded to float32): b in a's frame.
 * OARD_EINVAL for null a / b / seg_ptr / rmsd, n_segments < 0, lda < 3 or ldb < 3; n_segments == 0 returns OARD_OK without a launch.
 * Needs no oard_config and no topology (production and general path alike); no allocation, asynchronous on `stream`, capturable. */
int oard_kabsch_rmsd(const float* a_dev, int64_t lda, const float* b_dev, int64_t ldb,
                     const int32_t* seg_ptr_dev, int64_t n_segments, int flags /* bit 0: allow reflection */,
                     float cap /* <= 0: none */, float* rmsd_dev, float* rot_dev /* or NULL */,
                     float* aligned_dev /* or NULL */, oard_stream_t stream);

/* ---- validation metric with like atoms matched first ----------------------------------------------------------------------------------
 * Replaces: the permutation search of rmsd_core (oa_reactdiff/analyze/rmsd.py:36-51) in front of the superposition above.  Defined as
 *     M(a, b) = min over the permutations pi mapping every row of a to a row of b of the same species (and, with flags bit 0, over the
 *               z-mirror image of b) of the optimal-superposition RMSD of a against b[pi].
 * NOT replaced: pymatgen's genetic matcher and its `threshold`, and its Hungarian matcher's axis heuristics, which define no function
 * of the inputs.  Per segment (csrc/oard_match.h, one wavefront each, float64, bitwise independent of the other segments):
 *   status 0, exact:  the number of such permutations, prod c_s!, is below exact_limit (0 .. 10000; the reference's `< 1e4`; 0 turns the
 *                     branch off): every one is evaluated and M returned.
 *   status 1, search: otherwise; assignment (minimum cost per species block for |a_i - R b_j|^2, Jonker-Volgenant) and superposition
 *                     alternate from five starts per chirality (the same-order fit and the four proper alignments of the principal
 *                     axes) until the permutation repeats or 32 assignments were made; the smallest RMSD is returned:
 *                     M <= result <= the same-order RMSD.
 *   status 2: the species of a's and b's rows differ as multisets;  status 3: more than 256 rows;  status 4: a non-finite coordinate
 *             (3 is checked first, then 4, then 2).  rmsd = cap if cap > 0, else NaN; rot / aligned NaN; perm the identity.
 *   An empty segment gives NaN and status 0.
 * Arguments as for oard_kabsch_rmsd, and: species_a_dev / species_b_dev, one int32 per row of a_dev / b_dev (species_b_dev NULL: the
 * same as species_a_dev); perm_dev (or NULL): [rows] int32, perm[r] = the row of b_dev matched to row r of a_dev (an index into the whole
 * array, inside r's segment); status_dev (or NULL): [n_segments] int32.  rot_dev as above; aligned_dev row r = rot (b_perm[r] - c_b) + c_a:
 * b in a's frame AND in a's row order.  The RMSD is the residual of a pass over the rows with the kept permutation and map.
 * OARD_EINVAL as for oard_kabsch_rmsd, and for a null species_a_dev or exact_limit outside 0 .. 10000. */
int oard_matched_rmsd(const float* a_dev, int64_t lda, const float* b_dev, int64_t ldb,
                      const int32_t* species_a_dev, const int32_t* species_b_dev /* or NULL */,
                      const int32_t* seg_ptr_dev, int64_t n_segments, int flags /* bit 0: allow reflection */,
                      float cap /* <= 0: none */, int exact_limit, float* rmsd_dev, float* rot_dev /* or NULL */,
                      float* aligned_dev /* or NULL */, int32_t* perm_dev /* or NULL */, int32_t* status_dev /* or NULL */,
                      oard_stream_t stream);

/* ---- distinct structures: all-pairs RMSD per group, greedy de-duplication -------------------------------------------------------------
 * Replaces: the two host loops over pymatgen of the reference's walkthrough - the all-pairs RMSD matrix over the transition states of
 * one reaction (demo.py:401-480, pymatgen_rmsd(..., ignore_chirality=True) over every i < j) and the de-duplication of generated
 * structures (demo.py:544-557: new when the smallest RMSD to the structures kept so far exceeds 0.1).  csrc/oard_pairwise.h.
 *
 * oard_pairwise_rmsd.  A member is a segment of ONE array: rows seg_ptr[s] .. seg_ptr[s + 1] of x_dev (row-major float32, row stride
 * ldx >= 3 in elements, coordinates in the first three columns, read where it lies; species_dev: one int32 per row, needed with flags
 * bit 1).  Group g is the members group_members[group_ptr[g] .. group_ptr[g + 1]] (int32 segment indices, in any order, not
 * necessarily adjacent in x; K_g of them).  pair_ptr / mat_ptr: int64 [n_groups + 1], the exclusive prefix sums of K_g (K_g - 1) / 2 and
 * of K_g^2; n_pairs / n_members their totals (pair_ptr[n_groups], group_ptr[n_groups]).  All tables are device arrays.
 * out_dev: the packed row-major K_g x K_g matrices, group g at mat_ptr[g].  One wavefront per unordered pair i < j (the upper triangle
 * row by row) runs the body of oard_kabsch_rmsd (flags bit 1 clear) or of oard_matched_rmsd (bit 1 set; exact_limit as there) with
 * member i as a and member j as b - the same bits as those calls on explicit copies - and writes [i, j] and [j, i] from the one value;
 * flags bit 0: the mirror image too.  A second small launch writes the diagonal: 0 for a finite, non-empty member.
 * status_dev (or NULL), int32 packed like out_dev: 0 exact or same-order fit, 1 search, 2 species lists differ, 3 a member of more than
 * 256 rows (bit 1 only), 4 a non-finite coordinate, 5 the two members have different row counts.  3, 4, 5, 2 are checked in this order,
 * so a non-finite or over-long member carries one code along its whole row and column, its diagonal entry included.  Statuses 2 .. 5 give
 * cap if cap > 0, else NaN; with a cap every value is min(value, cap).  A pair with an empty member - no rows, or a member index outside
 * [0, n_segments) - gives NaN, status 0.
 * Every index read from device memory is clamped before use (group boundaries to [0, n_members], segment boundaries to
 * [0, seg_ptr[n_segments]]; a group whose matrix does not lie inside [0, mat_ptr[n_groups]) is not written): wrong tables give wrong
 * numbers, never an access outside the arrays named.
 * OARD_EINVAL - before any HIP call - for a null x / seg_ptr / group_members / group_ptr / pair_ptr / mat_ptr / out, a negative count,
 * n_pairs > 0x7fffffff, ldx < 3, flags bit 1 without species_dev, exact_limit outside 0 .. 10000.  n_groups == 0: OARD_OK, no launch;
 * n_pairs == 0: the diagonal launch alone (if n_members > 0).  No allocation, asynchronous on `stream`, capturable.
 *
 * oard_leader_cluster.  dist_dev / mat_ptr_dev / group_ptr_dev as above (any float32 matrices, e.g. out_dev).  One wavefront per group
 * visits the members in the order order_dev gives (int32 group-local indices packed like the members; NULL: index order).  A member joins
 * the leader at the smallest distance dist[member, leader] if that is <= threshold (float32 compare: a NaN is never close; a tie goes to the
 * leader created first), else it becomes a leader.  label_dev [n_members] int32: the group-local index of each member's leader (a leader
 * labels itself); n_clusters_dev [n_groups] int32.  A group of more than OARD_LEADER_MAX members: label -1 throughout, n_clusters -1.
 * Integer work and float compares only.  OARD_EINVAL for a null dist / mat_ptr / group_ptr / label / n_clusters, n_groups < 0, a negative or
 * non-finite threshold; n_groups == 0: OARD_OK, no launch. */
#define OARD_LEADER_MAX 1024
int oard_pairwise_rmsd(const float* x_dev, int64_t ldx, const int32_t* species_dev /* or NULL without flags bit 1 */,
                       const int32_t* seg_ptr_dev, int64_t n_segments, const int32_t* group_members_dev, const int32_t* group_ptr_dev,
                       const int64_t* pair_ptr_dev, const int64_t* mat_ptr_dev, int64_t n_groups, int64_t n_pairs, int64_t n_members,
                       int flags /* bit 0: allow reflection, bit 1: match like atoms first */, float cap /* <= 0: none */,
                       int exact_limit, float* out_dev, int32_t* status_dev /* or NULL */, oard_stream_t stream);
int oard_leader_cluster(const float* dist_dev, const int64_t* mat_ptr_dev, const int32_t* group_ptr_dev,
                        const int32_t* order_dev /* or NULL */, int64_t n_groups, float threshold, int32_t* label_dev,
                        int32_t* n_clusters_dev, oard_stream_t stream);

/* ---- ranking metrics: midranks per segment, AUROC, Pearson, Spearman --------------------------------------------------------------
 * Replaces: the torchmetrics objects ConfModule logs through (oa_reactdiff/trainer/pl_trainer.py:475 BinaryAUROC, :485-486
 * PearsonCorrCoef / SpearmanCorrCoef; used at :568, :579, :581), per segment instead of per call.
 * score_dev / target_dev: contiguous float32 [n]; segment g is rows seg_ptr[g] .. seg_ptr[g + 1] (seg_ptr_dev: n_segments + 1 ascending
 * int32, as for oard_kabsch_rmsd); every boundary is clamped to [0, n] on the device, so a wrong seg_ptr reads nothing outside the arrays.
 * rank_score_dev / rank_target_dev (or NULL): float64 [n], the 1-based average rank ("midrank") of every row among the rows of its
 *     segment, rank_i = #{x_j < x_i} + (#{x_j == x_i} + 1) / 2 = scipy.stats.rankdata(method="average"); int32 compare-and-count, nothing
 *     is sorted: exact half-integers, independent of launch shape and row order; O(sum n_g^2) compares.  Rows of no segment get NaN.
 * out_dev (or NULL): [n_segments, OARD_RANK_COLS] float64, per segment
 *     0 n_g   1 n_pos = rows with target >= 0.5   2 AUROC   3 Pearson(score, target)   4 Spearman = Pearson of the two midranks
 *     5 mean |score - target|   6 mean score   7 mean target
 *     AUROC = (R_pos - n_pos (n_pos + 1) / 2) / (n_pos n_neg), R_pos the score-midrank sum of the positive rows as an exact integer of
 *     twice-ranks (ties count half: BinaryAUROC(thresholds=None)); Pearson from centred sums behind a first pass for the means; float64
 *     sums in a fixed order, one wavefront per segment: a segment's bits depend on its own values alone (csrc/oard_rank.h).
 *     Without both rank arrays the ranks behind cols 2 and 4 are counted inside that wavefront - meant for short segments; pass both
 *     arrays for long ones.
 * Empty segment: col 0 = 0, the rest NaN.  n_pos == 0 or n_pos == n_g: AUROC = 0 (torchmetrics' value where undefined).  Zero variance:
 * Pearson / Spearman NaN (0 / 0, as scipy).  A NaN in score or target of a segment: its cols 2-7 and its ranks are NaN, nothing faults,
 * the other segments are untouched.  +-inf is ordered like any value (ranks, AUROC, Spearman defined; cols 3, 5-7 follow IEEE).
 * OARD_EINVAL - before any HIP call - for n < 0 or n >= 2^31, n_segments < 0, all three outputs NULL, and with n_segments > 0 for a null
 * score_dev / target_dev / seg_ptr_dev; n_segments == 0 returns OARD_OK without a launch.  No oard_config, no topology, no allocation;
 * asynchronous on `stream`, capturable. */
#define OARD_RANK_COLS 8
int oard_rank_metrics(const float* score_dev, const float* target_dev, int64_t n,
                      const int32_t* seg_ptr_dev, int64_t n_segments,
                      double* rank_score_dev /* [n] or NULL */, double* rank_target_dev /* [n] or NULL */,
                      double* out_dev /* [n_segments, 8] or NULL */, oard_stream_t stream);

/* ---- reaction dataset: one gather launch per batch (csrc/oard_dataset.h) --------------------------------------------------------
 * Replaces: ProcessedTS1x.__getitem__ + BaseDataset.collate_fn (oa_reactdiff/dataset/base_dataset.py:51-88) over what
 * ProcessedTS1x.__init__ builds per sample (dataset/transition1x.py:21-150, base_dataset.py:142-217).
 *
 * oard_reaction_store is a plain description of arrays the caller owns: no handle, no hidden state.  Per SOURCE object (0 reactant,
 * 1 transition state, 2 product): offsets [n_raw + 1] (exclusive prefix sums of the atom counts), raw float32 positions [sum n, 3], atomic
 * numbers [sum n] (1, 6, 7, 8 or 9: the caller checks).  sel [n_sel]: the selected raw reactions.  A virtual sample index v in
 * [0, n_sel * (1 + swap) * (1 + reflect)) decodes as  f_bit = v / (n_sel * s), j = v % (n_sel * s), s_bit = j / n_sel, r = sel[j % n_sel]
 * (original block, swapped block, then the reflected copy of both).  Output object k reads source src_obj[k]; a swapped sample reads
 * source 2 - src_obj[k].  A reflected sample negates the last raw coordinate of every object with reflect_obj[k].  center: positions
 * minus their mean over the molecule (float64 sum in a fixed order, one rounding).  zero_charge: the charge column is 0.  append_frag:
 * charge has a second column holding append_charge[k].  target / rmsd (or NULL): [n_raw] columns read at v % n_raw, the reference's
 * unselected lists.  ediff[0] / ediff[1] (or NULL): [n_raw] columns of the named object and of its swap partner, read at r.
 *
 * oard_dataset_gather writes samples index_dev[first .. first + B) into the outputs: per output object k  size [B], pos [n_k, 3],
 * one_hot [n_k, 5], charge [n_k, 1 + append_frag], mask [n_k] (= b), where sample b starts at row
 * epoch_off_dev[k][first + b] - epoch_off_dev[k][first]  (epoch_off_dev[k]: exclusive prefix sums of object k's atom counts along
 * index_dev, one entry more than index_dev); condition [B] = 0; target / rmsd / ediff [B] where the store has the column (the output is
 * required exactly then).  The pointer ARRAYS are host arrays of n_obj device pointers.  OARD_EINVAL - before any HIP call - for a NULL
 * store, array or entry, n_obj not 1 or 3, a src_obj outside 0..2, a flag outside {0, 1}, n_raw / n_sel < 1, n_sel > n_raw, first < 0, B < 0,
 * (first + B) or B * n_obj >= 2^31, a column / output mismatch.  B == 0 returns OARD_OK without a launch.  One launch, no allocation,
 * no copy; asynchronous on `stream`, capturable.  No counterpart kernel in the reference. */
#define OARD_STORE_OBJECTS 3
typedef struct oard_reaction_store {
    const int64_t* offsets[OARD_STORE_OBJECTS];
    const float* pos[OARD_STORE_OBJECTS];
    const int32_t* z[OARD_STORE_OBJECTS];
    const int64_t* sel;
    const int64_t* target;
    const float* rmsd;
    const float* ediff[2];
    int64_t n_raw, n_sel;
    int32_t n_obj;
    int32_t src_obj[OARD_STORE_OBJECTS];
    int32_t reflect_obj[OARD_STORE_OBJECTS];
    int32_t append_charge[OARD_STORE_OBJECTS];
    int32_t swap, reflect, center, zero_charge, append_frag;
} oard_reaction_store;
int oard_dataset_gather(const oard_reaction_store* store, const int64_t* index_dev, const int64_t* const* epoch_off_dev,
                        int64_t first, int64_t B,
                        int64_t* const* size_dev, float* const* pos_dev, int64_t* const* one_hot_dev, int64_t* const* charge_dev,
                        int64_t* const* mask_dev, int64_t* condition_dev, int64_t* target_dev /* or NULL */,
                        float* rmsd_dev /* or NULL */, float* ediff_dev /* or NULL */, oard_stream_t stream);

/* The library's own streams of the current device(three non-blocking streams, chosen once per device so that each runs on a hardware
 * queue of its own beside the caller's stream - the runtime serves a process's streams from 4 queues): 0 = the training sweep's
 * gradient stream (and the second sub-batch of a multi-part forward), 1 = the third sub-batch, 2 = topology uploads (and the fourth).
 * For callers that want a second in-order queue WITHOUT adding a fifth stream to the process: DDPMTrainer's two-micro-batch step runs
 * its second micro-batch on stream 1, which is idle in training.  No counterpart in the reference. */
int oard_library_stream(int which, oard_stream_t* out);

/* ---- general edge lists (round 6) --------------------------------------------------------------------------------------------
 * Replaces: EGNNDynamics.forward on an edge_index that is NOT the complete graph per sample.  The reference accepts any edge list
 * (dynamics/egnn_dynamics.py:63-72), builds incomplete ones with get_edges_index(..., edge_cutoff=) (utils/_graph_tools.py:31-33, plumbed
 * through trainer/pl_trainer.py:68,94 and dynamics/_base.py:59), and its model tests run disconnected and cut graphs
 * (tests/model/test_equiv.py:177-230, tests/model/test_subgraphs.py:285-339).  Production never leaves the complete graph
 * (trainer/train_ts1x.py:106), so this path is built for parity first (csrc/oard_general.h): explicit edge list, CSR gathers in
 * edge order, the reference's literal node frame (leftnet.py:812-834) on float64 geometry, float64 accumulation, raw (unpacked) parameters.
 * Its dense layers run on the float64 matrix pipe (k_general_gemm_f64, csrc/oard_general.hip); the environment variable
 * OARD_GENERAL_GEMM=threads, read on every call, runs them on plain threads instead (the cross-check form; same results, ~18 x the time).
 * Inference only.
 *
 * oard_graph_create: host arrays in (combined_mask / n_frag_switch as for oard_topology_create; edge_index [2, E] row-major, reference
 * node ids; self loops, duplicates and edges across samples are taken as given, as the reference does), device tables out.
 * oard_graph_is_complete: 1 iff the edge SET is get_edges_index(combined_mask, remove_self_edge=True) in any order - the caller may then
 * use oard_forward instead.  oard_graph_forward: as oard_forward, with the canonical parameter pointers (oard_pack_weights' order) in
 * place of the packed blob; asynchronous on `stream`; the workspace is the caller's and carries everything the call needs. */
typedef struct oard_graph oard_graph;
int oard_graph_create(const oard_config* cfg, const int64_t* combined_mask_host, const int64_t* n_frag_switch_host, int64_t n_nodes,
                      const int64_t* edge_index_host, int64_t n_edges, oard_graph** out);
void oard_graph_destroy(oard_graph* graph);
int64_t oard_graph_num_nodes(const oard_graph* graph);
int64_t oard_graph_num_edges(const oard_graph* graph);
int64_t oard_graph_object_rows(const oard_graph* graph, int object);   /* rows of xh[object] */
int oard_graph_is_complete(const oard_graph* graph);
size_t oard_graph_workspace_bytes(const oard_config* cfg, const oard_graph* graph);
int oard_graph_forward(const oard_config* cfg, const oard_graph* graph, const float* const* params_dev, size_t n_params,
                       const float* const* xh_dev, const float* t_dev, int t_is_scalar, const float* conditions_dev,
                       float* const* out_dev, void* workspace_dev, size_t workspace_bytes, int32_t* status_dev, oard_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OARD_H */

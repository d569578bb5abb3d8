/*
 * dfmdock_amd.h - C ABI of the MI355X-native DFMDock sampling engine.
 *
 * This is the drop-in boundary for the ONE hot path this project accelerates
 * (SURVEY.md section 8): the reverse-diffusion sampler over rigid-body poses and
 * the score network it calls.  The reference has no FFI layer - the path sits
 * behind plain Python call signatures - so each entry point below names the
 * reference call it replaces (paths relative to the reference checkout):
 *
 *   dfm_model_create    <- Score_Model.load_from_checkpoint / Score_Net.__init__
 *                          (src/inference_base.py:611-616, src/models/score_net_mlsb.py:249-341)
 *   dfm_complex_create  <- get_batch_from_inputs + get_position_matrix
 *                          (src/inference_base.py:192-253)
 *   dfm_score           <- Score_Model.forward(batch)  (src/models/score_model_mlsb.py:61-63 ->
 *                          src/models/score_net_mlsb.py:343-425); with dfm_hparams.family = 1:
 *                          DFMDock.forward(batch) (src/models/DFMDock.py:68-75 -> src/models/egnn_net.py:408-505)
 *   dfm_sample          <- Euler_Maruyama_sampler(model, batch, ...) (src/inference_base.py:390-468),
 *                          batched over B independent trajectories
 *   dfm_diffusion_coef  <- R3Diffuser.diffusion_coef / SO3Diffuser.diffusion_coef
 *                          (src/utils/r3_diffuser.py:23-24, src/utils/so3_diffuser.py:219-227)
 *
 * Conventions: plain pointers and sizes, caller owns every host buffer, the
 * library owns device memory behind opaque handles, no global state besides the
 * thread-local error string.  All entry points return 0 on success and a
 * negative dfm_status otherwise (the reference raises Python exceptions:
 * ValueError for t outside [0,1] -> DFM_E_INVALID).  A handle must not be used by
 * two host threads at once (no internal locking per handle); DIFFERENT complex
 * handles of one model may be driven from different host threads concurrently:
 * each complex owns a non-blocking HIP stream and every upload, launch and
 * release of the handle is ordered on that stream alone, so creating / checking
 * the next complex of a set overlaps the sampling of the current one
 * (dfmdock_amd/driver.py: run_set; the reference's loop is serial,
 * src/inference_mlsb.py:415-439).  One process per GPU.
 * Status of that guarantee (r05 / r06): concurrent handles once produced a silent miscompute - waves of an LDS-free geometry kernel
 * binning wrong dihedrals from correct inputs while another handle's 160 KiB message-kernel workgroups were resident.  r06 traced it to
 * one instruction form hipcc's SLP vectoriser had emitted (a packed fp32 multiply with op_sel = [0,1]: low result from the HIGH half of
 * source 1) and reproduced it without the engine: while one wave of a SIMD executes a 16-bit-input MFMA, such an instruction issued by
 * another wave of that SIMD returns wrong values (profiles/r06_concurrency.txt, tools/ubench/pk_erratum.hip) - hardware, not data flow.  Fenced three ways: no kernel of the library contains such an instruction
 * (built with -fno-slp-vectorize, disassembly audited by tests/test_abi_cpu.py: THE fence), every kernel launch holds some LDS (keeps
 * it off CUs that a message kernel's workgroup fills), and dfmdock_amd/driver.py re-samples one complex alone after an overlapped run and compares bit for bit
 * (falling back to the serial driver on a mismatch).  tests/test_gpu_concurrency.py holds the shipped build to 0 deviations in a
 * victim x aggressor matrix over every kernel of the path.  CALLERS that run their OWN kernels on the same GPU next to this library
 * should know the form (tools/ubench/pkmul_victim.hip).
 * A model lives on the device that was current at dfm_model_create (dfm_set_device), a
 * complex on its model's device; every entry point switches to the handle's device for
 * the duration of the call and restores the caller's current device.
 * Everything computes on the GPU: there is no CPU fallback in this library.
 */
#ifndef DFMDOCK_AMD_H
#define DFMDOCK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dfm_model dfm_model;
typedef struct dfm_complex dfm_complex;
typedef struct dfm_native dfm_native;

typedef enum {
    DFM_OK = 0,
    DFM_E_INVALID = -1,   /* bad argument (shape, range, NULL)          */
    DFM_E_HIP = -2,       /* HIP runtime error (see dfm_last_error)      */
    DFM_E_OOM = -3,       /* device or host allocation failed            */
    DFM_E_NODEVICE = -4   /* no usable gfx950 device                     */
} dfm_status;

/* configs/model/score_model_mlsb.yaml:3-27 (+ score_net_mlsb.py:33,:85 constants) */
typedef struct {
    int lm_embed_dim;          /* 1301 = 1280 (ESM-2) + 21 (one-hot)   */
    int positional_embed_dim;  /* 66, or 67 = 66 relpos + 1 "sym" channel (configs/model/DFMDock.yaml:5):
                                  the homomer flag of the complex, see dfm_complex_set_homomer            */
    int spatial_embed_dim;     /* 100 = 40 + 24 + 24 + 12               */
    int node_dim;              /* 256 (only value supported by kernels) */
    int edge_dim;              /* 128                                   */
    int inner_dim;             /* 128                                   */
    int depth;                 /* 6                                     */
    int knn;                   /* 20                                    */
    int n_sample;              /* 40                                    */
    float cut_off;             /* 20.0  energy mask                     */
    float mask_dist;           /* 22.0  angle-feature mask              */
    double r3_min_sigma, r3_max_sigma;    /* 0.1, 30.0                  */
    double so3_min_sigma, so3_max_sigma;  /* 0.1, 1.5 (logarithmic)     */
    int family;                /* 0: Score_Net (src/models/score_net_mlsb.py:249-425, what inference_single.py loads);
                                  1: EGNN_Net behind DFMDock.forward (src/models/egnn_net.py:408-505,
                                     src/models/DFMDock.py:68-75, configs/model/DFMDock.yaml: mask_dist 20):
                                     no coordinate update, pair force / energy / confidence heads          */
    int agg_mean;              /* family 1: `agg` 'mean' (1, default) or 'sum' (0), egnn_net.py:438-474     */
} dfm_hparams;

/* flags for dfm_score / dfm_sample */
enum {
    DFM_F_MFMA16 = 1u << 0,          /* the 16-bit MFMA engine (default without flag: exact fp32): per-edge 256 x 256
                                        contractions on v_mfma_f32_32x32x16 with fp16 operands and fp32 accumulation in every
                                        layer, gathered operands (Wb h_j, lookup tables, A_i) stored as fp16, node-level GEMMs
                                        as three split-bf16 terms (~1e-5), geometry / GraphNorm statistics / heads / SDE step
                                        fp32.  dfm_config_string() describes the plan in force.                         */
    DFM_F_BF16 = DFM_F_MFMA16,       /* name of rounds 1-2 (the engine then took bf16 operands in layers 0..depth-2)    */
    DFM_F_ENERGY = 1u << 1,          /* dfm_score: also evaluate the energy head                 */
    DFM_F_NOISE_ANNEALING = 1u << 2, /* inference_base.py:428-430                                */
    DFM_F_CLASH_FORCE = 1u << 3,     /* inference_base.py:458-461                                */
    DFM_F_ODE = 1u << 4,             /* so3_diffuser.py:367-368                                  */
    DFM_F_PROFILE = 1u << 5,         /* time the dominant kernel with HIP events + its in-kernel clock stamps (dfm_get_profile) */
    DFM_F_STEP_ENERGY = 1u << 6,     /* dfm_sample: evaluate the energy head on every step (traces) */
    DFM_F_F16 = 1u << 7,             /* like DFM_F_MFMA16 but A_i = Wa h_i + b1 stays fp32 (one more load per chunk)     */
    DFM_F_IRES = 1u << 8,            /* dfm_score: also evaluate the interface-residue head (score_net_mlsb.py:383) */
    DFM_F_DIST = 1u << 10,           /* dfm_score, family 1: also evaluate dist_logits = to_dist(cat[h_r, h_l, D]) over all R x L pairs
                                        (egnn_net.py:347-352,:447; a training-loss input, never read by a sampler); fp32 in every engine */
    DFM_F_BF16_OPS = 1u << 9,        /* with DFM_F_MFMA16: bf16 instead of fp16 MFMA operands in layers 0..depth-2 (the r02
                                        plan; ~3 % faster).  OUTSIDE SURVEY 8(d)'s 1e-2 gate: measured up to 1.5e-2 on f /
                                        tr_score / rot_score over four weight draws (profiles/r03_tol_report.txt) - an opt-in
                                        for callers who accept that; tested at 2e-2                                      */
    /* Layer 0 behind the per-complex message table (DFM_F_MFMA16 engine and the fp32 engine, a table each; src/models/egnn.py:95-104 evaluated once per
       intra-chain residue pair instead of once per edge, trajectory and step - in layer 0 the node features are the pose-independent
       embedding, and the geometry of two residues of one chain does not change under the rigid motion of the ligand).  dfm_sample
       uses the table whenever the complex is eligible (depth >= 2, (R^2 + L^2) * 516 B and the per-batch row buffers within the
       budgets in api_complex.hip), whatever the batch size; dfm_score is a pure function of its arguments and uses it only on request.
       Inter-chain edges, and intra-chain edges whose feature bins in the pose at hand differ from the table's, go through the edge
       model as before.  Against the direct evaluation the only difference is the fp16 rounding of each stored message before the
       K-row sum (fp32 engine: fp32 rows of 1 KiB, only the ORDER of the K-row sum differs, <= 2e-5; measured: tests/test_gpu_l0_table.py).                                                                  */
    DFM_F_L0_TABLE = 1u << 11,       /* dfm_score: use (and if necessary build) the table.  A hit needs the edge's bin code AND its squared
                                        C-alpha distance in the pose at hand to equal those the entry was built with on the handle's stored
                                        pose (the distance up to the rounding of a rigid motion, 1e-3 A x max(d, 1)): any lig_pos is safe - an
                                        intra-chain pair whose geometry differs (another conformer, a perturbed backbone) is a miss and goes
                                        through the edge model like an inter-chain edge.  Whether a complex uses the table depends on the
                                        complex alone (R^2 + L^2 <= 8 M pairs), never on B: a batch whose per-edge buffers (532 B per edge)
                                        do not fit fails with DFM_E_OOM instead of changing the arithmetic.                       */
    DFM_F_NO_L0_TABLE = 1u << 12,    /* dfm_sample: evaluate layer 0 directly                                            */
    DFM_F_RESTRAINTS = 1u << 14,     /* dfm_sample: apply the interface restraint step (dfm_complex_set_restraints) after every step's
                                        Euler-Maruyama update with t_i <= t_start, before the clash force.  With no set stored the flag
                                        does nothing: the results are bitwise those of the unflagged call                   */
    DFM_F_SYMMETRY = 1u << 15,       /* dfm_sample / dfm_refine: apply the Cn symmetry step (dfm_complex_set_symmetry) as the LAST thing
                                        that moves the pose in every step with t_i <= t_start: evaluation, heads, restraint step, clash
                                        force, symmetry step.  With no symmetry stored the flag does nothing: the results are bitwise
                                        those of the unflagged call                                                          */
    DFM_F_GRAPH = 1u << 13           /* dfm_sample: capture ONE step (score evaluation + heads + update) as a hipGraph and replay it
                                        num_steps times instead of enqueueing every launch (ignored when anything is injected,
                                        traced or profiled).  Same kernels and arguments - the per-step / per-call scalars are
                                        read from device memory - so the trajectories are bitwise those of the plain path
                                        (tests/test_gpu_graph.py).  Opt-in: on MI355X the stream is paced by the device-side
                                        dispatch of ~30 dependent launches per evaluation, not by the host, and the replay
                                        measures 0.2 - 1.9 % SLOWER at B = 1 ... 120 (profiles/r04_graph_ab.txt); it is there
                                        for hosts that cannot keep a stream fed (DFM_GRAPH=1 in the environment: default on) */
};

/* Parameters of the restraint step (dfm_complex_set_restraints).  Defaults (p_or_null = NULL): DESIGN.md "Interface restraints". */
typedef struct {
    float k_tr;       /* A per unit of force (U in A^2, F in A):           dtau   = clip(k_tr F, max_tr)      default 0.25   */
    float k_rot;      /* rad per unit of torque (A^2):                     domega = clip(k_rot T, max_rot)    default 3e-3   */
    float max_tr;     /* A, largest translation of one restraint step                                         default 10.0   */
    float max_rot;    /* rad, largest rotation of one restraint step                                          default 0.3    */
    float t_start;    /* the step runs on step i when t_i <= t_start (1.0: every step)                         default 1.0    */
} dfm_restraint_params;

/* Parameters of the symmetry step (dfm_complex_set_symmetry).  The defaults (p_or_null = NULL) are starting values: nobody has measured
 * them against a trained checkpoint. */
typedef struct {
    float gain_rot;     /* in (0, 1]: fraction of the angle error one step removes: domega = clip(gain_rot (theta* - theta) u, max_rot)  default 0.5 */
    float gain_tr;      /* in (0, 1]: fraction of the screw translation one step removes: dtau = clip(-gain_tr s u, max_tr)              default 0.5 */
    float max_rot;      /* rad, largest rotation of one symmetry step                                                                   default 0.3 */
    float max_tr;       /* A, largest translation of one symmetry step                                                                  default 10.0 */
    float t_start;      /* the step runs on step i when t_i <= t_start (1.0: every step)                                                 default 1.0 */
    int32_t snap_last;  /* non-zero: the LAST step of a sampler call projects exactly (gains 1, nothing clipped)                          default 1 */
} dfm_symmetry_params;

/* Output of dfm_symmetry_eval.  Required: step.  Any other pointer may be NULL. */
typedef struct {
    double *theta;        /* [B]    rad, rotation angle of the monomer-to-monomer transform T, in [0, pi]                 */
    double *screw;        /* [B]    A, translation of T along its axis                                                   */
    double *axis;         /* [B,3]  unit axis u of T                                                                     */
    double *axis_point;   /* [B,3]  a point of the axis of the projected (pure-rotation) transform: the assembly's axis   */
    double *fit_rmsd;     /* [B]    A, rms residual of the fit of the receptor onto the pose                              */
    double *sym_rmsd;     /* [B]    A, rms displacement of the pose's atoms under the full projection                     */
    int32_t *order_m;     /* [B]    m of theta* = 2 pi m / n (0: no axis, or a non-finite pose)                           */
    float *step;          /* [B,6]  dtau, domega of a non-final step                                                     */
} dfm_symmetry_out;

/* Output of dfm_score.  Required: tr_score, rot_score.  Any other pointer may be NULL. */
typedef struct {
    float *tr_score;      /* [B,3]                                                      */
    float *rot_score;     /* [B,3]                                                      */
    float *energy;        /* [B]      (needs DFM_F_ENERGY)                              */
    int32_t *num_clashes; /* [B]      (needs DFM_F_ENERGY)                              */
    float *f;             /* [B,L,3]  per-ligand-residue force                          */
    /* debug / parity taps */
    float *h_last;        /* [B,N,H]  node features after the last layer.  They feed the energy / ires / dist heads only
                                      (score_net_mlsb.py:383-390): a call that asks for none of those and passes h_last = NULL
                                      computes the last layer for the ligand nodes alone (all that f needs, :396-398) -
                                      bitwise the same f / tr_score / rot_score                               */
    float *h_first;       /* [B,N,H]  node features after the first layer               */
    int32_t *edges;       /* [B,N,K]  edge list actually used                           */
    uint32_t *edge_codes; /* [B,N,K]  packed feature bins: d | omega<<6 | theta<<11 | phi<<16 | relpos<<20 */
    float *confidence;    /* [B]      family 1 + DFM_F_ENERGY: confidence_logits (egnn_net.py:444); may be NULL */
    float *ires;          /* [B,N]    needs DFM_F_IRES: to_ires(node_out) (score_net_mlsb.py:297-303,:383; family 1:
                                      ires_logits, egnn_net.py:362-368,:462); may be NULL                     */
    float *dist_logits;   /* [B,R,L,64] needs DFM_F_DIST and a family-1 model (egnn_net.py:447,:500); may be NULL  */
} dfm_score_out;

/* Injected randomness for parity tests (every pointer may be NULL = draw natively with Philox) */
typedef struct {
    const float *R0;       /* [B,9]  initial rotation matrices (row-major)              */
    const float *tr_draw;  /* [B,3]  the N(0,30^2) draws of randomize_pose               */
    const float *z_rot;    /* [B,steps,3] N(0,1) draws of the SO(3) update                */
    const float *z_tr;     /* [B,steps,3] N(0,1) draws of the R^3 update                  */
    const int32_t *edges;  /* [B,steps+1,N,K] edge lists, one per score evaluation       */
} dfm_inject;

typedef struct {
    float *lig_pos;       /* [B,L,9]  final ligand backbone (N,CA,C)                     */
    float *rot_update;    /* [B,3]    accumulated rotation, axis-angle                   */
    float *tr_update;     /* [B,3]    accumulated translation                            */
    float *energy;        /* [B]      energy of the final pose                           */
    int32_t *num_clashes; /* [B]                                                         */
    float *final_scores;  /* [B,6]    tr_score, rot_score of the final evaluation (may be NULL) */
    /* optional traces (NULL to skip) */
    float *trace_pose;    /* [B,steps,L,9]  pose after every step                        */
    float *trace_scores;  /* [B,steps+1,8]  tr_score, rot_score, energy, num_clashes per evaluation */
    float *init_pose;     /* [B,L,9]        pose after randomize_pose                    */
} dfm_traj_out;

/* Local refinement (dfm_refine): where the trajectories start.  The pose is noised with the reference's forward process at t_begin
 * (score_model_mlsb.py:65-94: IGSO(3) rotation about the ligand centroid + N(0, sigma_r3(t_begin)^2) translation; dfmdock_amd/refine.py
 * is the float64 definition) and the reverse SDE runs over linspace(t_begin, eps, num_steps). */
typedef struct {
    float t_begin;            /* eps < t_begin <= 1                                                    */
    int perturb;              /* 1: forward marginal at t_begin (default); 0: start at the pose itself  */
    const float *start_pos;   /* [B,L,9] one start pose per trajectory, or NULL: the stored ligand pose */
} dfm_refine_params;

/* Injected draws of the start of dfm_refine / dfm_forward_marginal (every pointer may be NULL = draw natively with Philox) */
typedef struct {
    const float *u_angle;     /* [B]   uniform draw of the rotation angle                               */
    const float *axis_draw;   /* [B,3] N(0,1) draws of the axis (normalised by the kernel)              */
    const float *tr_draw;     /* [B,3] N(0,1) draws of the translation                                  */
} dfm_refine_inject;

typedef struct {
    double edge_kernel_ms;    /* summed HIP-event time of the per-edge message kernel     */
    int64_t edge_kernel_launches;
    int64_t edge_rows;        /* edge rows (B*N*K) processed by those launches           */
    double total_ms;          /* HIP-event time of the whole last dfm_sample / dfm_score  */
    double phase_cycles[4];   /* diagnostic builds only (-DDFM_EDGE_STAMP), else 0: shader cycles per 32-row tile of the
                                 message kernel's third launch, mean over the 8 waves of workgroup 0:
                                 prologue | chunks 0-6 | chunk 7 + bias | epilogue                */
    double slot_cycles[16];   /* diagnostic builds only: summed cycles between consecutive MFMA slots of chunk 3 (wave 0) */
    /* layer 0 behind the message table (DFM_F_L0_TABLE): its launches are NOT part of edge_kernel_* above */
    int64_t l0_evals;         /* evaluations whose layer 0 ran through the table                                 */
    int64_t l0_edges;         /* edges of those layer-0 passes (B*N*K each)                                       */
    int64_t l0_miss_rows;     /* of which evaluated by the edge model (inter-chain + bin mismatches)              */
    double l0_rows_ms;        /* summed HIP-event time of the row-list message launches                           */
    double l0_gather_ms;      /* ... of the gather-sum launches                                                  */
    double l0_build_ms;       /* table build of this call (0 when the table already existed)                      */
    int64_t edge_lig_launches;/* of edge_kernel_launches: last-layer launches over the ligand nodes only          */
    double edge_lig_ms;       /* their share of edge_kernel_ms                                                    */
    /* the shader clock the message kernel actually ran at (the chip's power management, not the kernel, sets it): workgroup 0's first wave
     * reads s_memtime (shader cycles) and s_memrealtime (100 MHz) when it starts and when it leaves, summed over the call's launches;
     * MHz = 100 * edge_shader_cycles / edge_ref_ticks.  0 when the call had no profiled message launch.                              */
    double edge_shader_cycles;
    double edge_ref_ticks;
} dfm_profile;

/* Output of dfm_complex_selfcheck: how far the 16-bit MFMA engine is from the fp32 engine (the reference's own arithmetic) on THIS
 * model and THIS complex, and how much of the fp16 range the model's activations use.  No reference call has a counterpart: the
 * reference computes in fp32 throughout; this is the runtime evidence SURVEY 8(d) gate (5) needs for weights the build has never
 * seen (src/inference_base.py:611-616 loads whatever checkpoint the user has).
 *
 * Deviations: L-inf over L-inf of f / tr_score / rot_score, |dE| / max(|E|, 0.1) of the energy, each the WORST over the n_eval
 * evaluations (same pose, n_eval engine-drawn graphs, n_eval times t); the gates are SURVEY 8(d)'s for 16-bit kernels.
 * The two scores are unit vectors of the pooled force mean_l f and torque mean_l (r_l x f_l) times a learned scale
 * (score_net_mlsb.py:396-411), so their deviation is governed by the force deviation over a cancellation ratio:
 * |d mean f| / |mean f| <= score_bound[0] = sqrt(3) dev_f max|f| / |mean_l f| and the same with r x f for the torque (rigorous for
 * the pooled vectors; the unit vector and the scale net add a model-dependent factor of order 1).  A small cancel_ratio means an
 * ill-conditioned pose - the reference's own fp32 scores are then sensitive to rounding as well - not a broken engine.
 * Range telemetry (from the fp32 pass, per layer l = 0 .. depth-1; the values as the 16-bit engine STORES them, i.e. times
 * log2(e) where the stored operand carries that factor): everything the 16-bit engine keeps in fp16 must stay below 65504 -
 * the engine saturates silently otherwise (conversions clamp).  range_ok = every entry below `limit` (6.0e4). */
typedef struct {
    int n_eval, depth;
    float dev_f, dev_tr_score, dev_rot_score, dev_energy;    /* worst over the evaluations                                   */
    float cancel_ratio[2];                                   /* |mean_l v| / mean_l |v| for v = f and v = r x f (fp32 pass): the
                                                                smallest over the evaluations                                */
    float score_bound[2];                                    /* bound of the relative deviation of the pooled force / torque  */
    float gate_f, gate_score, gate_energy;                   /* 1e-2, 1e-2, 3e-2                               */
    float limit;                                             /* 6.0e4                                                        */
    float max_h[9];       /* |h| entering layer l; [depth] = the final node features                                        */
    float max_A[8];       /* |log2e (Wa h_i + b1)|           stored fp16 (DFM_F_MFMA16) / fp32 (DFM_F_F16)                   */
    float max_Bm[8];      /* |log2e Wb h_j|                  stored fp16                                                     */
    float max_tab[8];     /* largest |entry| of the layer's merged lookup tables (log2e-scaled), stored fp16                 */
    float max_sum16[8];   /* bound of the packed fp16 sum Bm_j + two table rows: max_Bm + the two tables' maxima             */
    float max_pre[8];     /* |log2e pre-activation of edge_mlp.0|: the producer SiLU's output is stored fp16                 */
    float max_acc[8];     /* |log2e pre-activation of edge_mlp.2|: bounds the gated messages the last layer stores as fp16   */
    float headroom;       /* limit / largest of all the above (>= 1 when range_ok)                                          */
    int64_t saturated;    /* fp16 values found AT the saturation value (+-65504 or inf) in A / Bm of the 16-bit pass itself   */
    int range_ok;         /* 1: every tracked magnitude below limit and saturated == 0                                       */
    int dev_ok;           /* 1: dev_f <= gate_f, dev_energy <= gate_energy, each score deviation <= max(gate_score, 2 score_bound[.]) */
    int ok;               /* range_ok && dev_ok                                                                              */
} dfm_selfcheck_out;

const char *dfm_last_error(void);
/* One line describing the precision plan and every diagnostic environment switch / build knob in force in this process
 * (DFM_EDGE_SPLIT; DFM_LIB is the loader's): benches and tests print it, so that a run under
 * a stray variable cannot pass for the shipped engine.  The pointer stays valid for the life of the process. */
const char *dfm_config_string(void);
int dfm_device_count(int *count);
int dfm_set_device(int device);
/* fills hp with the reference configuration */
void dfm_default_hparams(dfm_hparams *hp);
/* number of floats the blob must hold for hp (state_dict order, see dfmdock_amd/weights.py) */
int64_t dfm_param_count(const dfm_hparams *hp);

dfm_model *dfm_model_create(const float *blob, size_t n_floats, const dfm_hparams *hp);
void dfm_model_destroy(dfm_model *m);

/* NULL with DFM_E_INVALID, nothing created or enqueued: a NULL pointer, R or L < 1, R + L > 4096, a NaN or infinite value in rec_pos
 * or lig_pos (the stored pose must be numbers: the layer-0 table and operands are built from it). */
dfm_complex *dfm_complex_create(dfm_model *m, const float *rec_x /*[R,lm]*/, const float *lig_x /*[L,lm]*/,
                                const float *rec_pos /*[R,9]*/, const float *lig_pos /*[L,9]*/, int R, int L);
void dfm_complex_destroy(dfm_complex *cx);
/* Replace the poses stored by dfm_complex_create (either pointer may be NULL = keep): rec_pos [R,9] is what every later
 * dfm_score / dfm_sample call sees as the receptor, lig_pos [L,9] is the start pose of dfm_sample.  The node features and
 * everything derived from them stay resident - a caller that re-centres the complex every step (DFMDock.move_to_lig_center,
 * src/models/DFMDock.py:254-257) or docks several ligand conformations does not pay the feature upload again.  A NaN or infinite
 * value in either array: DFM_E_INVALID before anything is copied - both stored poses, the tables built from them and every later
 * result stay as they were.  On a DFM_E_HIP return the stored poses are unspecified (one of the two may have been replaced): call again. */
int dfm_complex_set_pose(dfm_complex *cx, const float *rec_pos_or_null, const float *lig_pos_or_null);
/* positional_embed_dim = 67 only: value of the 67th ("sym") position channel for this complex - 1 when receptor and ligand
 * have the same sequence (is_homomer, src/datasets/docking_dataset.py:129), 0 otherwise (the default).  DFM_E_INVALID for a
 * 66-channel model and flag != 0.  ASSUMPTION: the reference tree has no producer of a 67-channel position matrix
 * (utils/crop.get_position_matrix returns 66 channels and nothing concatenates is_homomer); the layout taken here is
 * [relpos one-hot 66 | flag], the same constant on every residue pair.  A checkpoint trained with another layout of that
 * channel needs this entry point revisited. */
int dfm_complex_set_homomer(dfm_complex *cx, int flag);
/* Interface distance restraints of the complex: n_groups groups, group g = pairs[group_start[g] .. group_start[g+1]) of (receptor residue
 * i in [0, R), ligand residue j in [0, L)), an upper bound upper[g] > 0 (A) and a weight weight[g] >= 0.  With receptor CA y_i as the
 * sampler sees it (the stored rec_pos, as the clash force) and ligand CA x_j of a trajectory: d_g = min over the group of |x_j - y_i|
 * (the first minimal pair in list order: a group of many pairs is an ambiguous restraint), v_g = max(0, d_g - u_g),
 * U = sum_g w_g v_g^2.  The restraint step of DFM_F_RESTRAINTS moves the ligand rigidly down U: F = -dU/dx summed over the arg-min
 * residues, T = sum (x_j* - c) x F_g about the centroid c the sampler rotates about (ligand CA; all backbone atoms for family 1),
 * dtau = clip(k_tr F, max_tr), domega = clip(k_rot T, max_rot) with clip(v, m) = v min(1, m / |v|), applied as the Euler-Maruyama step
 * is (modify_coords and the rot_update / tr_update bookkeeping, src/inference_base.py:453-456), in the clash force's slot right before
 * it (:458-461), so dfm_traj_out's rot_update / tr_update still describe the final pose.  A step with dtau = domega = 0 leaves every bit
 * of the pose alone.  Uploaded on the handle's stream; n_groups = 0 clears the set.  Limits: 1 <= n_groups <= 4096, at most 2^20 pairs
 * in all, no empty group; bad input returns DFM_E_INVALID and keeps the stored set.  A captured step graph (DFM_F_GRAPH) is invalidated:
 * the next call captures again.  p_or_null = NULL: the defaults (dfm_restraint_params).  No reference call has a counterpart. */
int dfm_complex_set_restraints(dfm_complex *cx, int n_groups, const int32_t *group_start /*[G+1]*/, const int32_t *pairs /*[P,2]*/,
                               const float *upper /*[G]*/, const float *weight /*[G]*/, const dfm_restraint_params *p_or_null);
/* The restraint terms at B poses lig_pos [B,L,9]: energy U [B], the number of groups with v_g = 0 [B] and (step_or_null) the step the
 * sampler would take there [B,6] = dtau, domega.  Runs the sampler's kernel (k_restraint) in its evaluation mode.  No set stored: zeros. */
int dfm_restraint_eval(dfm_complex *cx, int B, const float *lig_pos, float *energy, int32_t *n_satisfied, float *step_or_null);
/* Cn symmetric docking of a homo-oligomer: the ligand is a copy of the receptor's own chain (R == L, residue k of one is residue k of the
 * other) and the assembly wanted is the cyclic n-mer.  With the stored receptor backbone y and a trajectory's pose x: (Q, tau) = the
 * least-squares fit (proper rotation) of y onto x over all 3 R backbone atoms, the monomer-to-monomer transform T; theta in [0, pi] and u
 * the angle and unit axis of Q (quaternion with w >= 0; |v| <= 1e-9: no axis, a zero step); c the centroid the sampler rotates about
 * (ligand CA; all backbone atoms for family 1); g = Q^T (c - tau); s = u . (c - g) the translation along the axis; theta* = 2 pi m / n with
 * m in 1 .. n / 2, gcd(m, n) = 1, closest to theta (ties: the smaller m).  Rotating x about c by (theta* - theta) u and shifting it by
 * -s u makes T a pure rotation by theta* about an axis parallel to u: T^n = identity.  The symmetry step of DFM_F_SYMMETRY takes
 * domega = clip(gain_rot (theta* - theta) u, max_rot), dtau = clip(-gain_tr s u, max_tr) with the restraint step's clip, and on the last
 * step of a call with snap_last the whole projection, so final poses are symmetric to fp32 rounding.  It is applied as the restraint
 * step is (modify_coords and the rot_update / tr_update bookkeeping) as the last thing that moves the pose in a step; a step of all zeros
 * leaves every bit alone.  A pose with a non-finite coordinate gets a NaN step; the other trajectories are unaffected.  The fit needs no
 * reference ligand, so the step is also right under dfm_refine with foreign start poses.
 * n = 0 clears the stored symmetry (p_or_null is then ignored); 2 <= n <= 24 otherwise.  DFM_E_INVALID, the stored state kept: R != L, n outside the range, a gain
 * outside (0, 1], a maximum that is not finite and > 0, a NaN.  A captured step graph (DFM_F_GRAPH) is invalidated: the next call captures
 * again.  p_or_null = NULL: the defaults (dfm_symmetry_params) - starting values nobody has measured against a trained checkpoint.  No
 * reference call has a counterpart. */
int dfm_complex_set_symmetry(dfm_complex *cx, int n, const dfm_symmetry_params *p_or_null);
/* The symmetry terms at B poses lig_pos [B,L,9] (dfm_symmetry_out; the definition in float64 numpy: dfmdock_amd/symmetry.py).  Runs the
 * sampler's kernel (k_symmetry) in its evaluation mode; `step` is the step of a non-final iteration.  No axis: theta = 0, order_m = 0, a
 * zero step, fit_rmsd as fitted and NaN elsewhere.  A non-finite pose: NaN everywhere, order_m = 0.  Nothing stored: zeros. */
int dfm_symmetry_eval(dfm_complex *cx, int B, const float *lig_pos /*[B,L,9]*/, dfm_symmetry_out *out);
/* Pose clustering of B ligand poses lig_pos [B,L,9] (N, CA, C per residue, dfm_traj_out's layout) over the ligand residues
 * residues_or_null[n_res] (NULL: all L; n_res is then ignored).  Distance: rmsd_ab = sqrt(mean over the 3 n_res atoms of |x_a - x_b|^2)
 * with NO superposition - the receptor is fixed in every trajectory of a complex, so this is the pairwise L-RMSD of CAPRI / DockQ.
 * Each pair sums direct differences in a fixed order over the coordinates: the matrix is bitwise symmetric, and a pair's value does
 * not depend on B or on the order of the poses.  Neighbours: rmsd_ab <= radius (a pose is its own neighbour).  Key order: key_or_null
 * ascending (lower = better; NULL: index order), ties to the lower index, NaN last.
 * A pose with a non-finite coordinate among the compared residues: its whole row and column of the dfm_pose_rmsd matrix, the diagonal
 * included, are not finite (NaN for a NaN coordinate; +-inf off the diagonal for an infinite one) and every other entry keeps its bits;
 * a coordinate outside the compared residues is never read.  Such a pose is no pose's neighbour, ITSELF INCLUDED: it never opens a
 * cluster under either rule, joins none and keeps cluster_of = -1.
 *   rule DFM_CLUSTER_ENERGY (leader clustering): walk the poses in key order; an unassigned pose opens a cluster and its unassigned
 *     neighbours join it.
 *   rule DFM_CLUSTER_SIZE (greedy, ClusPro style): repeatedly the unassigned pose with the most unassigned neighbours (ties: better key,
 *     then lower index) and its unassigned neighbours form the next cluster.
 * Both stop after max_clusters clusters or when no pose that is its own neighbour is left, so every cluster formed has size >= 1 and
 * B poses that are all non-finite give *n_clusters = 0.  Out: *n_clusters, center[k] and size[k] for k < n_clusters (the arrays hold at least
 * min(max_clusters, B) entries), cluster_of[B] (-1: not in any of the clusters formed); clusters are numbered in the order they formed.
 * Results equal the float64 definition dfmdock_amd/cluster.py exactly wherever no pair lies within float32 rounding of the radius.
 * Limits: 1 <= B <= 65536, L >= 1, residues in [0, L) without repeats, radius finite and > 0, rule 0 or 1, max_clusters >= 1 - else
 * DFM_E_INVALID; DFM_E_OOM when the B x ceil(B/32) neighbour bitmask (512 MB at B = 65536) or the poses do not fit on the device.
 * Both calls take the MODEL handle (its device) and no complex: the drivers close a complex - and its workspace - right after sampling
 * and cluster later.  Every call owns a non-blocking stream and device temporaries of its own, so calls may run from several host threads
 * at once and next to that model's complex handles.  No reference call has a counterpart. */
enum { DFM_CLUSTER_ENERGY = 0, DFM_CLUSTER_SIZE = 1 };
/* the [B,B] RMSD matrix itself (evaluation) */
int dfm_pose_rmsd(dfm_model *m, int B, int L, const float *lig_pos, const int32_t *residues_or_null, int n_res, float *rmsd);
int dfm_pose_cluster(dfm_model *m, int B, int L, const float *lig_pos, const int32_t *residues_or_null, int n_res,
                     const float *key_or_null, float radius, int rule, int max_clusters, int32_t *n_clusters, int32_t *center,
                     int32_t *size, int32_t *cluster_of);
/* GPU milliseconds of the calling thread's last dfm_pose_rmsd / dfm_pose_cluster: the distance kernel (k_pose_dist) and the clustering
 * kernels after it (0 for dfm_pose_rmsd) - tools/cluster_bench.py */
int dfm_pose_last_timing(double *dist_ms, double *cluster_ms);
/* Docking metrics of P model poses against one native pose: c_rmsd, i_rmsd, l_rmsd, fnat and DockQ as the reference's compute_metrics
 * defines them (src/utils/metrics.py:3-121; dfmdock_amd/metrics.py is the float64 definition this call is tested against), batched on
 * the GPU.  Backbones are [n,9] = (N, CA, C) per residue, dfm_traj_out's layout.
 *   dfm_native_create: the native receptor rec_pos [R,9] and ligand lig_pos [L,9].  Precomputes on the GPU what depends on the native
 *     alone: the interface residues (minimum backbone-atom distance to the other chain < iface_cutoff; the reference uses 10.0), the
 *     native contacts (residue pairs with that distance < contact_cutoff; 5.5) and the receptor's share of the fits' sums.  NULL on
 *     failure (dfm_last_error): NULL pointers, R or L < 1, R x L > 2^27 pairs, cutoffs not finite.  Lives on the MODEL handle's device,
 *     needs the model only for that - the drivers close a complex right after sampling and evaluate later.
 *   dfm_native_info: counts and, where the pointer is not NULL, the interface residue indices (ascending; [n_iface_rec], [n_iface_lig])
 *     and the contact pairs [n_contacts,2] = (receptor residue, ligand residue) in row-major order of the R x L matrix.
 *   dfm_pose_metrics: P >= 1 poses, ligand lig_pos [P,L,9]; receptor rec_pos_or_null [P,R,9], or NULL = the native receptor in every
 *     pose (what every driver of this engine produces: the receptor never moves).  Per pose: three Kabsch fits in fp64 - all 3 (R + L)
 *     atoms (c_rmsd), the interface atoms (i_rmsd), the receptor atoms with the fit applied to the ligand (l_rmsd) - each the RMSD of
 *     the explicitly transformed points; n_recovered = native contact pairs whose minimum backbone-atom distance in the pose is below
 *     contact_cutoff; fnat = round(n_recovered / (n_contacts + 1e-6), 6) and DockQ = (fnat + 1 / (1 + (i_rmsd / 1.5)^2) +
 *     1 / (1 + (l_rmsd / 8.5)^2)) / 3 are finished in double on the host.  No interface residue: i_rmsd and dockq NaN; no native
 *     contact: fnat 0.  A pose with NaN coordinates gets NaN where the definition gives NaN and leaves the other poses alone.  A pose's
 *     outputs depend on that pose and the native alone - not on P, its index, or how the call splits P into chunks (64 MiB of poses
 *     each).  Every output pointer of dfm_metrics_out may be NULL.  DFM_E_INVALID: NULL handle / lig_pos / out, P < 1.
 * A dfm_native is read-only after creation: any number of host threads may call dfm_pose_metrics on it at once, next to sampling
 * handles; every call owns a non-blocking stream and its device temporaries.  No reference call is batched: the reference evaluates one
 * pose per compute_metrics call on the host (src/inference_mlsb.py:232-262). */
dfm_native *dfm_native_create(dfm_model *m, const float *rec_pos /*[R,9]*/, const float *lig_pos /*[L,9]*/, int R, int L,
                              float iface_cutoff, float contact_cutoff);
void dfm_native_destroy(dfm_native *nat);
int dfm_native_info(const dfm_native *nat, int32_t *n_iface_rec, int32_t *n_iface_lig, int32_t *n_contacts, int32_t *iface_rec_or_null,
                    int32_t *iface_lig_or_null, int32_t *contacts_or_null /*[n_contacts,2]*/);
typedef struct {
    double *c_rmsd, *i_rmsd, *l_rmsd, *fnat, *dockq;   /* [P] each, or NULL */
    int32_t *n_recovered;                              /* [P] or NULL       */
} dfm_metrics_out;
int dfm_pose_metrics(dfm_native *nat, int P, const float *lig_pos, const float *rec_pos_or_null, dfm_metrics_out *out);
/* GPU milliseconds of the calling thread's last dfm_pose_metrics, summed over its chunks: the host-to-device copies of the poses and
 * the three kernels (k_metrics_reduce, k_metrics_solve, k_metrics_resid) - tools/metrics_bench.py */
int dfm_metrics_last_timing(double *copy_ms, double *kernel_ms);
/* Consensus contact scoring of P ligand poses of one complex (CONSRANK style): which inter-residue contacts the ensemble agrees on, and
 * how well every pose agrees with the ensemble - a ranking that needs neither a native nor the energy head.  dfmdock_amd/consensus.py
 * is the float64 definition this call is tested against.  rec_pos [R,9] (N, CA, C per residue; the receptor is the same in every pose),
 * lig_pos [P,L,9], member_or_null [P] (non-zero: the pose is a member of the ensemble; NULL: every pose; M = number of members).
 *   contact (p,i,j): the minimum over the 9 backbone-atom pairs of sqrt((dx*dx + dy*dy) + dz*dz), in fp64 on the fp32 inputs, is
 *     < cutoff (strict; the cutoff is widened to double; 5.5 is what dfm_native_create's callers use).  A NaN distance is no contact.
 *   count [R,L]: member poses with the contact.  rec_count [R] / lig_count [L]: member poses in which the residue has a contact.
 *   per pose, member or not: n_contacts [P], and score_sum [P] = the sum of count over the pose's contacts (a member's own contacts are
 *     part of count).  The consensus score score_sum / (M n_contacts) is finished by the caller (consensus.finish).
 *   bits [P,R,ceil(L/64)]: the contacts themselves, bit j % 64 of word j / 64 = contact (i,j); unused high bits are 0.
 * Every output pointer may be NULL.  All results are integers: apart from pairs whose distance rounds onto the cutoff they equal the
 * definition exactly, and they do not depend on the order of the poses or on how the call splits P into chunks
 * (dfm_consensus_chunk_poses poses each; a call of more than one chunk evaluates the contact bits twice - once to count, once to score -
 * instead of keeping them).  A pose with NaN coordinates has no contact there and disturbs no other pose.
 * DFM_E_INVALID, nothing enqueued: NULL m / rec_pos / lig_pos / out, P < 1 or > 65536 (count stays an int32), R or L < 1,
 * R x L > 2^27, cutoff not finite or <= 0, no member.  DFM_E_OOM when the poses, the bits of a chunk or the R x L counts do not fit.
 * Within these limits the cost is proportional to P x R x L, except that lig_count takes R / 64 serial steps of one wave per pose and
 * 64 ligand residues: sized for protein chains (R, L up to a few thousand), slow for a receptor of millions of residues.
 * Takes the MODEL handle for its device only.  Every call owns a non-blocking stream and its device temporaries, so calls may run from
 * several host threads at once and next to that model's sampling handles.  No reference call has a counterpart. */
typedef struct {
    int32_t *count;        /* [R,L]  or NULL */
    int32_t *rec_count;    /* [R]    or NULL */
    int32_t *lig_count;    /* [L]    or NULL */
    int32_t *n_contacts;   /* [P]    or NULL */
    int64_t *score_sum;    /* [P]    or NULL */
    uint64_t *bits;        /* [P,R,ceil(L/64)] or NULL: bit j%64 of word j/64 = contact (i,j); unused high bits 0 */
} dfm_consensus_out;
int dfm_pose_consensus(dfm_model *m, int P, int R, int L, const float *rec_pos, const float *lig_pos,
                       const uint8_t *member_or_null, float cutoff, dfm_consensus_out *out);
/* poses per chunk of a dfm_pose_consensus call on an R + L complex (host arithmetic; < 1 for R or L < 1) */
int dfm_consensus_chunk_poses(int R, int L);
/* GPU milliseconds of the calling thread's last dfm_pose_consensus, summed over its chunks and passes: the host-to-device copies of the
 * poses and the kernels (k_contact_bits, k_contact_count, k_contact_marginals, k_contact_score) - tools/consensus_bench.py */
int dfm_consensus_last_timing(double *copy_ms, double *kernel_ms);
/* All-atom clash and contact screen of P rigid poses of one ligand (CAPRI's steric rule): the only calls that read atoms beyond the
 * backbone.  dfmdock_amd/sterics.py is the float64 definition these calls are tested against.  rec_atoms [Ar,3] and lig_atoms [Al,3] are
 * heavy atoms (the caller filters hydrogens); center [3] is the point the sampler rotates the ligand about (the CA centroid for the
 * first model family, the all-atom mean for the second); a pose is (rot [3] axis-angle, tr [3]) = dfm_traj_out.rot_update / tr_update.
 *   pose p of ligand atom a: (a - center) R(rot_p)^T + center + tr_p in fp64 on the fp32 inputs, R as the host's axis_angle_to_matrix
 *     (small-angle branch below 1e-6 rad); distance of a pair: sqrt((dx*dx + dy*dy) + dz*dz) in fp64.
 *   n_clash [P]: pairs (receptor atom, ligand atom) closer than clash_cutoff (strict; default 3.0).  n_contact [P]: pairs closer than
 *     contact_cutoff (default 5.0, >= clash_cutoff).  min_dist [P]: the smallest distance among the pairs below contact_cutoff, +inf
 *     without one.  lig_clash / lig_contact [P,Al]: the same counts per ligand atom, in the caller's atom order.
 *   A NaN distance is neither: a pose with a NaN or infinite rot / tr gets 0, 0 and +inf and disturbs no other pose (not an error).
 * dfm_atoms_create bins the receptor atoms into a uniform grid whose cell edge is contact_cutoff (a counting sort on the host, once),
 * sorts the ligand atoms spatially into blocks of 64 and uploads both; the handle is read-only afterwards.  dfm_atoms_info: the number
 * of cells, the most atoms in one cell, the cell edge.
 * Every output pointer may be NULL.  Counts are integers and min_dist a minimum: apart from pairs whose distance rounds onto a cutoff
 * the results equal the definition, and none depends on P, on a pose's index, on the order of the poses or on the chunks of a call.
 * Per-atom output is produced chunk_poses poses at a time (0: as many as fill 64 MiB of it; without per-atom output: 32768, the launch
 * limit); dfm_pose_sterics_chunked overrides the creator's chunk_poses for one call.
 * DFM_E_INVALID / NULL, nothing enqueued: NULL m / rec_atoms / lig_atoms / center (a / rot / tr / out), Ar or Al < 1 or > 2^24, a cutoff
 * not finite or <= 0, contact_cutoff < clash_cutoff, chunk_poses < 0, a non-finite receptor atom, ligand atom or centre, a receptor
 * bounding box of more than 2^24 cells, P < 1.  Counts are int32: a pose may have at most 2^31 - 1 pairs below the contact cutoff.
 * DFM_E_OOM when the atoms or a chunk's per-atom output do not fit.
 * Takes the MODEL handle for its device only.  Every call owns a non-blocking stream and its device temporaries, so calls on one handle
 * may run from several host threads at once and next to that model's sampling handles.  No reference call has a counterpart. */
typedef struct dfm_atoms dfm_atoms;
typedef struct {
    float clash_cutoff, contact_cutoff;
    int chunk_poses;       /* 0: default */
} dfm_sterics_params;
typedef struct {
    int32_t *n_clash, *n_contact;      /* [P]    or NULL */
    double *min_dist;                  /* [P]    or NULL */
    int32_t *lig_clash, *lig_contact;  /* [P,Al] or NULL */
} dfm_sterics_out;
dfm_atoms *dfm_atoms_create(dfm_model *m, int Ar, const float *rec_atoms, int Al, const float *lig_atoms, const float center[3],
                            const dfm_sterics_params *p_or_null);
void dfm_atoms_destroy(dfm_atoms *a);
int dfm_atoms_info(const dfm_atoms *a, int32_t *n_cells, int32_t *max_cell_atoms, float *cell_edge);
int dfm_pose_sterics(dfm_atoms *a, int P, const float *rot, const float *tr, dfm_sterics_out *out);
int dfm_pose_sterics_chunked(dfm_atoms *a, int P, const float *rot, const float *tr, int chunk_poses, dfm_sterics_out *out);
/* GPU milliseconds of the calling thread's last dfm_pose_sterics, summed over its chunks: the host-to-device copies of the poses and
 * the kernels (k_sterics_pose, k_sterics, the memsets of the per-atom output) - tools/sterics_bench.py */
int dfm_sterics_last_timing(double *copy_ms, double *kernel_ms);
/* diagnostic (tools/sterics_bench.py): counts_or_null [3] receives, of the calling thread's last counted dfm_pose_sterics, the waves
 * launched (poses x blocks of 64 ligand atoms), those that left at the block's sphere test and those that left at its box test;
 * `enable` != 0 makes this thread's next calls count (one atomic per leaving wave: not for timing) */
int dfm_sterics_exit_counts(int enable, uint64_t *counts_or_null);
/* Buried solvent-accessible surface area (Shrake-Rupley) of P rigid poses of one ligand.  dfmdock_amd/surface.py is the float64
 * definition these calls are tested against.  Atoms, centre and poses as for dfm_atoms_create / dfm_pose_sterics; rec_radius [Ar] and
 * lig_radius [Al] are van der Waals radii.
 *   sphere points: dirs [K,3], K a multiple of 64 in 64 .. 256 (default 128).  The definition's table is the golden spiral z_k =
 *     1 - (2k+1)/K, r_k = sqrt(1 - z_k^2), phi_k = k pi (3 - sqrt 5), u_k = (r cos phi, r sin phi, z) rounded to fp32; dirs == NULL
 *     computes it with the C library, whose cos / sin may round differently from another one's (the Python wrapper passes its table).
 *   R_i = (double)radius_i + (double)probe (default 1.4).  Both chains together hold at most 16 distinct radius values (fp32 bit
 *     patterns); the class of an atom is the index of its value in their ascending list.
 *   distance: d = sqrt((dx*dx + dy*dy) + dz*dz) in fp64.  Point k of atom i of a chain in its input frame is c_i + R_i u_k (fp64,
 *     component-wise); it is exposed iff no OTHER atom j of that chain has d < R_j (strict).  Taken once, at creation.
 *   pose p: x_a as dfm_pose_sterics moves ligand atom a; w_k = (R[:,0] u0 + R[:,1] u1) + R[:,2] u2 with R = R(rot_p); the ligand point
 *     is x_a + R_a w_k, the receptor point c_b + R_b u_k.  A point is buried in pose p iff it is exposed and some atom j of the OTHER
 *     chain has d < R_j (strict).  A NaN distance buries nothing: a pose with a NaN or infinite rot / tr gets all zeros (not an error).
 *   lig_buried [P,Al], rec_buried [P,Ar]: buried points per atom, in the caller's atom order; lig_points, rec_points [P]: their sums;
 *     class_points [P,2,16]: the sums per chain (receptor = 0) and radius class; bsa [P] = sum over chain (receptor first) and class
 *     (ascending) of count * (4.0 pi R_c R_c / K), left to right, on the host: equal counts give bitwise equal areas.  bsa is the
 *     total over both sides; the "interface area" is half of it.
 * dfm_surface_info (every pointer may be NULL): the isolated SASA of each chain (class sums in the same order), the exposed points per
 * atom (rec_exposed [Ar], lig_exposed [Al]), the number of radius classes and their values (class_radius [16]), the receptor grid's
 * cells, the most atoms in one cell and the cell edge.
 * Every output pointer may be NULL.  Counts are integers: apart from points whose distance rounds onto a radius the results equal the
 * definition, and none depends on P, on a pose's index, on the order of the poses or on the chunks of a call.  A call works through
 * chunk_poses poses at a time (0: as many as fill 64 MiB of receptor masks - Ar K / 8 bytes per pose - and per-atom output, at most
 * 32768); dfm_pose_bsa_chunked overrides the creator's chunk_poses for one call.
 * DFM_E_INVALID / NULL, nothing enqueued: NULL m / rec_atoms / rec_radius / lig_atoms / lig_radius / center (s / rot / tr / out), Ar or
 * Al < 1 or > 2^24, a non-finite atom, radius, centre, probe or direction, a radius or probe <= 0, K not a multiple of 64 in 64 .. 256,
 * more than 16 radius classes, chunk_poses < 0, a bounding box of either chain of more than 2^24 grid cells, P < 1.
 * DFM_E_OOM when the atoms or a chunk do not fit.
 * Takes the MODEL handle for its device only.  The handle is read-only after creation; every call owns a non-blocking stream and its
 * device temporaries, so calls on one handle may run from several host threads at once.  No reference call has a counterpart. */
typedef struct dfm_surface dfm_surface;
typedef struct {
    float probe;           /* > 0 */
    int K;                 /* sphere points per atom */
    const float *dirs;     /* [K,3] or NULL */
    int chunk_poses;       /* 0: default */
} dfm_surface_params;
typedef struct {
    int32_t *lig_buried;               /* [P,Al]   or NULL */
    int32_t *rec_buried;               /* [P,Ar]   or NULL */
    int32_t *lig_points, *rec_points;  /* [P]      or NULL */
    int32_t *class_points;             /* [P,2,16] or NULL */
    double *bsa;                       /* [P]      or NULL */
} dfm_bsa_out;
dfm_surface *dfm_surface_create(dfm_model *m, int Ar, const float *rec_atoms, const float *rec_radius, int Al, const float *lig_atoms,
                                const float *lig_radius, const float center[3], const dfm_surface_params *p_or_null);
void dfm_surface_destroy(dfm_surface *s);
int dfm_surface_info(const dfm_surface *s, double *sasa_rec, double *sasa_lig, int32_t *rec_exposed, int32_t *lig_exposed,
                     int32_t *n_classes, float *class_radius, int32_t *n_cells, int32_t *max_cell_atoms, float *cell_edge);
int dfm_pose_bsa(dfm_surface *s, int P, const float *rot, const float *tr, dfm_bsa_out *out);
int dfm_pose_bsa_chunked(dfm_surface *s, int P, const float *rot, const float *tr, int chunk_poses, dfm_bsa_out *out);
/* GPU milliseconds of the calling thread's last dfm_pose_bsa, summed over its chunks: the host-to-device copies of the poses and the
 * kernels (k_surface_pose, k_surface, k_surface_finish, the memsets of the masks and of the per-atom output) - tools/surface_bench.py */
int dfm_bsa_last_timing(double *copy_ms, double *kernel_ms);
/* Interface energy of P rigid poses of one ligand: soft Lennard-Jones plus Coulomb with the dielectric eps = dielectric_slope r over the
 * heavy-atom pairs of the two chains within a cutoff - the physics rescoring step of docking pipelines.  dfmdock_amd/ifenergy.py is the
 * float64 definition these calls are tested against.  Atoms, centre and poses as for dfm_atoms_create / dfm_pose_sterics.  Per atom:
 * rmin_half (A, in (0, 8]), sqrt_eps (sqrt(kcal/mol), in [0, 2]), charge (e, |q| <= 4).  Scalars: cutoff (A, in (0, 16]; 8.0 is usual),
 * soft (in [0.5, 1]; 0.6), elec_min_dist (A, >= 1; 3.0), dielectric_slope (> 0; 4.0).  The cutoff is a plain truncation, no switching.
 *   per pair, fp64 on the widened fp32 inputs, in this order of operations (no square root, one division per term):
 *     r2 = (dx*dx + dy*dy) + dz*dz; the pair counts iff r2 < cutoff*cutoff (strict; a NaN is no pair)
 *     Rm = rh_a + rh_b; f = soft*Rm; r2v = r2 < f*f ? f*f : r2; s2 = (Rm*Rm)/r2v; s6 = (s2*s2)*s2; e = se_a*se_b
 *     rep = e*(s6*s6); att = -2.0*(e*s6); m = elec_min_dist; r2c = r2 < m*m ? m*m : r2
 *     elec = ((332.0637/dielectric_slope)*(q_a*q_b))/r2c
 *   each term is rounded on its own to quanta of 2^-20 kcal/mol: Q(x) = (int64) rint(x * 2^20), ties to even.
 *   rep_q, att_q, elec_q [P]: int64 sums of the rounded terms over the pose's pairs; n_pairs [P]: their number; lig_vdw_q (rep + att) and
 *     lig_elec_q [P,Al]: the same sums per ligand atom, in the caller's atom order.  kcal/mol = q * 2^-20.
 *   A pose with a NaN or infinite rot / tr gets zeros and disturbs no other pose (not an error).
 * Every output pointer may be NULL.  The sums are integer sums: the results equal the definition's, and none depends on P, on a pose's
 * index, on the order of the poses or on the chunks of a call.  dfm_iface_create bins the receptor into cells of the cutoff and rejects
 * a complex whose sums could reach 2^62 quanta: pairs of one pose <= Al min(Ar, 27 max_cell_atoms), times the largest term its own
 * parameters allow (dfm_poseprep.h: iface_sum_bound); dfm_iface_info reports cells, the most atoms in one cell, the cell edge and that
 * bound in quanta.  Per-atom output is produced chunk_poses poses at a time (0: as many as fill 64 MiB of it; without it 32768).
 * DFM_E_INVALID / NULL, nothing enqueued: a NULL pointer among the inputs, Ar or Al < 1 or > 2^24, a non-finite atom, centre or
 * parameter, a parameter or scalar outside the limits above, a receptor bounding box of more than 2^24 cells, the sum bound,
 * chunk_poses < 0, P < 1.  DFM_E_OOM when the atoms or a chunk's per-atom output do not fit.
 * Takes the MODEL handle for its device only.  The handle is read-only after creation; every call owns a non-blocking stream and its
 * device temporaries, so calls on one handle may run from several host threads at once.  No reference call has a counterpart. */
typedef struct dfm_iface dfm_iface;
typedef struct {
    int64_t *rep_q, *att_q, *elec_q;   /* [P]    or NULL */
    int64_t *n_pairs;                  /* [P]    or NULL */
    int64_t *lig_vdw_q, *lig_elec_q;   /* [P,Al] or NULL */
} dfm_iface_out;
dfm_iface *dfm_iface_create(dfm_model *m, int Ar, const float *rec_atoms, const float *rec_rmin_half, const float *rec_sqrt_eps,
                            const float *rec_charge, int Al, const float *lig_atoms, const float *lig_rmin_half, const float *lig_sqrt_eps,
                            const float *lig_charge, const float center[3], float cutoff, float soft, float elec_min_dist,
                            float dielectric_slope);
void dfm_iface_destroy(dfm_iface *h);
int dfm_iface_info(const dfm_iface *h, int32_t *n_cells, int32_t *max_cell_atoms, float *cell_edge, double *sum_bound_q);
int dfm_pose_iface_energy(dfm_iface *h, int P, const float *rot, const float *tr, dfm_iface_out *out);
int dfm_pose_iface_energy_chunked(dfm_iface *h, int P, const float *rot, const float *tr, int chunk_poses, dfm_iface_out *out);
/* GPU milliseconds of the calling thread's last dfm_pose_iface_energy, summed over its chunks: the host-to-device copies of the poses
 * and the kernels (k_iface_pose, k_iface, the memsets of the per-atom output) - tools/iface_bench.py */
int dfm_iface_last_timing(double *copy_ms, double *kernel_ms);
/* Residue contacts of P rigid poses of one ligand over all heavy atoms, counted by residue class - which residues touch which, and the
 * input of the contacts-based affinity estimate (IC-NIS).  dfmdock_amd/affinity.py is the float64 definition these calls are tested
 * against.  Atoms, centre and poses as for dfm_atoms_create / dfm_pose_sterics.  rec_res [Ar] / lig_res [Al]: the residue index of each
 * atom, in [0, Rr) / [0, Lr); a residue without atoms is legal and never in contact.  rec_class [Rr] / lig_class [Lr]: 0 apolar, 1
 * polar, 2 charged.  cutoff (A, in (0, 16]; 5.5 is usual).
 *   an atom pair counts iff d = sqrt((dx*dx + dy*dy) + dz*dz) < cutoff (strict), fp64 on the widened fp32 receptor atom and the fp64
 *     ligand atom of the pose; a NaN is no pair.
 *   C_p = the SET of (receptor residue i, ligand residue j) with at least one counting atom pair.
 *   ic [P,6]: |C_p| split by the unordered pair of classes in the order AA, AP, AC, PP, PC, CC (index a (5 - a) / 2 + b, a <= b);
 *     n_pairs [P] = |C_p| = the sum of the six; n_rec_res / n_lig_res [P]: residues with at least one contact; rec_degree [P,Rr] /
 *     lig_degree [P,Lr]: the number of partner residues; contact_bits [P,Lr,W], W = ceil(Rr / 32): bit i & 31 of word i >> 5 of row j
 *     is set iff (i, j) is in C_p.
 *   A pose with a NaN or infinite rot / tr gets zeros and disturbs no other pose (not an error).
 * Every output pointer may be NULL.  Everything is an integer and a set does not depend on the order its members were found in: the
 * results equal the definition's, and none depends on P, on a pose's index, on the order of the poses or on the chunks of a call.  A
 * call works through chunk_poses poses at a time (0: as many as fill 64 MiB of bitmap - Lr W 4 bytes per pose - at most 32768);
 * dfm_rescon_info reports the receptor grid's cells, the most atoms in one cell, the cell edge, W and that default chunk.
 * DFM_E_INVALID / NULL, nothing enqueued: a NULL pointer among the inputs, Ar or Al < 1 or > 2^24, a non-finite atom or centre, Rr or Lr
 * < 1 or > 4096, a residue index out of range, a class above 2, a cutoff outside (0, 16], a receptor bounding box of more than 2^24
 * cells, chunk_poses < 0, P < 1 or > 65536.  DFM_E_OOM when the atoms or a chunk do not fit.
 * Takes the MODEL handle for its device only.  The handle is read-only after creation; every call owns a non-blocking stream and its
 * device temporaries, so calls on one handle may run from several host threads at once.  No reference call has a counterpart. */
typedef struct dfm_rescon dfm_rescon;
typedef struct {
    int32_t *ic;                        /* [P,6]    or NULL */
    int32_t *n_pairs;                   /* [P]      or NULL */
    int32_t *n_rec_res, *n_lig_res;     /* [P]      or NULL */
    int32_t *rec_degree;                /* [P,Rr]   or NULL */
    int32_t *lig_degree;                /* [P,Lr]   or NULL */
    uint32_t *contact_bits;             /* [P,Lr,W] or NULL */
} dfm_rescon_out;
dfm_rescon *dfm_rescon_create(dfm_model *m, int Ar, const float *rec_atoms, const int32_t *rec_res, int Rr, const uint8_t *rec_class, int Al,
                              const float *lig_atoms, const int32_t *lig_res, int Lr, const uint8_t *lig_class, const float center[3],
                              float cutoff);
void dfm_rescon_destroy(dfm_rescon *h);
int dfm_rescon_info(const dfm_rescon *h, int32_t *n_cells, int32_t *max_cell_atoms, float *cell_edge, int32_t *row_words, int32_t *chunk_poses);
int dfm_pose_rescon(dfm_rescon *h, int P, const float *rot, const float *tr, dfm_rescon_out *out);
int dfm_pose_rescon_chunked(dfm_rescon *h, int P, const float *rot, const float *tr, int chunk_poses, dfm_rescon_out *out);
/* GPU milliseconds of the calling thread's last dfm_pose_rescon, summed over its chunks: the host-to-device copies of the poses and the
 * kernels (the memset of the bitmap, k_rescon_pose, k_rescon, k_rescon_finish) - tools/affinity_bench.py */
int dfm_rescon_last_timing(double *copy_ms, double *kernel_ms);
/* The kernel milliseconds of that call by phase, from the call's own events: zeroing the bitmap, the walk (k_rescon_pose, k_rescon) and
 * k_rescon_finish; their sum is kernel_ms */
int dfm_rescon_last_phases(double *zero_ms, double *walk_ms, double *finish_ms);
/* Interface hydrogen bonds and salt bridges of P rigid poses of one ligand over the POLAR atoms of the two chains - what an interface
 * report prints next to the contacts.  dfmdock_amd/hbonds.py is the float64 definition these calls are tested against and types the
 * atoms (polar_atoms).  Heavy atoms only: the files carry no hydrogens; HIS counts as donor, acceptor and cation; no agreement with the
 * counts of any published tool is claimed.  Centre and poses as for dfm_atoms_create / dfm_pose_sterics.  Per chain: xyz [N,3] the polar
 * atoms, ante [N,3] the antecedent of each (the bonded heavy atom its angle is taken at; the ligand's rides with the pose), role [N] bits
 * DONOR 1, ACCEPTOR 2, CATION 4, ANION 8, SIDECHAIN 16, res [N] the residue index of each atom in [0, n_res); a residue without polar
 * atoms is legal.  hb_cutoff, salt_cutoff (A, in (0, 8]; 3.5 and 4.0 are usual); min_cos2 = cos^2 of the smallest angle, in [0, 1) -
 * exactly 0 for 90 degrees - as the double the definition uses.
 *   posed ligand atom X with antecedent XA, receptor atom Y with antecedent YA, fp64 on the widened fp32 receptor and the fp64 pose:
 *     d = Y - X, r2 = (dx*dx + dy*dy) + dz*dz;  u = XA - X, uu = |u|^2, du = u.d;  w = YA - Y, ww = |w|^2, dw = -(w.d)
 *   hydrogen bond iff one atom is a DONOR and the other an ACCEPTOR, r2 < hb_cutoff^2 (strict), du <= 0 and du*du >= min_cos2 (uu r2),
 *     dw <= 0 and dw*dw >= min_cos2 (ww r2); a pair that is complementary in both directions is one bond.  Salt-bridge atom pair iff
 *     one is a CATION and the other an ANION and r2 < salt_cutoff^2; a pair may be both.  A NaN is neither.
 *   n_hbond [P]; hb_kind [P,3]: the bonds by the number of SIDECHAIN atoms among the two (0, 1, 2), summing to n_hbond; n_salt_atoms [P]:
 *     the salt-bridge atom pairs; n_salt [P]: the DISTINCT (receptor residue, ligand residue) pairs with at least one; rec_hb [P,Nr] /
 *     lig_hb [P,Nl]: the bonds each polar atom takes part in, rec_sb / lig_sb: its salt-bridge partners, in the caller's atom order.
 *   A pose with a NaN or infinite rot / tr gets zeros and disturbs no other pose (not an error).
 * Every output pointer may be NULL.  Everything is an integer: the results equal the definition's, and none depends on P, on a pose's
 * index, on the order of the poses or on the chunks of a call.  The salt bridges are found in a bitmap per pose over the charged residues
 * of the two chains (those with a CATION or ANION atom; a chain without one is legal); a call works through chunk_poses poses at a time
 * (0: as many as fill 64 MiB of bitmap, at most 32768).  dfm_hbond_info reports the receptor grid's cells, the most atoms in one cell,
 * the cell edge = max(hb_cutoff, salt_cutoff), the charged residues of the two chains and that default chunk.
 * dfm_hbond_create returns NULL on failure and, with `status` not NULL, stores DFM_OK or the error code there.  DFM_E_INVALID / NULL,
 * nothing enqueued: a NULL pointer among the inputs, Nr or Nl < 1 or > 2^24, a non-finite atom, antecedent or centre, n_rec_res or
 * n_lig_res < 1 or > 4096, a role outside the five bits, a residue index out of range, a cutoff outside (0, 8], min_cos2 outside [0, 1),
 * a receptor bounding box of more than 2^24 cells, chunk_poses < 0, P < 1 or > 65536.  DFM_E_OOM when the atoms or a chunk do not fit.
 * Takes the MODEL handle for its device only.  The handle is read-only after creation; every call owns a non-blocking stream and its
 * device temporaries, so calls on one handle may run from several host threads at once.  No reference call has a counterpart. */
typedef struct dfm_hbond dfm_hbond;
typedef struct {
    int32_t *n_hbond;                   /* [P]      or NULL */
    int32_t *hb_kind;                   /* [P,3]    or NULL */
    int32_t *n_salt, *n_salt_atoms;     /* [P]      or NULL */
    int32_t *rec_hb, *lig_hb;           /* [P,Nr], [P,Nl] or NULL */
    int32_t *rec_sb, *lig_sb;           /* [P,Nr], [P,Nl] or NULL */
} dfm_hbond_out;
dfm_hbond *dfm_hbond_create(dfm_model *m, int Nr, const float *rec_xyz, const float *rec_ante, const uint8_t *rec_role, const int32_t *rec_res,
                            int n_rec_res, int Nl, const float *lig_xyz, const float *lig_ante, const uint8_t *lig_role,
                            const int32_t *lig_res, int n_lig_res, const float center[3], float hb_cutoff, double min_cos2,
                            float salt_cutoff, int *status);
void dfm_hbond_destroy(dfm_hbond *h);
int dfm_hbond_info(const dfm_hbond *h, int32_t *n_cells, int32_t *max_cell_atoms, float *cell_edge, int32_t *n_rec_charged,
                   int32_t *n_lig_charged, int32_t *chunk_poses);
int dfm_pose_hbonds(dfm_hbond *h, int P, const float *rot, const float *tr, dfm_hbond_out *out);
int dfm_pose_hbonds_chunked(dfm_hbond *h, int P, const float *rot, const float *tr, int chunk_poses, dfm_hbond_out *out);
/* GPU milliseconds of the calling thread's last dfm_pose_hbonds, summed over its chunks: the host-to-device copies of the poses and the
 * kernels (the memsets of the bitmap and of the per-atom output, k_hbond_pose, k_hbond, k_hbond_finish) - tools/hbonds_bench.py */
int dfm_hbond_last_timing(double *copy_ms, double *kernel_ms);
/* The kernel milliseconds of that call by phase, from the call's own events: the memsets, the walk (k_hbond_pose, k_hbond) and
 * k_hbond_finish; their sum is kernel_ms */
int dfm_hbond_last_phases(double *zero_ms, double *walk_ms, double *finish_ms);
/* Tabulated pair potential of P rigid poses of one ligand, E = the sum over heavy-atom pairs of table[type_a][type_b][bin(r)] - the
 * shape of DFIRE, DOPE, ITScore-PP, ZRANK's ACE term or a table fitted to one's own decoys - and, optionally, the pair counts
 * N[type_a][type_b][bin] such a potential is a linear function of.  The library ships NO table: the table, its edges and the types come
 * from the caller, and nothing is claimed about the ranking quality of any potential.  dfmdock_amd/pairpot.py is the float64 definition
 * these calls are tested against.  Atoms, centre and poses as for dfm_atoms_create / dfm_pose_sterics.  rec_type [Ar] / lig_type [Al]:
 * the type of each atom, in [0, T), 1 <= T <= 256.  edges [NB+1]: 1 <= NB <= 64, finite, strictly ascending, edges[0] >= 0, edges[NB] <=
 * 16 (A); the cutoff is edges[NB].  table [T,T,NB]: kcal/mol, indexed (LIGAND type, RECEPTOR type, bin), finite, |x| <= 1024; it need
 * not be symmetric.
 *   table_q = (int64) rint((double) table * 2^20), ties to even: quanta of 2^-20 kcal/mol, |q| <= 2^30.
 *   e2[k] = (double) edges[k] * (double) edges[k], which is exact.  Per pair, fp64 on the widened fp32 receptor atom and the fp64 ligand
 *     atom of the pose: r2 = (dx*dx + dy*dy) + dz*dz; the pair counts iff e2[0] <= r2 < e2[NB] (a NaN is no pair); its bin is
 *     k = #{j : e2[j] <= r2} - 1.  No square root is taken anywhere.
 *   energy_q [P]: the int64 sum of table_q[ta][tb][k] over the pose's pairs; n_pairs [P]: their number, also where the table holds 0;
 *     lig_q [P,Al]: the same sum per ligand atom, in the caller's atom order; counts [P,T,T,NB]: the pairs by (ligand type, receptor
 *     type, bin), so that sum(counts) = n_pairs and <counts, table_q> = energy_q.  kcal/mol = q * 2^-20.
 *   A pose with a NaN or infinite rot / tr gets zeros and disturbs no other pose (not an error).
 * Every output pointer may be NULL.  Everything is an integer sum: the results equal the definition's, and none depends on P, on a
 * pose's index, on the order of the poses or on the chunks of a call.  counts costs one global atomic per pair and is the slow path; a
 * call without it runs a kernel that holds none of that code.  dfm_pairpot_create bins the receptor into cells of edges[NB] and refuses
 * a complex whose poses could have more than 2^31 - 1 pairs in range - pairs of one pose <= Al min(Ar, 27 max_cell_atoms)
 * (dfm_poseprep.h: pairpot_pair_bound) - so that counts fits int32 and |energy_q| < 2^61; dfm_pairpot_info reports cells, the most
 * atoms in one cell, the cell edge, that bound, T and NB.  A call works through chunk_poses poses at a time (0: the creator's, and if
 * that is 0 too as many as fill 64 MiB of counts plus lig_q, whichever the call asks for; without either 32768).
 * DFM_E_INVALID / NULL, nothing enqueued, the first of these in this order: a NULL m; a NULL atom set or centre, Ar or Al < 1 or > 2^24,
 * a non-finite atom or centre; a NULL rec_type or lig_type; T outside 1 .. 256; NB outside 1 .. 64, NULL edges, an edge that is not
 * finite, not above its predecessor, below 0 or above 16; a NULL table, an entry that is not finite or above 1024 in magnitude; a type
 * out of range (receptor first); chunk_poses < 0; a receptor bounding box of more than 2^24 cells; the pair bound; a ligand whose
 * extent about the centre overflows fp32.  For a call: a NULL h, rot, tr or out, P < 1, chunk_poses < 0.  DFM_E_OOM when the atoms, the
 * table or a chunk's output do not fit.
 * Takes the MODEL handle for its device only.  The handle is read-only after creation; every call owns a non-blocking stream and its
 * device temporaries, so calls on one handle may run from several host threads at once.  No reference call has a counterpart. */
typedef struct dfm_pairpot dfm_pairpot;
typedef struct {
    int64_t *energy_q;                  /* [P]        or NULL */
    int64_t *n_pairs;                   /* [P]        or NULL */
    int64_t *lig_q;                     /* [P,Al]     or NULL */
    int32_t *counts;                    /* [P,T,T,NB] or NULL */
} dfm_pairpot_out;
dfm_pairpot *dfm_pairpot_create(dfm_model *m, int Ar, const float *rec_atoms, const int32_t *rec_type, int Al, const float *lig_atoms,
                                const int32_t *lig_type, const float center[3], int T, int NB, const float *edges, const float *table,
                                int chunk_poses);
void dfm_pairpot_destroy(dfm_pairpot *h);
int dfm_pairpot_info(const dfm_pairpot *h, int32_t *n_cells, int32_t *max_cell_atoms, float *cell_edge, double *pair_bound, int32_t *T,
                     int32_t *NB);
int dfm_pose_pairpot(dfm_pairpot *h, int P, const float *rot, const float *tr, dfm_pairpot_out *out);
int dfm_pose_pairpot_chunked(dfm_pairpot *h, int P, const float *rot, const float *tr, int chunk_poses, dfm_pairpot_out *out);
/* GPU milliseconds of the calling thread's last dfm_pose_pairpot, summed over its chunks: the host-to-device copies of the poses and the
 * kernels (the memsets of lig_q and counts, k_pairpot_pose, k_pairpot) - tools/pairpot_bench.py */
int dfm_pairpot_last_timing(double *copy_ms, double *kernel_ms);
/* The kernel milliseconds of that call by phase, from the call's own events: the memsets, the walk (k_pairpot_pose, k_pairpot) and the
 * finish, which this call does not have (about 0); their sum is kernel_ms */
int dfm_pairpot_last_phases(double *zero_ms, double *walk_ms, double *finish_ms);
/* Rigid pose fit of P decoys of one complex: from the backbone coordinates of a rigidly placed ligand back to the pose
 * (rot_update, tr_update) of dfm_traj_out, the one form every dfm_pose_* call, dfm_refine's start and the drivers' output path take -
 * the door for decoys this engine did not sample.  dfmdock_amd/fit.py (fit_poses) is the float64 definition this call is tested
 * against.  Backbones are [n,9] = (N, CA, C) per residue; the points of a fit are all 3 n atoms with equal weights.
 *   lig_ref [L,9]: the input ligand, lig_pos [P,L,9]: the decoys' ligands, center: the point the sampler rotates the ligand about
 *   (CA centroid of lig_ref for family 0, backbone centroid for family 1).  rec_ref_or_null [R,9] and rec_pos_or_null [P,R,9], both or
 *   neither: the input receptor and the decoys' receptors, for decoys that sit in a frame of their own.
 *   With a receptor, (Q, s) is the Kabsch fit of rec_pos[p] onto rec_ref (the proper rotation the SVD gives with its reflection fix),
 *   rec_rmsd the root mean square of |Q y + s - y_ref|, and the decoy's ligand becomes x' = Q x + s; without one x' = x.  (R, t) is the
 *   Kabsch fit of lig_ref onto x' and rmsd the root mean square of the explicit residuals |R x0 + t - x'| - above a tolerance of the
 *   caller's the decoy is no rigid image of the input.  rot = the axis-angle of R, angle in [0, pi], taken from Horn's quaternion
 *   (exactly zero for the identity); tr = t + R c - c, so that x = (x0 - c) R(rot)^T + c + tr.
 *   Everything is fp64 on the fp32 inputs; rot and tr are rounded to fp32 at the end.  A pose with a non-finite coordinate has rot, tr,
 *   rmsd and rec_rmsd NaN and leaves the other poses alone.  A pose's outputs depend on that pose and the references alone - not on P,
 *   its index, or how the call splits P into chunks (64 MiB of decoys each; dfm_pose_fit_chunked: chunk_poses > 0 poses each).
 * DFM_E_INVALID: a NULL m / lig_ref / lig_pos / center / out / out->rot / out->tr / out->rmsd, P < 1, L < 1, exactly one of the two
 * receptor pointers, R < 1 or a NULL out->rec_rmsd_or_null with a receptor, chunk_poses < 0.  Takes the MODEL handle for its device
 * only; every call owns a non-blocking stream and its device temporaries, so calls may run from several host threads at once.  The
 * reference has no such call: it replaces the host-side Kabsch fit a user of the reference would write around the rot_update /
 * tr_update bookkeeping of src/inference_base.py to bring outside decoys into its convention. */
typedef struct {
    float *rot;                 /* [P,3] */
    float *tr;                  /* [P,3] */
    double *rmsd;               /* [P]   */
    double *rec_rmsd_or_null;   /* [P], needed with a receptor */
} dfm_fit_out;
int dfm_pose_fit(dfm_model *m, int P, int L, const float *lig_ref /*[L,9]*/, const float *lig_pos /*[P,L,9]*/, int R,
                 const float *rec_ref_or_null /*[R,9]*/, const float *rec_pos_or_null /*[P,R,9]*/, const float center[3], dfm_fit_out *out);
int dfm_pose_fit_chunked(dfm_model *m, int P, int L, const float *lig_ref, const float *lig_pos, int R, const float *rec_ref_or_null,
                         const float *rec_pos_or_null, const float center[3], int chunk_poses, dfm_fit_out *out);
/* GPU milliseconds of the calling thread's last dfm_pose_fit, summed over its chunks: the host-to-device copies of the decoys and the
 * three kernels (k_fit_reduce, k_fit_solve, k_fit_resid) - tools/fit_bench.py */
int dfm_fit_last_timing(double *copy_ms, double *kernel_ms);
/* Cryo-EM density fit of P rigid poses of one ligand: which of these models does the map support?  Per pose and channel the sum over
 * the ligand's atoms of w_a times the trilinear value of a 3-D grid at the posed atom - a gather, not a cell walk - plus the atoms inside
 * the grid and those in density above a threshold.  dfmdock_amd/density.py is the float64 definition these calls are tested against, and
 * holds the host finishes (MRC files, simulated maps, the closed-form correlation).  Nothing is claimed about ranking quality on real maps.
 *   Frame: the receptor's coordinates are taken to be in the map's frame; fitting the receptor into the map is not done.  Centre and
 *     poses as for dfm_atoms_create / dfm_pose_sterics: pose p of atom a is (a - center) R(rot_p)^T + center + tr_p in fp64.
 *   Grid: grids [C,nz,ny,nx] float32, 1 <= C <= 4 channels on ONE orthogonal grid, 2 <= n <= 1024 nodes per axis, every value finite and
 *     at most 2^10 in magnitude; origin [3] and voxel [3] float32 in A, (x, y, z), voxel finite and in (0, 16] and possibly anisotropic;
 *     node (iz, iy, ix) sits at origin + (ix, iy, iz) * voxel.  lig_w [Al]: the atoms' weights, finite, |w| <= 2^7.
 *   One atom, one channel, everything widened to fp64, in this order, nothing contracted:
 *     ux = (x - ox) / vx ; ix = floor(ux) ; fx = ux - ix        (same for y, z)
 *     inside  iff 0 <= ux < nx-1 and 0 <= uy < ny-1 and 0 <= uz < nz-1   (NaN is outside)
 *     c00 = c000 + fx*(c100 - c000) ; c10 = c010 + fx*(c110 - c010)      (cXYZ: the node at ix+X, iy+Y, iz+Z)
 *     c01 = c001 + fx*(c101 - c001) ; c11 = c011 + fx*(c111 - c011)
 *     c0  = c00  + fy*(c10 - c00)   ; c1  = c01  + fy*(c11 - c01)
 *     val = c0   + fz*(c1 - c0)
 *     term_q = (int64) rint((w_a * val) * 2^20), ties to even; 0 for an outside atom.  No square root, no transcendental.
 *   sum_q [P,C]: the int64 sums of term_q; n_inside [P]: the atoms inside; n_above [P]: the inside atoms whose channel-0 val >= threshold
 *     (a float32, widened); atom_q [P,Al]: term_q of channel 0, in the caller's atom order.  Values are q * 2^-20.
 *   A pose with a NaN or infinite rot / tr gets zeros and disturbs no other pose (not an error).
 * Every output pointer may be NULL.  Everything is an integer sum: the results equal the definition's, and none depends on P, on a
 * pose's index, on the order of the poses or on the chunks of a call.  |term_q| <= 2^37; dfm_density_create refuses a ligand whose
 * Al * 2^37 quanta could reach 2^62 (dfm_poseprep.h: density_sum_bound).  The device holds the grid channel-interleaved, 16 bytes per
 * node.  dfm_density_info reports the grid's shape, C, the poses of a chunk of a call with atom_q and that bound.  A call works through
 * chunk_poses poses at a time (0: as many as fill 64 MiB of atom_q; without atom_q 32768).
 * DFM_E_INVALID / NULL (*err, when given, holds the code), nothing enqueued, the first of these in this order: a NULL m; C outside 1 .. 4,
 * an axis outside 2 .. 1024, a NULL origin, voxel or grids, a non-finite origin, a voxel outside (0, 16], a grid value that is not finite
 * or above 2^10 in magnitude; a NULL lig_atoms, lig_w or center, Al < 1 or > 2^24, a non-finite atom, a weight that is not finite or
 * above 2^7 in magnitude, a non-finite centre; a threshold that is not finite; the sum bound.  For a call: a NULL h, rot, tr or out,
 * P < 1, chunk_poses < 0.  DFM_E_OOM when the grid, the atoms or a chunk's output do not fit.
 * Takes the MODEL handle for its device only.  The handle is read-only after creation; every call owns a non-blocking stream and its
 * device temporaries, so calls on one handle may run from several host threads at once.  No reference call has a counterpart. */
typedef struct dfm_density dfm_density;
typedef struct {
    int64_t *sum_q;                     /* [P,C]  or NULL */
    int32_t *n_inside;                  /* [P]    or NULL */
    int32_t *n_above;                   /* [P]    or NULL */
    int64_t *atom_q;                    /* [P,Al] or NULL */
} dfm_density_out;
dfm_density *dfm_density_create(dfm_model *m, int nx, int ny, int nz, const float origin[3], const float voxel[3], int C,
                                const float *grids, int Al, const float *lig_atoms, const float *lig_w, const float center[3],
                                float threshold, int *err);
void dfm_density_destroy(dfm_density *h);
int dfm_density_info(const dfm_density *h, int32_t *nx, int32_t *ny, int32_t *nz, int32_t *C, int32_t *chunk_poses, double *sum_bound);
int dfm_pose_density(dfm_density *h, int P, const float *rot, const float *tr, dfm_density_out *out);
int dfm_pose_density_chunked(dfm_density *h, int P, const float *rot, const float *tr, int chunk_poses, dfm_density_out *out);
/* GPU milliseconds of the calling thread's last dfm_pose_density, summed over its chunks: the host-to-device copies of the poses and the
 * kernels (k_density_pose, k_density) - tools/density_bench.py */
int dfm_density_last_timing(double *copy_ms, double *kernel_ms);
/* edges per node for this complex: min(N,20) + min(40, N-20) */
int dfm_complex_degree(const dfm_complex *cx);
/* Device blocks released by destroyed handles are parked per device for the next handle (a set driver creates and destroys a
 * complex every ~100 ms; hipMalloc / hipFree of gigabyte workspaces cost milliseconds and drain the device): at most
 * DFM_ALLOC_CACHE_FRAC (default 0.25) of the device's memory, DFM_ALLOC_CACHE=0 disables it.  dfm_trim_cache hands every parked
 * block of `device` (< 0: all devices; an index past the last device: nothing, returns 0) back to the driver - for processes that
 * share a GPU - and returns the bytes freed. */
long long dfm_trim_cache(int device);
/* What the allocator's two diagnostics did in this process so far (DFM_ALLOC_POISON=<byte> fills every device block handed out,
 * DFM_ALLOC_GUARD=<KiB> puts bands of 0xA5 around it and checks them at release): out[0] blocks handed out, out[1] bytes filled
 * with the poison byte, out[2] guard bands checked, out[3] guard bands found damaged, out[4] / out[5] the size of the first damaged
 * block and the damaged byte's offset from the block's start (negative: head band; >= size: tail band), both -1 while no band is
 * damaged.  Without the variables only out[0] counts. */
int dfm_alloc_diag(int64_t out[6]);

/* NON-FINITE POSES IN THE TRUNK CALLS (dfm_score, dfm_score_distogram, dfm_sample, dfm_refine, dfm_complex_selfcheck).
 * A pose can carry a NaN or an infinite coordinate: dfm_score, dfm_score_distogram and dfm_refine(start_pos) take host poses
 * unchecked, an injected tr_draw or R0 can be NaN, and the restraint and symmetry steps give a non-finite pose a NaN step.
 * Such a pose is not an error of the call.  What holds for it (tests/test_gpu_nonfinite.py, launch by launch in
 * tests/test_gpu_geom_kernels.py and tests/test_gpu_head_kernels.py):
 *   1. In range.  Whatever the coordinates, every index a kernel forms from them stays inside its array: graph edges are residue
 *      indices in [0, N), and so are the positions in the row list and the layer-0 table that follow from them.
 *   2. Contained.  A pose (trajectory) with a non-finite coordinate changes no bit of any other pose's outputs in the same call.
 *   3. Visible.  The pose preparation marks a pose with a NaN or infinite coordinate in ANY backbone atom: every prepared coordinate
 *      of it is NaN.  Its tr_score, rot_score, energy and f are NaN - the energy too, although no residue pair of it passes
 *      D < cut_off - and from dfm_sample / dfm_refine also its lig_pos, rot_update and tr_update, from the first evaluation that
 *      sees the coordinate on.  num_clashes of such a pose is 0 (no pair passes D <= 3; an integer has no NaN).
 *      The clash force (DFM_F_CLASH_FORCE) does the same on its own: a pose with a non-finite coordinate in any atom gets a NaN
 *      shift - its whole pose and tr_update are NaN - instead of a finite shift from the atoms that are numbers.
 *      dfm_score_distogram: its nll, nll_near and exp_contacts are NaN, n_near is 0, its slices of the per-pair maps are NaN, and
 *      EVERY entry of pcontact_mean is NaN, since that map is the mean over all B poses.
 *   4. Stored poses are refused.  The layer-0 message table and the layer-0 operands are built from the stored pose:
 *      dfm_complex_create and dfm_complex_set_pose return NULL / DFM_E_INVALID for a NaN or infinite value in rec_pos or lig_pos,
 *      before anything is created, copied or enqueued; dfm_complex_set_pose then keeps BOTH stored poses as they were.  So
 *      dfm_complex_selfcheck, which runs the stored pose, never sees one.
 *   5. Ordering rule of the graph.  Of the C-alpha distances of a node, a NaN (either sign, any payload) orders after every
 *      number, +inf included, and all NaN tie; ties go by ascending residue index.  Only residues are candidates (j < N: no
 *      padding slot of the selection is ever taken).  In the sampling race a candidate at a NaN distance (NaN race key) is drawn
 *      only after every candidate with a number key; a residue at +inf has the key +inf.  A node none of whose distances is a
 *      number (every node of a marked pose) therefore has the kNN slots 0 .. knn-1 and the next nsamp residues. */

/* B score evaluations of poses lig_pos[B,L,9] at times t[B].  Non-finite poses: see above (rules 1-3). */
int dfm_score(dfm_complex *cx, int B, const float *lig_pos, const float *t, const int32_t *edges_or_null,
              uint64_t seed, uint32_t flags, dfm_score_out *out);

/* The distogram head of the second family (EGNN_Net.to_dist, egnn_net.py:347-352,:447) reduced on the device: for every pose the
 * 64-bin logits z of each receptor / ligand residue pair are turned, inside the pair kernel, into
 *   pair_nll = -log_softmax(z)[bin(D)]      D: the pose's own CA-CA distance; bin(d) = #{k : d^2 > bounds[k]^2},
 *                                           bounds = linspace(3.25, 50.75, 63) (utils/loss.py:65-93, distogram_loss)
 *   pcontact = sum_{k < contact_bins} softmax(z)[k]        edist = sum_k softmax(z)[k] centre[k],  centre[k] = 3.25 + (k - 0.5) step
 * and per pose nll = mean over the R L pairs (the reference's distogram_loss of the pose against its own prediction), nll_near / n_near
 * = mean / count over pairs with D < near_cutoff (n_near = 0: NaN), exp_contacts = sum of pcontact.  pcontact_mean[R,L] is the mean of
 * pcontact over the B poses, added in index order in double.  The logits are never stored (DFM_F_DIST returns them).  fp32 throughout in
 * every engine; fixed-order reductions, no atomics: a pose's numbers do not depend on B, on its index or on which maps are asked for.
 * The forward is dfm_score's (same arguments; flags: the engine flags DFM_F_MFMA16 / DFM_F_F16 / DFM_F_BF16_OPS only).
 * DFM_E_INVALID, nothing enqueued: a NULL required pointer, B < 1, a family-0 model, contact_bins outside 1..63, any other flag.
 * A pose with a non-finite coordinate (rules 1-3 above): its per-pose outputs and map slices are NaN (n_near 0), every entry of
 * pcontact_mean is NaN, and the other poses keep their bits. */
typedef struct {
    int32_t contact_bins;   /* bins 0 .. contact_bins - 1 count as contact: 7 <-> d <= 7.85 A */
    float near_cutoff;      /* <= 0: the model's cut_off */
} dfm_distogram_params;
typedef struct {
    float *nll;             /* [B]      required */
    float *nll_near;        /* [B]      required */
    int32_t *n_near;        /* [B]      required */
    float *exp_contacts;    /* [B]      required */
    float *pair_nll;        /* [B,R,L]  or NULL */
    float *pcontact;        /* [B,R,L]  or NULL */
    float *edist;           /* [B,R,L]  or NULL */
    float *pcontact_mean;   /* [R,L]    or NULL */
} dfm_distogram_out;
int dfm_score_distogram(dfm_complex *cx, int B, const float *lig_pos, const float *t, const int32_t *edges_or_null,
                        uint64_t seed, uint32_t flags, const dfm_distogram_params *params, dfm_distogram_out *out);
/* GPU milliseconds of the calling thread's last dfm_score_distogram: the copies (poses and times up, results down) and everything
 * between them (forward, to_dist.0 projection, k_pair_dist_sum, k_dist_finish, k_dist_mean) - tools/distogram_bench.py */
int dfm_distogram_last_timing(double *copy_ms, double *kernel_ms);

/* B independent trajectories of the Euler-Maruyama sampler.  A trajectory whose pose becomes non-finite (an injected NaN draw, a NaN
 * step) stays NaN to the end and leaves the others alone: rules 1-3 of "non-finite poses" above. */
int dfm_sample(dfm_complex *cx, int B, int num_steps, float eps, float tr_noise_scale, float rot_noise_scale,
               uint32_t flags, uint64_t seed, const dfm_inject *inj_or_null, dfm_traj_out *out);

/* Local refinement: B trajectories that start from a given pose instead of randomize_pose.  Trajectory b starts from
 * p->start_pos[b] (NULL: the stored ligand pose of the complex), noised with the forward marginal at p->t_begin unless p->perturb is 0,
 * and runs dfm_sample's steps over linspace(t_begin, eps, num_steps) (t_begin = 1: dfm_sample's grid bit for bit); flags, the noise
 * scales and inj->z_rot / z_tr / edges mean what they mean for dfm_sample.  rot_update / tr_update start as the noise rotation /
 * translation and are composed as in dfm_sample: they map the START pose of a trajectory onto its final pose; init_pose is the pose
 * after the start.  A start_pos[b] that is a rigid motion of the stored ligand pose hits the layer-0 message table; any other conformer
 * misses edge by edge and goes through the edge model (the rule of DFM_F_L0_TABLE).  DFM_E_INVALID, nothing enqueued: p NULL, t_begin
 * NaN, <= eps or > 1, num_steps < 2, inj->R0 or inj->tr_draw set (they belong to randomize_pose; the start is injected through rinj).
 * start_pos is not checked: a start_pos[b] with a NaN or infinite coordinate gives trajectory b NaN outputs and leaves the others alone
 * (rules 1-3 of "non-finite poses" above). */
int dfm_refine(dfm_complex *cx, int B, int num_steps, float eps, float tr_noise_scale, float rot_noise_scale, uint32_t flags,
               uint64_t seed, const dfm_refine_params *p, const dfm_inject *inj_or_null, const dfm_refine_inject *rinj_or_null,
               dfm_traj_out *out);
/* The draws dfm_refine starts from at t_begin = t, by the same kernel: rotation vectors rot [B,3] (axis-angle) and translations
 * tr [B,3] of B trajectories with `seed` (or the injected draws).  0 <= t <= 1. */
int dfm_forward_marginal(dfm_complex *cx, int B, float t, uint64_t seed, const dfm_refine_inject *rinj_or_null, float *rot, float *tr);
/* The IGSO(3) table dfm_refine looks rotation angles up in at time t: the index of sigma_so3(t) on the reference's 1000-point sigma
 * grid (the grid value below it, so3_diffuser.py:199-206), that sigma, and the cdf [1000] over omega_k = k pi / 1000 (float64, computed
 * on the device once per index and cached on the model handle).  Any output pointer may be NULL. */
int dfm_igso3_table(dfm_model *m, double t, int *sigma_idx, double *sigma, double *cdf);

int dfm_get_profile(const dfm_complex *cx, dfm_profile *p);

/* Runs the stored pose of the complex (dfm_complex_create / dfm_complex_set_pose) through the fp32 engine and through the 16-bit
 * engine `flags` selects (DFM_F_MFMA16, the default when neither is given, or DFM_F_F16; DFM_F_BF16_OPS is honoured) on the same
 * n_eval (1..16) engine-drawn graphs at times t[n_eval] (NULL: spread over [1, 0.001]) and fills `out` (see dfm_selfcheck_out).
 * Costs one fp32 + one 16-bit batched evaluation of n_eval poses (about 0.1 s at 300+300); the drivers call it once per complex.
 * The stored pose is finite by construction (rule 4 of "non-finite poses" above). */
int dfm_complex_selfcheck(dfm_complex *cx, int n_eval, const float *t_or_null, uint64_t seed, uint32_t flags, dfm_selfcheck_out *out);

/* which: 0 = R^3 (VE), 1 = SO(3) (logarithmic).  Returns DFM_E_INVALID for t outside [0,1] on SO(3). */
int dfm_diffusion_coef(const dfm_hparams *hp, int which, double t, double *g_out, double *sigma_out);

#ifdef __cplusplus
}
#endif
#endif /* DFMDOCK_AMD_H */

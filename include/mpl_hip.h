/*
 * mpl_hip.h -- C ABI of libmpl_hip.so: the MI355X (gfx950) implementation of OpenMPL's
 * multi-view pose-lifting forward pass.
 *
 * The reference has no FFI layer: its "operator API" for this path is the Python
 * nn.Module contract of MPL/lib/models/multiview_mpl.py.  This
 * header is the boundary a binding for that contract calls: plain pointers and sizes,
 * no torch types.  All `const float*` below are DEVICE pointers to fp32 data in the
 * reference's own parameter layouts (nn.Linear weight = [out][in] row-major, i.e. the
 * tensors of the reference state_dict are consumed as they are).  The one exception is
 * optional DERIVED data: the packed fp16x2 / bf16 copies of the FPT Linear weights that
 * mpl_pack_h2 / mpl_pack_bf16 build from those tensors; whoever hands them over
 * must rebuild them when the source parameters change (the Python binding keys them on
 * the parameters' storage addresses and versions).
 * `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); every call only
 * enqueues work on it and never synchronises.  Every function returns 0 on success or a
 * negative MPL_E_* code (mpl_hip_error_string() explains it); nothing falls back to a CPU
 * path.
 *
 * Reference interface each entry point replaces (file:line in /root/reference/MPL/lib/models/):
 *   mpl_forward            MultiView_MPL.forward              multiview_mpl.py:450-525
 *   mpl_spt_tokens         Spatial_forward_features + per-view glue   :349-414, :458-499
 *   mpl_block_stack        the `for blk in self.blocks` loop of forward_features  :420-423
 *                          (Block :84-92, Attention :53-67, Mlp :31-37)
 *   mpl_ln_linear          nn.LayerNorm + nn.Linear (+GELU | +residual) pairs inside Block
 *   mpl_token_attention    Attention.forward minus the two Linear layers   :55-64
 *   mpl_fuse_head          forward_features tail :425-446 + default head :283-286,:521-523
 *   mpl_triangulate_rays   lib/multiviews/triangulate.py (the triangulation baseline)
 *   mpl_epipolar_errors    lib/utils/calib.py:94-169 (distance_between_two_skew_lines, smart_pseudo_remove_weight)
 *   mpl_triangulate_robust lib/multiviews/triangulate.py:88-112 (view selection by confidence) + pair consensus
 *   mpl_procrustes_align   lib/utils/pose_utils.py:61-143 (PoseUtils.procrustes, one numpy SVD per pose)
 *   mpl_synthesize_views   lib/dataset/multiview_amass_h36m_mpl.py:317-342 + joints_dataset_mpl.py:588-774 (synthetic detections)
 *   mpl_decode_heatmaps    lib/core/inference.py:22-81 (get_max_preds, get_final_preds) + lib/utils/transforms.py:51-94
 *   mpl_decode_heatmaps_ex the same with a sub-pixel peak: the intent of lib/core/inference.py:84-134 (find_tensor_peak_batch)
 *   mpl_render_heatmaps    lib/dataset/joints_dataset_mpl.py:828-870 (generate_heatmap)
 *   mpl_rpsm               lib/multiviews/pictorial.py:18-247 (rpsm, recursive_infer, infer, compute_unary_term, compute_grid)
 *   mpl_undistort_points   lib/multiviews/cameras.py:22-46 (project_point_radial) and its inverse, which the reference leaves to
 *                          pymvg on the host (lib/multiviews/triangulate.py:26-38)
 *   mpl_prepare_inputs_ex  mpl_prepare_inputs for a calibration with k, p (lib/dataset/joints_dataset_mpl.py:269, :337)
 *   mpl_synthesize_views_ex  mpl_synthesize_views with the projection of lib/multiviews/cameras.py:22-46
 */
#ifndef MPL_HIP_H_
#define MPL_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPL_HIP_ABI_VERSION 14
#define MPL_MAX_VIEWS 32
#define MPL_MAX_APPS 64 /* max Block applications in one stack schedule */

/* error codes */
#define MPL_OK 0
#define MPL_E_INVALID (-1)     /* bad argument / shape */
#define MPL_E_UNSUPPORTED (-2) /* flag combination or size not implemented in HIP */
#define MPL_E_WORKSPACE (-3)   /* workspace too small */
#define MPL_E_LAUNCH (-4)      /* hip runtime reported an error at launch */
#define MPL_E_DEVICE (-5)      /* a kernel of an EARLIER call on this device reported a failure (see mpl_device_error) */

/* flag bits of mpl_config.flags == constructor kwargs of MultiView_MPL (multiview_mpl.py:98-117) */
#define MPL_F_MULTI_SPT (1u << 0)       /* multiple_spatial_blocks */
#define MPL_F_CONF_ADD (1u << 1)        /* add_confidence_input */
#define MPL_F_CONF_MULT (1u << 2)       /* mult_confidence_emb */
#define MPL_F_CONF_ATTN_W (1u << 3)     /* confidence_as_attention_uncertainty_weight */
#define MPL_F_POS3D_LEARN (1u << 4)     /* pose_3d_emb_learnable */
#define MPL_F_POS3D_SPATIAL (1u << 5)   /* add_3D_pos_encoding_in_Spatial */
#define MPL_F_RAYS_TOKEN (1u << 6)      /* input_rays_as_token */
#define MPL_F_POS3D_TO_RAYS (1u << 7)   /* add_3D_pos_encoding_to_rays */
#define MPL_F_NO_SPT (1u << 8)          /* no_transformer_spt */
#define MPL_F_NO_FPT (1u << 9)          /* no_transformer_fpt */
#define MPL_F_CONF_IN_FPT (1u << 10)    /* confidence_in_FPT */
#define MPL_F_KPTOK (1u << 11)          /* FPT_blocks_view_keypoint_tokens: FPT blocks of width d over 17*V tokens */
/* not a constructor kwarg: engine selection of the FPT block stack.  Stacks of up to 80 token rows (a single frame, a few
 * persons; groups of sequences of at most 16 rows, as many as the compute units hold) normally run the small-batch engine (csrc/sm_stack.hip: exact fp32 MFMA, the whole chip per GEMM), larger ones the
 * team kernels (fp16x2 operands): two fp32 engines that agree to ~1e-7 but not bit for bit.  With this flag the team kernels
 * run for EVERY batch size, so that a pose carries the same bits whatever batch or shard it arrives in. */
#define MPL_F_NO_SMALL_STACK (1u << 12)
/* not a constructor kwarg: run the SPT stage on the shape-general kernel (csrc/spt_any.hip: any J / d / H, fp32 FMA on the
 * nn.Linear tensors) also at J = 17, d = 32, H = 8, where the tuned kernels normally run.  Every other shape takes it anyway. */
#define MPL_F_GENERIC_SPT (1u << 13)

/* epilogues of mpl_ln_linear */
#define MPL_EPI_BIAS 0          /* y = a W^T + b                       (attn.qkv) */
#define MPL_EPI_BIAS_GELU 1     /* y = gelu_erf(a W^T + b)             (mlp.fc1 + nn.GELU) */
#define MPL_EPI_BIAS_RESIDUAL 2 /* y = r + a W^T + b                   (attn.proj / mlp.fc2 + residual) */

/* Parameters of one Block (multiview_mpl.py:70-92), device pointers, reference layouts:
 * norm{1,2}.{weight,bias} (D); attn.qkv (3D,D),(3D); attn.proj (D,D),(D);
 * mlp.fc1 (2D,D),(2D); mlp.fc2 (D,2D),(D). */
typedef struct mpl_block_weights {
    const float *ln1_w, *ln1_b;
    const float *qkv_w, *qkv_b;
    const float *proj_w, *proj_b;
    const float *ln2_w, *ln2_b;
    const float *fc1_w, *fc1_b;
    const float *fc2_w, *fc2_b;
    /* Optional packed bf16 operands (mpl_pack_bf16) of the four Linear layers: qkv built with norm1 folded, fc1 with norm2
     * folded, proj / fc2 plain.  When all four are non-NULL in every block of a stack whose shape the engine supports (D 544
     * or 1088, n_tok <= 32), the stack's GEMMs run on the bf16 matrix cores with bf16 operands and fp32
     * accumulation (activations handed from GEMM to GEMM as bf16; LayerNorm statistics, softmax, GELU, the residual
     * stream and the output stay fp32) -- BASELINE.json configs[2] "bf16".  The fp32 tensors remain the source of truth.
     * For every other stack shape of up to 32 tokens per sequence (any width up to 4096, any head count that divides it) the
     * same four fields carry the shape-general operands of mpl_pack_bf16_any instead, and the stack runs one plain launch per
     * GEMM (csrc/b1_any.hip, same rounding points).  mpl_bf16_operand_layout(dim, heads, n_tok) says which of the two layouts a
     * stack expects: the library launches by it, whoever packs must pack by it. */
    const uint16_t *qkv_w16, *proj_w16, *fc1_w16, *fc2_w16;
    /* qkv_w3: the row-local split operand of a d = 32 block (mpl_spt_pack for the SPT blocks of an mpl_spt_set, mpl_d32_pack for
     * the keypoint-token FPT blocks); proj_w3 / fc1_w3 / fc2_w3 are unused and must be NULL (they carried the three-part bf16
     * operands of the round-2 fp32 engine, removed in round 5). */
    const uint16_t *qkv_w3, *proj_w3, *fc1_w3, *fc2_w3;
    /* Optional fp16x2 operands (mpl_pack_h2) of the four Linear layers, same folding as above: the DEFAULT fp32 engine of the
     * FPT block stack (csrc/h2_gemm.hip).  Every fp32 operand is split in two fp16 parts under an exact power-of-two scale
     * (per weight column; static per activation column, from a data-free bound), each product is accumulated in fp32
     * from three partial products ("3xTF32" on the fp16 matrix cores): as accurate as an fp32 GEMM, half the matrix
     * instructions of the round-2 three-part engine.  Used when all four are non-NULL (and the *_w16 are NULL) in every block; shapes must satisfy mpl_pack_h2_bytes() != 0.  qkv_h2 / fc1_h2 come from mpl_pack_h2 (norm1 /
     * norm2 folded); proj_h2 / fc2_h2 from mpl_pack_h2_scaled against the static output scales of the layer that produces their
     * input: in_scale = mpl_pack_h2_out_scale(qkv_h2, 3D, D) + 2D (the v columns) for proj, mpl_pack_h2_out_scale(fc1_h2, 2D, D)
     * for fc2.  The stack verifies that pairing on the device (fingerprints inside the operands) and poisons the call's output
     * (NaN poses, MPL_E_DEVICE) on a mismatch.  The team kernels take widths 544 and 1088 (no LayerNorm folds into an operand beyond
     * K = 1088) with a head dim that divides 136 and is a multiple of 4, while the score matrices of a slice fit the LDS beside
     * the q | k | v tile (head dim 8: up to 14 tokens per sequence, head dim 4: up to 6); for every other stack the four fields
     * are ignored and the nn.Linear tensors above run (mpl_block_stack_form: MPL_FORM_UNPACKED). */
    const uint16_t *qkv_h2, *proj_h2, *fc1_h2, *fc2_h2;
} mpl_block_weights;

/* Per-view (or shared) spatial parameter set, multiview_mpl.py:159-195, :236-249. */
typedef struct mpl_spt_set {
    const float *embed_w, *embed_b;  /* Spatial_patch_to_embedding[.v]  (d,in_chans),(d) */
    const float *conf_w, *conf_b;    /* confidence_to_embedding[.v]     (d,1),(d) or NULL */
    const float *pos_embed;          /* Spatial_pos_embed[.v]           (J,d) */
    const mpl_block_weights *blocks; /* DEVICE array [depth]            Spatial_blocks[.v] */
} mpl_spt_set;

typedef struct mpl_config {
    int32_t num_joints; /* NETWORK.NUM_JOINTS (17) */
    int32_t dim;        /* NETWORK.DIM = embed_dim_ratio (32) */
    int32_t depth;      /* NETWORK.TRANSFORMER_DEPTH */
    int32_t heads;      /* NETWORK.TRANSFORMER_HEADS */
    int32_t num_views;  /* V, a constructor constant (multiview_mpl.py:534-546) */
    int32_t in_chans;   /* 2, or 3 with confidence_input_as_third (:159-168) */
    uint32_t flags;     /* MPL_F_* */
    int32_t reserved;
} mpl_config;

typedef struct mpl_weights {
    const mpl_spt_set *spt_sets;       /* DEVICE array: [V] if MPL_F_MULTI_SPT else [1] */
    const float *spatial_norm_w, *spatial_norm_b;          /* Spatial_norm (d) */
    const float *pos_3d_embed;                             /* (J, d|2d) */
    const float *pos_3d_view_coding;                       /* (J, d|2d) */
    const float *pos_3d_linear_w, *pos_3d_linear_b;        /* (d|2d,3),(d|2d) */
    const float *ray_embed_w, *ray_embed_b;                /* ray_to_embedding (d,3),(d) or NULL */
    const float *conf_fpt_w, *conf_fpt_b;                  /* confidence_to_embedding_FPT (d,1),(d) or NULL */
    const mpl_block_weights *fpt_blocks;                   /* HOST array [depth]: blocks.{l} */
    const float *view_norm_w, *view_norm_b;                /* View_norm (J*d) */
    const float *wmean_w, *wmean_b;                        /* weighted_mean Conv1d (1,V,1),(1) */
    const float *head_ln_w, *head_ln_b;                    /* head.0 (J*d) */
    const float *head_w, *head_b;                          /* head.1 (3J, J*d),(3J) */
    uint32_t spt_packed;  /* != 0: EVERY block of every spt_set carries the operand of mpl_spt_pack in its qkv_w3 field: the
                           * SPT Linear layers run as fp32 arithmetic on the fp16 matrix cores (spt3_kernel); 0: the fp32
                           * matrix instructions read the nn.Linear weights in place */
    uint32_t reserved;
} mpl_weights;

typedef struct mpl_inputs {
    int32_t batch;
    int32_t reserved;
    const float *poses[MPL_MAX_VIEWS];   /* V x (B,J,3) contiguous: x_norm, y_norm, conf (function_mpl.py:350) */
    const float *rays[MPL_MAX_VIEWS];    /* V x (B,J,3) or NULL when unused by the flags */
    const float *centers[MPL_MAX_VIEWS]; /* V x (B,1,3) or NULL */
} mpl_inputs;

int mpl_hip_abi_version(void);
const char *mpl_hip_error_string(int code);

/* The supported envelope, decided here and nowhere else: MPL_OK or MPL_E_UNSUPPORTED (MPL_E_INVALID for a NULL cfg).
 * mpl_forward and mpl_spt_tokens refuse anything outside it before they launch.
 *   1 <= num_joints <= 64;  1 <= dim <= 128;  heads >= 1 with dim % heads == 0 (the reference fails in the qkv reshape otherwise);
 *   FPT width J*d (x2 with MPL_F_RAYS_TOKEN) <= 4096;  1 <= num_views <= MPL_MAX_VIEWS;  depth 0..60 (0..31 with
 *   MPL_F_CONF_ATTN_W: every SPT block then runs twice);
 *   MPL_F_POS3D_TO_RAYS only with MPL_F_RAYS_TOKEN and not with MPL_F_POS3D_SPATIAL (the reference fails, :483);
 *   MPL_F_KPTOK (FPT blocks over J*V tokens of width d): not with MPL_F_RAYS_TOKEN; up to 32 tokens any head dim; more tokens
 *   need head dim 4 or 8 with J*V*hd*8 <= 64 KiB (K / V of one head resident in LDS), or a head dim that is a multiple of 16 up to
 *   128 with J*V <= 2048 (K / V streamed through LDS, token_attention_wide.hip).  Any other head dim beyond 32 tokens is refused. */
int mpl_config_supported(const mpl_config *cfg);

/* FPT token width D_f = J*d (x2 with MPL_F_RAYS_TOKEN), multiview_mpl.py:140-142. */
int mpl_fpt_width(const mpl_config *cfg);

/* Bytes of scratch mpl_forward needs for `batch` poses (activations only; 256-B aligned). */
size_t mpl_forward_workspace_bytes(const mpl_config *cfg, int batch);

/* Whole forward: V x (B,J,3) keypoints -> out (B,J,3).  MultiView_MPL.forward :450-525. */
int mpl_forward(const mpl_config *cfg, const mpl_weights *w, const mpl_inputs *in, float *out,
                void *workspace, size_t workspace_bytes, void *stream);

/* Stage 1: embedding + SPT stack + Spatial_norm + per-view glue -> xs (B*V, D_f) row-major,
 * row = b*V + v.  Spatial_forward_features :349-414 and forward :458-499. */
int mpl_spt_tokens(const mpl_config *cfg, const mpl_weights *w, const mpl_inputs *in, float *xs, void *stream);

/* Stage 2: a stack of Blocks applied in place on x (n_seq*n_tok, D).  `schedule[i]` = layer
 * index of the i-th application (the reference applies the last layer twice, :420-423).
 * `blocks` is a HOST array.  Workspace: mpl_block_stack_workspace_bytes(). */
size_t mpl_block_stack_workspace_bytes(int n_seq, int n_tok, int dim);
int mpl_block_stack(float *x, int n_seq, int n_tok, int dim, int heads, const mpl_block_weights *blocks,
                    const uint8_t *schedule, int n_apps, void *workspace, size_t workspace_bytes, void *stream);
/* the same with engine flags (MPL_F_NO_SMALL_STACK; 0 = mpl_block_stack) */
int mpl_block_stack_ex(float *x, int n_seq, int n_tok, int dim, int heads, const mpl_block_weights *blocks,
                       const uint8_t *schedule, int n_apps, void *workspace, size_t workspace_bytes, unsigned flags, void *stream);

/* y[M,N] = epilogue( LN(x)[M,K] . W[N,K]^T + bias ); ln_w == NULL skips the LayerNorm.
 * `stats` is scratch for 2*M*max(1, K/136) floats (per-slice LayerNorm partials) when ln_w != NULL.
 * residual may alias y. */
int mpl_ln_linear(const float *x, int M, int K, const float *ln_w, const float *ln_b, float eps, const float *W,
                  const float *bias, int N, int epilogue, const float *residual, float *y, float *stats,
                  void *stream);

/* Split operand of ONE SPT block (d = 32: qkv 96x32, proj 32x32, fc1 64x32, fc2 32x64): the four weights as two fp16 parts
 * each (hi | lo, MFMA fragment order) under one exact power-of-two scale per output column, with norm1 / norm2 folded into
 * the qkv / fc1 weights; behind them the epilogue vectors c_n (bias + folded LayerNorm offset), the multipliers sc_n and the
 * static scales of the proj / fc2 inputs (the arithmetic of mpl_pack_h2).  mpl_spt_pack_bytes() = 48 KiB (34.6 KiB used).
 * `block` is a HOST struct whose pointers are device addresses -- EVERY weight, bias and LayerNorm vector of the block must
 * be set; the result goes into the qkv_w3 field of the block's entry in the DEVICE array of mpl_spt_set and is derived data:
 * repack when any tensor of the block changes. */
size_t mpl_spt_pack_bytes(void);
int mpl_spt_pack(const mpl_block_weights *block, uint16_t *dst, void *stream);
/* The same operand for a D = 32 FPT block (keypoint-token variant, multiview_mpl.py:261-266): identical layout, the q columns
 * NOT pre-scaled (the token attention kernel scales q itself).  A block whose qkv_w3 field carries it (proj_w3 / fc1_w3 /
 * fc2_w3 NULL) runs in mpl_block_stack as d32_qkv_kernel -> token attention -> d32_mlp_kernel: two row-local launches per
 * block application instead of four GEMMs and two LayerNorm-statistics passes. */
int mpl_d32_pack(const mpl_block_weights *block, uint16_t *dst, void *stream);

/* Packed bf16 operand of an nn.Linear layer (W[N][K], bias[N]) for the bf16 engine (csrc/b1_gemm.hip): ONE bf16 per weight
 * (round to nearest even of gamma o W) in MFMA fragment order, two 32-deep k-tiles per 2-KiB fragment slot (an odd k-tile count
 * is padded with a zero k-tile), followed by fp32 vectors of N entries: with ln_w / ln_b != NULL the LayerNorm in front of the
 * layer is folded in, LN(x).W^T + b = rstd (x16.(gamma o W)^T - mean s) + c with s_n = sum_k of the ROUNDED gamma_k W_nk and
 * c_n = b_n + sum_k beta_k W_nk (else c = bias, s = 0).  mpl_pack_bf16_bytes() is the size of `dst` in bytes, or 0 when the
 * shape is not supported (N must be a multiple of 136, K of 544). */
size_t mpl_pack_bf16_bytes(int N, int K);
int mpl_pack_bf16(const float *W, const float *bias, const float *ln_w, const float *ln_b, int N, int K, uint16_t *dst,
                  void *stream);

/* Which packed bf16 operands the *_w16 fields of a block stack of this shape carry -- ONE rule, by which mpl_block_stack launches and
 * a binding packs: MPL_BF16_TUNED = mpl_pack_bf16 (the team kernels take the shape: dim 544 or 1088, a head that tiles a
 * 136-column slice, n_tok <= 32); MPL_BF16_ANY = mpl_pack_bf16_any (every other dim <= 4096 with dim % heads == 0 and n_tok <= 32);
 * MPL_BF16_NONE = the shape has no bf16 engine (more than 32 tokens per sequence: the joints x views token grid).  No device needed. */
enum { MPL_BF16_NONE = 0, MPL_BF16_TUNED = 1, MPL_BF16_ANY = 2 };
int mpl_bf16_operand_layout(int dim, int heads, int n_tok);
/* 1 when the packed-operand team kernels (fp16x2: csrc/h2_gemm.hip, bf16: csrc/b1_gemm.hip) take a stack of this shape, 0 when not,
 * MPL_E_INVALID for a non-positive argument -- the ONE rule behind mpl_block_stack(_ex), mpl_block_stack_form(_ex) and
 * mpl_bf16_operand_layout: width 544 or 1088, a head dim that divides 136 and is a multiple of 4, and the score matrices of a slice
 * in LDS beside the q | k | v tile (n_tok <= 32; head dim 8: <= 14, head dim 4: <= 6).  Whoever packs fp16x2 operands asks it first
 * (mpl_pack_h2 folds no LayerNorm into an operand beyond K = 1088).  No device needed. */
int mpl_team_stack_shape(int dim, int heads, int n_tok);

/* Packed bf16 operand of an nn.Linear layer (W[N][K], bias[N]) for the shape-general bf16 engine (csrc/b1_any.hip), any
 * 1 <= N <= 16384, 1 <= K <= 8192: bf16(gamma o W) (round to nearest even of the fp32 product; gamma = 1 without a LayerNorm) as
 * [ceil(N/64)][ceil(K/32)][4 column tiles][64 lanes][8 bf16] -- lane l, element j of column tile t of block (nb, kt) is
 * W[64 nb + 16 t + (l & 15)][32 kt + 8 (l >> 4) + j], ZERO where that is beyond N or K -- followed by the fp32 vectors
 * c[N] = bias + W . beta and s[N] = sum_k of the ROUNDED gamma_k W_nk (c = bias, s = 0 without a LayerNorm), padded to 16 bytes.
 * ln_w and ln_b come together or not at all.  mpl_pack_bf16_any_bytes() = size of `dst`, 0 outside the limits above.  `dst` must be
 * 16-byte aligned (it is written and read as 16-byte fragments; MPL_E_INVALID otherwise). */
size_t mpl_pack_bf16_any_bytes(int N, int K);
int mpl_pack_bf16_any(const float *W, const float *bias, const float *ln_w, const float *ln_b, int N, int K, uint16_t *dst,
                      void *stream);
/* ONE GEMM of that engine, the unit-test entry (the forward reaches the kernel through mpl_block_stack):
 *   has_ln != 0: y = epi(rstd (bf16(x) . W16^T - mean s) + c) on the raw fp32 rows x[M][K]; stats = 2 * M * max(1, K / 136) floats of
 *     scratch; epilogue MPL_EPI_BIAS -> y fp32 [M][N], MPL_EPI_BIAS_GELU -> y bf16 (uint16_t) [M][N] = bf16(gelu_erf(.));
 *   has_ln == 0: y = residual + bf16(x) . W16^T + c, epilogue MPL_EPI_BIAS_RESIDUAL only (residual may alias y); x is rounded to
 *     bf16 rows in `workspace` (mpl_ln_linear_bf16_any_workspace_bytes(M, K), 16-byte aligned) first.
 * Other combinations are MPL_E_UNSUPPORTED: a Block has no other. */
size_t mpl_ln_linear_bf16_any_workspace_bytes(int M, int K);
int mpl_ln_linear_bf16_any(const float *x, int M, int K, int has_ln, float eps, const uint16_t *W16, int N, int epilogue,
                           const float *residual, void *y, float *stats, void *workspace, size_t workspace_bytes, void *stream);

/* Diagnostics (tools/chain_phase.py): when non-NULL, every packed-operand GEMM launch writes five shader-clock stamps per
 * wave (entry, k-loop start, k-loop end, stores issued, stores drained) at device_buffer[(block * 8 + wave) * 8 ..];
 * the buffer must hold 64 bytes per wave of the largest launch.  NULL (the default) switches it off.  The stamps are
 * compiled only into a library built with -DH2_DBG=1 (MPL_HIPCC_FLAGS); in the product build the call is a no-op. */
int mpl_x3_debug_buffer(void *device_buffer);
/* Diagnostics / A-B: bit 0: 0 (default) = a block stack on packed operands is ONE persistent launch (row-tile chains of
 * workgroups, h2_stack_kernel); 1 = one launch per GEMM (results agree to <= 4 ulp, each mode is bitwise
 * deterministic).  Bits 1-2: 0 = the stack picks its stage by the shape of the launch (fp16x2: teams that own two or more row
 * tiles walk PAIRS of tiles, h2_stack2_kernel; bf16: always one tile at a time), 1 / 2 = force the one- / two-tile stage
 * (fp16x2 only; bitwise the same poses).  Bit 3: no
 * small-batch engine (sm_stack.hip: stacks of up to 80 token rows run every GEMM on the whole chip, the activations handed
 * over as {value, tag} pairs, exact fp32 MFMA on the nn.Linear tensors in place; two fp32 engines, <= 1e-6 apart).  Bit 4: the 16-row teams in
 * the ring form (h2_stackn_kernel) instead of the direct-W form (h2_stackd_kernel).  Bits 5-6: row-narrow teams: 0 = by the
 * shape of the launch, 1 = never, 2 / 3 = 32- / 16-row workgroups wherever legal.  Bit 7: write-through hand-off stores also
 * for teams that sit on one XCD.  Every one of these forms yields bitwise the same poses.  Bits 8.. = stop after that many
 * GEMM phases (tools/chain_phase.py). */
int mpl_x3_stack_mode(int one_launch_per_gemm);

/* Which kernel form mpl_block_stack(_ex) takes for a stack of this shape on the current device, by the library's own rule
 * (csrc/h2_phase.hpp h2_stack_form, csrc/api.hip block_stack_impl): for benchmarks that name the kernel they time and tests that
 * pin the rule.  operand_parts: 2 = the blocks carry mpl_pack_h2 operands, 1 = bf16 operands in their *_w16 fields (in the layout
 * mpl_bf16_operand_layout names for the shape), 0 = neither; `flags` as
 * mpl_config.flags (MPL_F_NO_SMALL_STACK).  The small-batch engine additionally needs the nn.Linear tensors of the blocks
 * (the query assumes they are there).  Negative = MPL_E_*.  Every team form yields bitwise the same poses. */
enum {
    MPL_FORM_UNPACKED = 0,        /* no packed operands: one launch per GEMM on the fp32-MFMA engine (ln_gemm.hip / the D = 32 path) */
    MPL_FORM_SMALL = 1,           /* sm_stack_kernel: up to 80 token rows, every GEMM on the whole chip */
    MPL_FORM_TEAMS = 2,           /* h2_stack_kernel<NP>: one 64-row tile per team step */
    MPL_FORM_PAIRS = 3,           /* h2_stack2_kernel<2>: pairs of row tiles (fp16x2 operands only) */
    MPL_FORM_ROWS32 = 4,          /* h2_stackn_kernel<2>: 32-row teams */
    MPL_FORM_ROWS16 = 5,          /* h2_stackn_kernel<2>: 16-row teams, ring form (A/B, or A operand too large for LDS) */
    MPL_FORM_ROWS16_DIRECT = 6,   /* h2_stackd_kernel<2>: 16-row teams, direct-W form */
    MPL_FORM_PER_GEMM = 7,        /* h2_gemm_kernel: one launch per GEMM (mpl_x3_stack_mode bit 0) */
    MPL_FORM_BF16_ANY = 8         /* b1a_gemm_kernel: bf16 operands of mpl_pack_bf16_any, one launch per GEMM (any width) */
};
int mpl_block_stack_form(int n_seq, int n_tok, int D, int heads, int n_apps, int operand_parts, unsigned flags);
/* The same question with everything the launch rule looks at: n_blocks = distinct blocks the schedule indexes (mpl_block_stack_form
 * assumes the reference's schedule: n_apps - 1), raw_tensors != 0 = every nn.Linear / LayerNorm tensor of those blocks is present
 * (the small-batch engine reads them in place; a caller that hands over packed operands only gets the team kernels).  Both queries
 * and mpl_block_stack(_ex) itself go through ONE predicate (csrc/api.hip small_engine_taken + h2_phase.hpp h2_stack_form). */
int mpl_block_stack_form_ex(int n_seq, int n_tok, int D, int heads, int n_apps, int n_blocks, int raw_tensors, int operand_parts,
                            unsigned flags);
/* MPL_FORM_* of the calling thread's most recent successful mpl_block_stack(_ex) / mpl_forward: the form that was LAUNCHED (incl.
 * the fall-through when the small-batch engine's occupancy query refuses); negative before the first one. */
int mpl_block_stack_last_form(void);

/* Which kernel the SPT stage (mpl_spt_tokens, mpl_forward) launches for `batch` poses and how many sequences (one pose in one
 * view) share a workgroup, by the library's own rule (csrc/spt.hip spt_form: both launchers follow it).  The smallest c with
 * num_views * ceil(batch / c) <= compute units, at most 16 (tuned kernels, J 17 / d 32 / H 8) or what fits 64 KiB of LDS
 * (shape-general kernel).  use_packed != 0: the SPT blocks carry mpl_spt_pack operands (mpl_weights.spt_packed). */
enum {
    MPL_SPT_STAGED = 0,           /* spt_kernel<true>: fp32 MFMA, weights staged in LDS, up to 8 sequences per workgroup */
    MPL_SPT_FRAGS = 1,            /* spt_kernel<false>: weight fragments in registers, 9 .. 16 sequences per workgroup */
    MPL_SPT_PACKED = 2,           /* spt3_kernel<SS>: split operands, SS = 1, 2, 4, 8 or 16 sequences per workgroup */
    MPL_SPT_ANY = 3               /* spt_any_kernel: every other shape, and 17 / 32 / 8 with MPL_F_GENERIC_SPT */
};
/* kernel the SPT launch for `batch` poses takes and its sequences per workgroup (*seq_per_wg; SS for MPL_SPT_PACKED);
 * n_cus <= 0: ask the current device.  Launches nothing.  Negative = MPL_E_*. */
int mpl_spt_form(const mpl_config *cfg, int batch, int use_packed, int n_cus, int *seq_per_wg);

/* softmax(q k^T * hd^-0.5) v per (sequence, head) on a packed qkv (n_seq*n_tok, 3*dim). Attention :55-64.
 * n_tok <= 32: any head dim.  Beyond: head dim 4 or 8 with n_tok*hd*8 <= 64 KiB, or a multiple of 16 up to 128 with n_tok <= 2048;
 * anything else answers MPL_E_UNSUPPORTED and launches nothing. */
int mpl_token_attention(const float *qkv, int n_seq, int n_tok, int dim, int heads, float *out, void *stream);

/* Stage 3: strip ray features, View_norm, Conv1d weighted mean over views, head LN + Linear.
 * x (B*V, D_f) -> out (B, 3J).  forward_features :425-446, head :521-523.  Any E = J*d up to 4096 (J*d <= 544 and
 * 3J * J*d <= 28 K: the fused LDS form; beyond it a shape-general kernel, one workgroup per pose). */
int mpl_fuse_head(const mpl_config *cfg, const mpl_weights *w, const float *x, int batch, float *out, void *stream);

/* ---- output-side variants (constructor flags linear_weighted_mean, deep_head, head_kadkhod; :277-317, :506-519).
 * The default tail stays fused in mpl_fuse_head / mpl_forward; these building blocks let the binding compose the
 * other tails exactly as the reference does. */

/* strip ray features + View_norm + Conv1d weighted mean (:425-446) WITHOUT the head: x (B*V, D_f) -> y (B, J*d). */
int mpl_view_fuse(const mpl_config *cfg, const mpl_weights *w, const float *x, int batch, float *y, void *stream);

/* strip ray features + View_norm only (:425-439): x (B*V, D_f) -> xn (B, V*J*d), the input of the
 * linear_weighted_mean Linear (:441-443). */
int mpl_view_norm(const mpl_config *cfg, const mpl_weights *w, const float *x, int batch, float *xn, void *stream);

/* y[M,K] = LayerNorm(x[M,K]) (head[0] of every head variant, eps 1e-5). */
int mpl_layernorm(const float *x, int M, int K, const float *gamma, const float *beta, float eps, float *y,
                  void *stream);

/* y[M,N] = act( bn( [xa | xb] . W^T + bias ) ): nn.Linear on the concatenation of xa (M,Ka) and xb (M,Kb; may be
 * NULL/0) -- torch.cat([x_prev, x], dim=1) of head_kadkhod :511-513 without materialising it -- followed by an
 * optional BatchNorm1d in eval mode (running statistics, bn_w == NULL skips it) and an optional ReLU.
 * W is (N, Ka+Kb) row-major. */
int mpl_linear(const float *xa, int Ka, const float *xb, int Kb, int M, const float *W, const float *bias, int N,
               const float *bn_w, const float *bn_b, const float *bn_mean, const float *bn_var, float bn_eps, int relu,
               float *y, void *stream);

/* ---- input preparation (the step right before the path): raw per-view detections ->
 * the tensors mpl_forward consumes.  Replaces, per sample and view, normalize_screen_coordinates
 * (joints_dataset_mpl.py:817-820), the camera normalisation of __getitem__ (:615-623), create_3d_ray_coords (:872-904),
 * cam_center (:646) and the [x, y, conf] concat (:772).
 *   joints_px (B,V,J,2) pixel coordinates, conf (B,V,J) or NULL (-> 1), device;
 *   cams_dev device (V,16) float64: fx fy cx cy | R row-major (world->camera) | t (camera centre in world coords);
 *   img_w/img_h = NETWORK.IMAGE_SIZE; normalize_inputs = DATASET.INPUTS_NORMALIZED, normalize_cameras =
 *   DATASET.NORMALIZE_CAMERAS;  poses/rays/centers: host arrays of V device pointers to (B,J,3),(B,J,3),(B,1,3).
 * MPL_E_INVALID: joints_px or cams_dev NULL, a non-positive size or image size, views > MPL_MAX_VIEWS, a NULL table or entry;
 * MPL_E_UNSUPPORTED: batch * views * joints > 2^30 -- before any launch. */
int mpl_prepare_inputs(const float *joints_px, const float *conf, const double *cams_dev, int batch, int views,
                       int joints, float img_w, float img_h, int normalize_inputs, int normalize_cameras,
                       float *const *poses, float *const *rays, float *const *centers, void *stream);

/* ---- detector heatmaps -> pixel detections (-> model inputs), csrc/heatmaps.hip: the step in front of mpl_prepare_inputs, in
 * place of lib/core/inference.py:22-81 (get_max_preds on an np.ndarray, then get_final_preds: a Python double loop over (sample,
 * joint) and one cv2.getAffineTransform per sample, lib/utils/transforms.py:51-94), which would pull every heatmap to the host.
 * One launch; per heatmap (b, v, j), in this order:
 * a. peak (:34-49): idx = the first index of the maximum of the H*W values in row-major order, maxval = that value; NaN counts as
 * the maximum and the first NaN wins (np.argmax / np.amax); -0.0 and 0.0 tie.  x = idx % W, y = idx / W, both times (maxval > 0):
 * a map with no positive value gives (0, 0) and keeps its non-positive or NaN maxval.
 * b. post_process != 0 (TEST.POST_PROCESS, :63-72): where 1 < x < W-1 and 1 < y < H-1 (the reference's own strict bounds),
 * x += 0.25 * sign(hm[y][x+1] - hm[y][x-1]), y += 0.25 * sign(hm[y+1][x] - hm[y-1][x]); the sign is taken by comparison (exact
 * for every dtype), a NaN neighbour gives a NaN coordinate.  -> coords, in heatmap cells.
 * c. back to the image (transform_preds with rot = 0): k = scale[b,v,0] * 200 / W, pixel = center[b,v] + (coord - (W/2, H/2)) * k,
 * isotropic, scale[b,v,1] is not read (as in the reference); fp64 on the fp32 inputs, rounded once.  Without center / scale
 * pixels = coords.  The one deviation: the reference rounds the three anchor points of its affine fit to float32 before it
 * solves, the closed form does not (on the committed golden at most 3 fp32 ulps, and 20 at one pixel that is the small difference of
 * two large terms, where the rounded anchors are the ones in error).
 * d. pixels (B,V,J,2) and conf (B,V,J) = maxval are the joints_px / conf of mpl_prepare_inputs.  With cams_dev the same thread goes
 * on with the arithmetic of mpl_prepare_inputs on the fp32-rounded pixel and writes poses / rays / centers: bitwise what
 * mpl_prepare_inputs writes from pixels and conf.
 * heatmaps: HOST array of `views` device pointers; view v holds (B,J,H,W) values of `dtype` (MPL_HM_*), sample b starting at
 * element b * batch_stride: batch_stride = J*H*W for V separate tensors, V*J*H*W with heatmaps[v] = base + v*J*H*W for one
 * contiguous (B,V,J,H,W) tensor -- both are read in place.  16-bit values are widened exactly: decoding a 16-bit map equals
 * decoding its fp32 upcast bit for bit.  center, scale: device fp32 (B,V,2), both or neither.  coords: (B,V,J,2) or NULL.
 * cams_dev / img_w / img_h / normalize_* / poses / rays / centers: as for mpl_prepare_inputs; cams_dev NULL = no model inputs (the
 * tables are then not read).
 * A map whose base address and byte size are multiples of 16 is read with 16-byte loads, any other element by element; a map of
 * 64 KiB or more is shared by the four waves of a workgroup, a smaller one read by one wave.  The merge is a total order (NaN,
 * then value, then lower index), so all of these give identical outputs, run to run and batching to batching.
 * MPL_E_INVALID: heatmaps, one of its first `views` entries, pixels or conf NULL; a non-positive size; center without scale or the
 * reverse; cams_dev without all three tables, with a NULL entry in one, or with img_w / img_h <= 0; an unknown dtype;
 * batch_stride < J*H*W.  MPL_E_UNSUPPORTED: views > MPL_MAX_VIEWS, H*W > 2^20, batch*views*joints > 2^30.  All before any launch.
 * Stream-ordered, never synchronises; like the geometry calls it neither looks at nor sets the device error word. */
#define MPL_HM_F32 0
#define MPL_HM_F16 1
#define MPL_HM_BF16 2
int mpl_decode_heatmaps(const void *const *heatmaps, int dtype, long long batch_stride, int batch, int views, int joints,
                        int height, int width, int post_process, const float *center, const float *scale, float *pixels,
                        float *conf, float *coords, const double *cams_dev, float img_w, float img_h, int normalize_inputs,
                        int normalize_cameras, float *const *poses, float *const *rays, float *const *centers, void *stream);

/* Sub-pixel decoding: mpl_decode_heatmaps with step b replaced by a refinement of the integer peak (x0, y0).  `refine`:
 * MPL_REFINE_NONE is mpl_decode_heatmaps itself, same kernels and same bits (radius and threshold are not looked at);
 * MPL_REFINE_GAUSSIAN and MPL_REFINE_CENTROID exclude post_process.  A refinement applies only where 0 < maxval < inf; elsewhere
 * the coordinates are those of the plain decode ((0,0) for a non-positive or NaN peak, the integer peak for +inf).  The offset d
 * is fp64 on the exactly widened values, and x0 + d is rounded to fp32 once -> coords; steps c and d follow on that coordinate.
 * MPL_REFINE_GAUSSIAN: per axis the three values f-, f0, f+ on the peak's row (x) or column (y): a = ln f0 - ln f+,
 * b = ln f0 - ln f-, d = (b - a) / (2 (a + b)), exact for a Gaussian of any sigma and within +/-0.5 because f0 is the maximum.
 * d = 0 on an axis whose peak coordinate is 0 or the last one, where a neighbour is not positive and finite, or where a + b == 0.
 * MPL_REFINE_CENTROID: what find_tensor_peak_batch (lib/core/inference.py:84-134) means to compute.  Over the window
 * (x0 + i, y0 + j), |i|, |j| <= radius (1..8): w = the value where it is above `threshold` and inside the map, else 0
 * (F.threshold, padding_mode='zeros'); S = sum w + 2.22e-16; d = (sum w i / S, sum w j / S).  Deviations from the reference's
 * lines: the row is idx / W in integers (the reference divides truly), and the samples sit on the integer cells, the
 * align_corners=True reading of its normalize(), so an integer radius needs no interpolation; pix2coord is not applied, step c is
 * the way back to pixels.  The window is spread over the 64 lanes of the finishing wave and summed in a fixed order: the one-wave
 * and the four-wave form, every layout and every run give the same bits.
 * MPL_E_INVALID, besides those of mpl_decode_heatmaps: refine outside 0..2; a refinement together with post_process; with
 * MPL_REFINE_CENTROID a radius outside 1..8 or a NaN threshold.  All before any launch. */
#define MPL_REFINE_NONE 0
#define MPL_REFINE_GAUSSIAN 1
#define MPL_REFINE_CENTROID 2
int mpl_decode_heatmaps_ex(const void *const *heatmaps, int dtype, long long batch_stride, int batch, int views, int joints,
                           int height, int width, int post_process, const float *center, const float *scale, float *pixels,
                           float *conf, float *coords, const double *cams_dev, float img_w, float img_h, int normalize_inputs,
                           int normalize_cameras, float *const *poses, float *const *rays, float *const *centers, int refine,
                           int radius, double threshold, void *stream);

/* ---- heatmaps rendered from 2D joints, csrc/heatmap_render.hip: the producer in front of mpl_decode_heatmaps and mpl_rpsm, in
 * place of generate_heatmap (lib/dataset/joints_dataset_mpl.py:828-870, numpy, one joint at a time).  One launch, one wave per map.
 * The cell m of joint (b,v,j), fp64 on the fp32 inputs: with center / scale (device fp32 (B,V,2), both or neither)
 * m = (pixel - center[b,v]) / k + (W/2, H/2), k = scale[b,v,0] * 200 / W, the exact inverse of mpl_decode_heatmaps step c; with
 * stride_x, stride_y > 0 (both or neither, not together with center) m = pixel / stride, the reference's feat_stride; with neither
 * m = pixel.  cells (B,V,J,2) = m rounded once.
 * MPL_RENDER_REFERENCE is generate_heatmap: mu = trunc(m + 0.5) (towards zero, Python's int); weight = conf (NULL: 1), 0 when the
 * patch mu +/- 3 sigma lies wholly outside the map (mu - 3 sigma >= size or mu + 3 sigma + 1 < 0 on an axis); where
 * weight > 0.5 the cells of the patch inside the map hold exp(-(dx^2 + dy^2) / (2 sigma^2)) at integer dx, dy; every other cell is
 * 0.  3 * sigma must be an integer.
 * MPL_RENDER_SUBPIXEL: conf * exp(-((x - mx)^2 + (y - my)^2) / (2 sigma^2)) on every cell, weight = conf; a joint whose conf is not
 * above 0 gets a zero map and weight 0.
 * Both: a cell m that is not finite or beyond +/-2^30 gives a zero map and weight 0 (a deviation: the reference raises).  A value is
 * the fp64 product of its two separable factors, rounded once to `dtype`, denormals kept.  noise_level = a > 0 adds a * u to every
 * cell of every map (zero maps included) before that rounding, u = draw (((first_index + b) * V + v) * J + j) * H * W + y * W + x
 * of the stream noise_key (see mpl_synthesize_views for the draw): a run cut into batches is the uncut run; a == 0 draws nothing.
 * heatmaps / dtype / batch_stride: the table of mpl_decode_heatmaps, written in place; the caller sees to it that the maps do not
 * overlap.  A map whose base address and byte size are multiples of 16 is written with 16-byte stores, any other element by
 * element; the bits are the same.  pixels (B,V,J,2), conf (B,V,J) or NULL: device fp32.  weight (B,V,J), cells (B,V,J,2): fp32 out.
 * MPL_E_INVALID: heatmaps, one of its first `views` entries, pixels, weight or cells NULL; a non-positive size; center without
 * scale or the reverse; one stride without the other, a negative or NaN stride, strides together with center; an unknown dtype or
 * mode; sigma not in (0, 1e6]; 3 * sigma not an integer in MPL_RENDER_REFERENCE; noise_level negative or NaN; first_index < 0;
 * batch_stride < J*H*W.  MPL_E_UNSUPPORTED: views > MPL_MAX_VIEWS, H*W > 2^20, batch*views*joints > 2^30.  All before any launch.
 * Stream-ordered, never synchronises; neither looks at nor sets the device error word. */
#define MPL_RENDER_REFERENCE 0
#define MPL_RENDER_SUBPIXEL 1
int mpl_render_heatmaps(void *const *heatmaps, int dtype, long long batch_stride, int batch, int views, int joints, int height,
                        int width, const float *pixels, const float *conf, const float *center, const float *scale,
                        double stride_x, double stride_y, int mode, double sigma, double noise_level, uint64_t noise_key,
                        long long first_index, float *weight, float *cells, void *stream);

/* ---- recursive pictorial structure model, csrc/rpsm.hip: a 3D pose from the WHOLE heatmaps of all views, in place of
 * lib/multiviews/pictorial.py (numpy, fp64; one pose at a time, a dense nbins x nbins product per edge: 11 s per pose at 16^3 bins).
 * The numpy file is the reference, not pictorial_cuda.py: no [h-1, w-1] mix-up and no soft grid_sample border.  fp64 arithmetic on
 * the fp32 / 16-bit inputs; 2 + (number of tree levels that have children) launches, whatever batch and recur_depth.
 * Grid (compute_grid :106-117): l = linspace(-size/2, size/2, n) (i * step + start, the last point the stop), meshgrid in its default
 * xy indexing: bin (iy*n + ix)*n + iz is (l[ix] + cx, l[iy] + cy, l[iz] + cz) -- y slowest, z fastest; ties go to the first index.
 * Unary (compute_unary_term :144-188): per joint and bin 0.0 plus, view after view, the view's map of the joint sampled at the
 * projection of the bin: x_cam = R (X - t) (the layout of mpl_prepare_inputs), y = x_cam.xy / z, r2 = |y|^2,
 * y' = y (1 + k1 r2 + k2 r2^2 + k3 r2^3 + 2 p1 y.y + 2 p2 y.x) + (p2, p1) r2 (cameras.py:39-45; dist_dev (V,5) k1 k2 k3 p1 p2, NULL =
 * zeros, which give the pinhole bit for bit), px = f y' + c; the crop with rot = 0 in closed form,
 * u = ((px - center) * img_w / (200 * scale_x) + (img_w, img_h) / 2) * (W, H) / (img_w, img_h) (isotropic, scale_y is not read; the
 * inverse of mpl_decode_heatmaps step c; within 7e-15 of the reference's affine solve); then bilinear interpolation of the map at
 * (u_x, u_y) in cells, 0 outside [0, W-1] x [0, H-1] with the borders inside (RegularGridInterpolator(bounds_error=False,
 * fill_value=0); the reference's call only works for square maps, non-square ones get the obvious meaning).
 * Deviation 1 (as in mpl_synthesize_views): a point with z_cam <= 1e-9 contributes 0 from that view.
 * Max-product (infer :18-84): children before parents; a leaf's energy is its unary; for child c of a node and parent bin i the
 * candidates are all child bins j: energy_c[j] where | |g_parent[i] - g_child[j]| - limb[c] | <= tolerance, else 0.0; the first index
 * of the maximum is the back-pointer; the node's energy is its unary times the maxima of its children in ascending child order;
 * the root's first argmax, then down the back-pointers.  NaN counts as the maximum and the first NaN wins (np.argmax).
 * Deviation 2: a disallowed pair is 0.0 even where the child's energy is NaN (the reference multiplies 0 * NaN).
 * In the first round the grid is shared, so the norm depends on m = dix^2 + diy^2 + diz^2 only: the decision is taken as
 * | sqrt(m) * (grid_size / (n-1)) - limb | <= tolerance, which differs from the reference's norm of rounded coordinates only within
 * rounding of the boundary.
 * Recursion (rpsm :233-247): cur = grid_size / first_nbins; recur_depth times: a grid of recur_nbins^3 bins of extent cur about every
 * joint's current point, unary on the joint's own grid, pairwise by the norm between the two joints' grids, the same inference,
 * cur /= recur_nbins.  recur_depth = 0 returns the first round.
 * heatmaps / dtype / batch_stride: as for mpl_decode_heatmaps, read in place.  center, scale: device fp32 (B,V,2).  cams_dev: device
 * (V,16) doubles.  root_center: device fp32 (B,3).  limb: device fp32, row b at limb + b * limb_stride (limb_stride 0: one row for
 * every pose), indexed by the child joint, the root's entry not read.  parents: HOST array of `joints` ints, -1 for the one root.
 * workspace: mpl_rpsm_workspace_bytes(batch, joints, first_nbins) device bytes (fp64 energies per joint and bin, a 16-bit
 * back-pointer per edge and parent bin: 0.7 MB per pose at 17 joints and 16^3).
 * Outputs: poses (B,J,3) fp32, the fp64 grid point rounded once; bins (B, 1 + recur_depth, J) int32, the chosen bin of every round;
 * energy (B) doubles, the root's maximum of the first round.
 * stages: MPL_RPSM_ALL, or for measurements a subset of MPL_RPSM_UNARY | MPL_RPSM_LEVELS | MPL_RPSM_FINAL: only those launches
 * are issued, on the workspace as the call before left it.
 * Envelope: first_nbins 2..16, recur_nbins 2..4, recur_depth 0..16, joints <= 64, views <= MPL_MAX_VIEWS, H, W >= 2,
 * H*W <= 2^20, batch <= 2^20: MPL_E_UNSUPPORTED outside.  MPL_E_INVALID: a NULL pointer (dist_dev excepted), a non-positive
 * size, an unknown dtype, img_w / img_h / grid_size <= 0, tolerance < 0, 0 < limb_stride < joints, batch_stride < J*H*W, parents
 * that are not one tree with exactly one root, stages outside 1..7.  MPL_E_WORKSPACE: workspace NULL or too small.  All before any
 * launch.  Stream-ordered, never synchronises; neither looks at nor sets the device error word. */
#define MPL_RPSM_UNARY 1
#define MPL_RPSM_LEVELS 2
#define MPL_RPSM_FINAL 4
#define MPL_RPSM_ALL 7
size_t mpl_rpsm_workspace_bytes(int batch, int joints, int first_nbins); /* 0 outside the envelope */
int mpl_rpsm(const void *const *heatmaps, int dtype, long long batch_stride, int batch, int views, int joints, int height, int width,
             const float *center, const float *scale, const double *cams_dev, const double *dist_dev, double img_w, double img_h,
             const float *root_center, const float *limb, long long limb_stride, const int *parents, int first_nbins,
             int recur_nbins, int recur_depth, double grid_size, double tolerance, void *workspace, size_t workspace_bytes,
             float *poses, int32_t *bins, double *energy, int stages, void *stream);

/* ---- synthesis of the multi-view model inputs from 3D poses, csrc/synth.hip: the producer in front of mpl_prepare_inputs, in
 * place of what the reference's synthetic datasets run in numpy per sample and view inside Dataset.__getitem__:
 * lib/dataset/multiview_amass_h36m_mpl.py:317-342 (pose placement), lib/utils/calib.py:42-77 (projection),
 * lib/dataset/joints_dataset_mpl.py:592-613 (detection noise, confidence penalty), :701-727 (visibility under NO_AUGMENTATION),
 * :735-740 (missing joints), then :762-774, :615-623, :872-904 exactly as mpl_prepare_inputs.  One launch, one work item per
 * (pose, view, joint); fp64 arithmetic on the fp32 tensors, one rounding per output, no atomics: identical bits from run to run.
 * Steps, per item: 1. X = pose @ Rz(angle)^T about the world origin (rotation_deg, or opt->rotate: 360 * draw), then + the
 * translation (all three components of `translation`, or opt->room: (min + draw * (max - min)) in x and y);  2. x_cam = R (X - t),
 * px = (fx x / z + cx, fy y / z + cy) -> pixels_clean, depth = z;  3. if noise_level != 0: px += noise_level * n, n a
 * standard-normal pair, conf *= penalty(|noise_level * n|): MPL_SYNTH_PENALIZE_EXP_ERROR a exp(-b d), _LINEAR a d + b,
 * _EXP_SQRT exp(-d / 2);  4. clip != 0: conf = 0 unless 0 < x < w-1 and 0 < y < h-1, then x, y clamped to [0, w-1], [0, h-1];
 * clip == 0: conf = 0 where min(x, y) < 0, x >= w or y >= h, and px = (0,0) wherever conf <= 0;  5. if missing_level > 0: conf
 * and px times 0 where a uniform draw < missing_level -> pixels;  6. poses / rays / centers from that fp64 pixel with the
 * arithmetic and the normalize_* switches of mpl_prepare_inputs;  7. target = (X - target_offset) / target_scale per axis.
 * The one deviation: a joint at z <= 1e-9, where the reference divides anyway, gets conf 0 and px (0,0) in pixels_clean and
 * pixels and skips steps 3 to 5.
 * Random numbers: draw i of a stream is the top 53 bits of SplitMix64's finaliser of key + (i + 1) * 0x9E3779B97F4A7C15, a double
 * in [0,1) (openmpl_amd/detrng.py, which also derives the keys).  key_rot, key_room_x, key_room_y are indexed by first_index + b;
 * key_noise0, key_noise1, key_missing by ((first_index + b) * views + v) * joints + j: a run cut into batches draws what the uncut
 * run draws.  The normal pair is Box-Muller: u1 = 1 - draw(key_noise0), u2 = draw(key_noise1), r = sqrt(-2 ln u1),
 * n = (r cos 2 pi u2, r sin 2 pi u2).  A non-NULL rotation_deg (B), translation (B,3), noise (B,V,J,2; standard normal, before the
 * noise_level factor) or missing_u (B,V,J) replaces the stream of that step; a step that is off reads and draws nothing.
 * poses3d (B,J,3), conf (B,V,J) or NULL (-> 1): device fp32;  cams_dev: as for mpl_prepare_inputs.  Outputs: poses / rays /
 * centers host arrays of V device pointers (all three or all NULL), target (B,J,3), pixels, pixels_clean (B,V,J,2), depth (B,V,J),
 * each nullable, at least one given.
 * MPL_E_INVALID: poses3d, cams_dev or opt NULL, no output, a non-positive size, views > MPL_MAX_VIEWS, img_w or img_h <= 0, a
 * target_scale component that is 0, a penalize outside 0..3; MPL_E_UNSUPPORTED: batch * views * joints > 2^36 -- before any
 * launch.  Like the geometry calls it neither looks at nor sets the device error word. */
#define MPL_SYNTH_PENALIZE_NONE 0
#define MPL_SYNTH_PENALIZE_EXP_ERROR 1
#define MPL_SYNTH_PENALIZE_LINEAR 2
#define MPL_SYNTH_PENALIZE_EXP_SQRT 3
typedef struct mpl_synth_options {
    int32_t penalize;                          /* MPL_SYNTH_PENALIZE_* */
    int32_t clip;                              /* DATASET.CLIP_JOINTS */
    int32_t rotate, room;                      /* draw the rotation / the room translation (ignored where a tensor is given) */
    int32_t normalize_inputs, normalize_cameras;
    double noise_level, missing_level;         /* NOISE_LEVEL in pixels (0 = step 3 off), MISSING_LEVEL (<= 0 = step 5 off) */
    double penalize_a, penalize_b;
    double room_min_x, room_max_x, room_min_y, room_max_y;
    double img_w, img_h;                       /* NETWORK.IMAGE_SIZE */
    double target_scale[3], target_offset[3];
    uint64_t key_rot, key_room_x, key_room_y, key_noise0, key_noise1, key_missing;
    int64_t first_index;                       /* global index of pose 0 of this call */
} mpl_synth_options;
int mpl_synthesize_views(const float *poses3d, const double *cams_dev, const mpl_synth_options *opt, const float *conf,
                         const float *rotation_deg, const float *translation, const float *noise, const float *missing_u,
                         int batch, int views, int joints, float *const *poses, float *const *rays, float *const *centers,
                         float *target, float *pixels, float *pixels_clean, float *depth, void *stream);

/* ---- lens distortion, csrc/views.hpp and csrc/distortion.hip: one model for every call that projects or builds a ray.
 * The distortion record is dist_dev, device (V,5) float64 k1 k2 k3 p1 p2 per view, the layout mpl_rpsm takes.  With y = x_cam.xy / z
 * and r2 = |y|^2 the lens maps y to  y_d = y g + (p2, p1) r2,  g = 1 + (k1 r2 + k2 r2^2 + k3 r2^3) + (2 p1 y.y + 2 p2 y.x),  and
 * the pixel is f y_d + c: the reference's project_point_radial (lib/multiviews/cameras.py:22-46), the form of the H36M toolbox.  It
 * is NOT OpenCV's model, whose tangential terms are 2 p1 x y + p2 (r2 + 2 x^2) and p1 (r2 + 2 y^2) + 2 p2 x y.  The reference is not
 * consistent here: lib/multiviews/triangulate.py:26-38 hands the same five numbers, reordered to (k1 k2 p1 p2 k3), to pymvg, which
 * undistorts with OpenCV's model.  This library inverts the model it projects with.
 * The inverse is Newton's iteration in fp64 from y = y_d with the analytic 2x2 Jacobian J: at most 20 iterations (the
 * calibrations of Human3.6M and CMU Panoptic take 6); done when max |step| <= 1e-14 * max(1, |y|_inf); an iterate with det J <= 0
 * (the point lies beyond the fold of the polynomial, where no pinhole point maps to it), a non-finite value or an exhausted cap
 * makes the point NOT INVERTIBLE.  With all-zero coefficients the first residual is exactly 0 and y = y_d bit for bit.
 *
 * mpl_undistort_points: one launch, one work item per (b, v, j), fp64 on the fp32 pixel (x, y) of pixels (B,V,J,2).
 * MPL_DISTORT_REMOVE: y_d = ((x - cx) / fx, (y - cy) / fy), y_u its inverse, out = (x + fx (y_u.x - y_d.x), y + fy (y_u.y - y_d.y)),
 * rounded once: zero coefficients return the input.  A point that is not invertible gives NaN in both coordinates and valid = 0.
 * MPL_DISTORT_APPLY: the forward polynomial on a pinhole pixel, in the same form: y = ((x - cx) / fx, (y - cy) / fy),
 * out = (x + fx (y_d.x - y.x), y + fy (y_d.y - y.y)); always valid.
 * out_pixels (B,V,J,2) fp32; out_valid (B,V,J) bytes of 0 / 1, or NULL.  cams_dev as for mpl_prepare_inputs.
 * MPL_E_INVALID: pixels, cams_dev, dist_dev or out_pixels NULL, a non-positive size, views > MPL_MAX_VIEWS, an unknown direction;
 * MPL_E_UNSUPPORTED: batch * views * joints > 2^30 -- before any launch.  Stream-ordered, never synchronises; neither looks at nor
 * sets the device error word. */
#define MPL_DISTORT_REMOVE 0
#define MPL_DISTORT_APPLY 1
int mpl_undistort_points(const float *pixels, const double *cams_dev, const double *dist_dev, int batch, int views, int joints,
                         int direction, float *out_pixels, unsigned char *out_valid, void *stream);

/* mpl_prepare_inputs with a lens.  poses are what they are without it: the observed pixel, normalised as the switches say, plus
 * the confidence.  The ray goes through the undistorted pixel (x + fx D.x, y + fy D.y), D = y_u - y_d formed from the raw
 * intrinsics before any normalisation, on which the ray arithmetic of mpl_prepare_inputs then runs.  A joint that is not invertible
 * keeps its pinhole ray and gets confidence 0 in poses[..., 2], like a missing joint: mpl_triangulate_rays, mpl_triangulate_robust
 * and mpl_epipolar_errors then leave that view out.  dist_dev == NULL launches the kernel of mpl_prepare_inputs: same bits.  Zero
 * coefficients give those bits too.  Arguments and refusals otherwise as for mpl_prepare_inputs. */
int mpl_prepare_inputs_ex(const float *joints_px, const float *conf, const double *cams_dev, const double *dist_dev, int batch,
                          int views, int joints, float img_w, float img_h, int normalize_inputs, int normalize_cameras,
                          float *const *poses, float *const *rays, float *const *centers, void *stream);

/* mpl_synthesize_views with a lens.  Step 2 becomes px = (fx y_d.x + cx, fy y_d.y + cy) with y = x_cam.xy / z, the form of mpl_rpsm
 * (under zero coefficients this rounds differently from fx x / z + cx: within fp64 rounding of the pinhole launch, not bitwise);
 * pixels_clean, the noise, the visibility step and the missing-joint step act on distorted pixels, as a detector sees them; step 6
 * is the arithmetic of mpl_prepare_inputs_ex on the fp64 pixel.  Depth, target and the z <= 1e-9 rule do not change.
 * dist_dev == NULL launches the kernel of mpl_synthesize_views: same bits.  Arguments and refusals otherwise as for
 * mpl_synthesize_views. */
int mpl_synthesize_views_ex(const float *poses3d, const double *cams_dev, const double *dist_dev, const mpl_synth_options *opt,
                            const float *conf, const float *rotation_deg, const float *translation, const float *noise,
                            const float *missing_u, int batch, int views, int joints, float *const *poses, float *const *rays,
                            float *const *centers, float *target, float *pixels, float *pixels_clean, float *depth, void *stream);

/* ---- multi-view geometry on the tensors of mpl_inputs, csrc/geometry.hip: rays[v] (B,J,3) is a world point on the line of
 * sight of view v (joints_dataset_mpl.py:872-904), centers[v] (B,1,3) the camera centre; line v goes through c_v along
 * d_v = (r_v - c_v) / |r_v - c_v|.  rays / centers / conf are HOST arrays of `views` device pointers; conf may be NULL (every
 * confidence 1).  conf_stride: 1 = conf[v] is a (B,J) tensor; 3 = conf[v] is one of the model's own (B,J,3) pose tensors
 * (mpl_inputs.poses), whose channel 2 is read in place.  fp64 arithmetic on the fp32 inputs, fp32 outputs, one work item per
 * (sample, joint), no floating-point atomics: identical bits from run to run, and a sample does not depend on its batch mates.
 * MPL_E_INVALID: a NULL pointer, a non-positive size, a conf_stride other than 1 or 3; MPL_E_UNSUPPORTED: views > MPL_MAX_VIEWS,
 * joints > 64, batch * joints > 2^30, views < 2 for mpl_epipolar_errors -- before any launch.  Neither call looks at or sets
 * the device error word.
 * mpl_triangulate_rays: the geometric baseline of a multi-view lifter, in place of lib/multiviews/triangulate.py (pymvg, on the
 * host).  out_points (B,J,3) = cbar + A^-1 b with A = sum_v w_v (I - d_v d_v^T), b = sum_v w_v (I - d_v d_v^T)(c_v - cbar), cbar
 * the mean camera centre of the sample, w_v the confidence of (sample, view, joint); a view with w_v <= 0 or a non-finite w_v does
 * not take part.  out_residual (B,J) = sqrt(sum_v w_v dist(x, line_v)^2 / sum_v w_v).  A joint with fewer than two views taking
 * part, or with det(A / sum w) < 1e-10 (two views: sin^2(angle) / 4, i.e. lines within about 2e-5 rad of parallel), is
 * degenerate: its point and its residual are NaN.
 * mpl_epipolar_errors: lib/utils/calib.py:116-169 smart_pseudo_remove_weight with :94-113 distance_between_two_skew_lines, which
 * the multi-view datasets run in numpy per sample.  out_err (B,V,J): err[b,i,j] = conf_i / (V - 1) * sum_{k != i} dist(line_i,
 * line_k), dist = |(c_k - c_i) . (d_i x d_k)| / |d_i x d_k| (:162-165: every pair counts, the confidence scales only the view's
 * own total).  The one deviation: where |d_i x d_k|^2 < 1e-20 the reference divides 0 by 0; here the pair contributes the
 * distance of c_k to line i, the limit of the formula.  weight_in / weight_out (both or neither), (B,V,J): weight_out = 0 where
 * err > threshold, weight_in elsewhere (:167-168); two distinct buffers. */
int mpl_triangulate_rays(const float *const *rays, const float *const *centers, const float *const *conf, int conf_stride,
                         int batch, int views, int joints, float *out_points, float *out_residual, void *stream);
int mpl_epipolar_errors(const float *const *rays, const float *const *centers, const float *const *conf, int conf_stride,
                        int batch, int views, int joints, float *out_err, const float *weight_in, float threshold,
                        float *weight_out, void *stream);
/* mpl_triangulate_robust: mpl_triangulate_rays with the outliers taken out first, per (sample, joint) in three stages.
 * 1. Candidates: the views that take part (w_v > 0 and finite).  conf_threshold >= 0 (a negative or NaN value: off) adds the
 * view selection of lib/multiviews/triangulate.py:94-102 over all `views` confidences in fp64, literally: th = conf_threshold;
 * loop { sel = conf > th; if th < -1 stop; if |sel| <= 1 then th -= 0.05 (repeated subtraction: the reference's thresholds bit
 * for bit) else stop }; the candidates are sel without the views that do not take part.  Two deviations: below th = 0 the
 * reference would select zero-confidence views, here they stay out; and the reference never resets th between the joints of a
 * pose (a joint inherits what an earlier one lowered), here every joint starts at conf_threshold.
 * 2. Consensus, with threshold >= 0 (tau in world units; negative or NaN: off): every candidate pair i < k is a hypothesis, the
 * equal-weight least-squares point of the two lines (the midpoint of their common perpendicular), solved about the mean of the
 * two centres and skipped where det(A / 2) < 1e-10.  A hypothesis counts the candidates with dist(x, line_v) <= tau and costs
 * sum over the candidates of w_v min(dist^2, tau^2); the winner is the highest count, then the lowest cost, then the lowest i,
 * then the lowest k -- a total order, so the result does not depend on how the pairs were dealt out.  Its dist <= tau set is the
 * inlier set.  Without threshold every candidate is an inlier.
 * 3. Refit: out_points / out_residual are those of mpl_triangulate_rays with the weights w_v over the inlier set (cbar stays the
 * mean of all `views` centres).  With both stages off the call writes what mpl_triangulate_rays writes.
 * out_inliers (B,V,J), the layout of out_err: 1 for the views of the inlier set, else 0.  Fewer than two candidates, no
 * non-degenerate pair, a winning count below min_inliers, or a degenerate refit are statements about the joint: its point and
 * residual are NaN and its inliers all 0; a finite point has at least two inliers.  One launch; pairs are dealt to the waves of
 * a workgroup that holds the lines of 64 items in LDS.
 * Besides the codes above, MPL_E_INVALID: a NULL output, conf_threshold on without conf, min_inliers outside [2, views];
 * MPL_E_UNSUPPORTED: conf_threshold > 64 (the descent is a loop in every thread) -- before any launch. */
int mpl_triangulate_robust(const float *const *rays, const float *const *centers, const float *const *conf, int conf_stride,
                           int batch, int views, int joints, double threshold, double conf_threshold, int min_inliers,
                           float *out_points, float *out_residual, float *out_inliers, void *stream);

/* ---- refinement of 3D points by their reprojection error, csrc/refine.hip.  The triangulations above minimise the distance to the
 * lines of sight in world units; a detector errs in pixels.  mpl_refine_points minimises, per (sample, joint) and from the point it
 * is given, E(X) = sum_v w_v rho(|r_v|^2) with r_v = proj_v(X) - px_v in pixels, and reports the reprojection error of the result; with
 * max_iterations == 0 it is the reprojection error of any 3D estimate.  The reference has no such step.
 * points (B,J,3), pixels (B,V,J,2), conf (B,V,J) or NULL (every weight 1): the layout of mpl_prepare_inputs; cams_dev (V,16);
 * dist_dev (V,5) or NULL (the pinhole).  views <= MPL_MAX_VIEWS, joints <= 64, batch * views * joints <= 2^30.
 * Projection: that of mpl_synthesize_views_ex, x_cam = R (X - t), y = x_cam.xy / z, the lens polynomial above, px = f y_d + c; zero
 * coefficients give the pinhole projection.  Its Jacobian is analytic: diag(f) (the lens Jacobian of the inverse above)
 * (d y / d x_cam) R.
 * Participation: view v takes part in an item when w_v is finite and > 0 and both pixel coordinates are finite.
 * Cost: huber <= 0 or NaN, the plain mode: rho(s) = s.  huber = h > 0: rho(s) = s if s <= h^2, else 2 h sqrt(s) - h^2.  E is +inf
 * where a view that takes part has z_cam <= 1e-9 at X.
 * Iteration: Levenberg-Marquardt on the 3 unknowns.  H = sum w'_v J_v^T J_v, g = sum w'_v J_v^T r_v, w'_v = w_v in the plain mode and
 * the IRLS weight w_v min(1, h / |r_v|) in the Huber mode; (H + lambda diag H) delta = -g is solved in closed form; lambda starts at
 * 1e-3.  The trial X + delta is accepted only if its E is strictly lower, then lambda = max(lambda / 10, 1e-15); otherwise lambda *=
 * 10 and X stays: E never increases.  Every trial counts as one iteration.  After a trial, accepted or not: converged when
 * max |delta| <= step_tolerance * z_min, z_min the smallest z_cam at (the possibly new) X among the views that take part -- a length
 * scale that does not know whether the world is in metres or millimetres --; else capped when lambda > 1e12 or after max_iterations
 * trials.
 * Outputs per item: out_points (B,J,3) the final point; out_error (B,J) = sqrt(sum w |r|^2 / sum w) at it over the views that take
 * part, the plain weighted RMS in both modes, so that numbers compare across modes; out_errors (B,V,J) = |r_v| in pixels, NaN for a
 * view that takes no part; out_iterations (B,J) the trials made; out_status (B,J) bytes:
 *   0 converged;  1 capped;
 *   2 passed through: fewer than two views take part, or max_iterations == 0; the point is returned bit for bit and the errors are
 *     those of the views that take part;
 *   3 invalid: the given point is not finite, no view takes part, or a view that takes part has the point at z_cam <= 1e-9; point,
 *     error and errors are NaN.  A statement about the item: no device error, and no other item is touched.
 * out_errors, out_iterations and out_status may be NULL.
 * One launch, one thread per item, the views summed in their order, fp64 on the fp32 tensors, every output rounded once, no atomics:
 * identical bits from run to run and from batching to batching.  Stream-ordered, never synchronises; neither looks at nor sets the
 * device error word.
 * MPL_E_INVALID: points, pixels, cams_dev, out_points or out_error NULL, a size that is not positive or beyond the limits above;
 * MPL_E_UNSUPPORTED: max_iterations outside [0, 1000], a step_tolerance that is negative or not finite -- before any launch. */
int mpl_refine_points(const float *points, const float *pixels, const float *conf, const double *cams_dev, const double *dist_dev,
                      int batch, int views, int joints, double huber, int max_iterations, double step_tolerance,
                      float *out_points, float *out_error, float *out_errors, int *out_iterations, unsigned char *out_status,
                      void *stream);

/* ---- refinement of the camera poses by the same error, csrc/refine_cameras.hip: the transpose of mpl_refine_points.  The points are
 * given and the cameras move: per view v, from the pose it is given, E_v(R, t) = sum_{b,j} w_bvj rho(|r_bvj|^2) with
 * r = proj_v(X_bj) - px_bvj in pixels is minimised over the 6 unknowns of the pose.  Arguments, layouts, limits, projection, lens,
 * weights and rho are those of mpl_refine_points; the intrinsics and the lens row are not unknowns (the intrinsics are copied to
 * the output).  The reference has no such step (its PoseUtils.estimate_camera is a weak-perspective fit).
 * Participation: observation (b, j) of view v takes part when its weight is finite and > 0, its pixel is finite and the three
 * coordinates of X_bj are finite -- NaN joints of a triangulation drop out.  out_used[v] counts them.
 * Parametrisation: a trial pose is R' = exp([w]x) R, t' = t + dt, delta = (w, dt); exp([w]x) = I + a K + b K^2 with K = [w]x,
 * a = sin(th) / th, b = (1 - cos(th)) / th^2 (their series below th^2 = 1e-8), in fp64.  With x_cam = R (X - t) and M = d px / d x_cam
 * the 2x6 Jacobian is M [ -[x_cam]x | -R ].
 * Iteration: the loop of mpl_refine_points on 6 unknowns.  H = sum w' J^T J, g = sum w' J^T r with the IRLS weights;
 * (H + lambda diag H) delta = -g by an unpivoted Cholesky factorisation (a pivot that is <= 0 or not finite gives a NaN step, which
 * no trial survives); lambda starts at 1e-3; a trial that lowers E strictly and leaves every participating point at z_cam > 1e-9 is
 * accepted, then lambda = max(lambda / 10, 1e-15); otherwise lambda *= 10 and the pose stays: E never increases.  After a trial,
 * accepted or not: converged when max |w| <= step_tolerance and max |dt| <= step_tolerance * z_min, z_min the smallest depth of a
 * participating point at the accepted pose; else capped when lambda > 1e12 or after max_iterations trials.
 * Outputs per view: out_cams (V,16) the record with the final pose; out_error (V) = sqrt(sum w |r|^2 / sum w) there, the plain
 * weighted RMS in pixels in both modes; out_cost0, out_cost (V) = E at the given and at the final pose, in the mode of the call, so
 * out_cost <= out_cost0; out_used, out_iterations (V) ints; out_status (V) bytes:
 *   0 converged;  1 capped;
 *   2 passed through: bit v of fixed_mask is set, max_iterations == 0, or fewer than 3 observations take part; the record is
 *     returned bit for bit, error and costs are computed, out_cost == out_cost0;
 *   3 invalid: no observation takes part, the given record is not finite, or a participating point is not in front of the given
 *     camera; the record is returned as given (a NaN row would poison every later call), error and costs are NaN.  A statement
 *     about the view: no device error, and no other view is touched.
 * Bits of fixed_mask at or above `views` are ignored.  conf, dist_dev, out_cost0, out_cost, out_used, out_iterations and
 * out_status may be NULL.  out_cams may be cams_dev: a workgroup reads its row before it writes it and touches no other row.
 * One launch, one workgroup per view; the sums over the observations are fp64, reduced down the waves and across them in a fixed
 * order, without atomics: identical bits from run to run.  Stream-ordered, never synchronises; neither looks at nor sets the device
 * error word.  The trial count is bounded by max_iterations whatever the data.
 * MPL_E_INVALID: points, pixels, cams_dev, out_cams or out_error NULL, a size that is not positive or beyond the limits;
 * MPL_E_UNSUPPORTED: max_iterations outside [0, 1000], a step_tolerance that is negative or not finite -- before any launch. */
int mpl_refine_cameras(const float *points, const float *pixels, const float *conf, const double *cams_dev, const double *dist_dev,
                       int batch, int views, int joints, double huber, int max_iterations, double step_tolerance, unsigned fixed_mask,
                       double *out_cams, double *out_error, double *out_cost0, double *out_cost, int *out_used, int *out_iterations,
                       unsigned char *out_status, void *stream);

/* ---- locating cameras from scratch, csrc/locate_cameras.hip: robust resection.  mpl_refine_cameras starts from a pose that is
 * nearly right; mpl_locate_cameras finds one where there is none, in the presence of wrong detections, by hypothesise-and-score: per
 * view, `hypotheses` poses from six observations each, every one scored over all observations of the view.  Arguments, layouts and
 * limits are those of mpl_refine_cameras.  Of a view's record only fx fy cx cy are read, and its lens row; the pose fields of a view
 * that is not in fixed_mask are not looked at and may be NaN.  The reference has no such step.  One definition for the device and
 * for the float64 restatement of the tests:
 * 1. Participation is that of mpl_refine_cameras -- the weight finite and > 0, the pixel finite, the point finite -- and the pixel
 *    goes back through the lens (the inverse above succeeds).  Slot n = b * joints + j, N = batch * joints.  The normalised
 *    observation y = ((xu - cx) / fx, (yu - cy) / fy) of the undistorted pixel (xu, yu).
 * 2. Per view, m = the mean of the participating points and s = 1 / sqrt(mean |X - m|^2 / 3), in fp64, summed in a fixed order; the
 *    system is built on Xh = (s (X - m), 1).
 * 3. Hypothesis h of view v draws six distinct participating slots: slot k, attempt a (0 .. 15) takes
 *    n = floor(draw(keys[v], (h * 6 + k) * 16 + a) * N), draw the counter-based generator of mpl_synthesize_views; the first attempt
 *    that participates and is not already chosen is kept; sixteen failures make the hypothesis void.  keys: HOST array of `views`
 *    stream keys (Python: detrng._stream_key(seed, "locate_cameras", lane=v)).
 * 4. The 12 x 12 system has the rows [Xh, 0, -y0 Xh] and [0, Xh, -y1 Xh] of the six samples; P (3 x 4, row-major) is its right
 *    singular vector of the smallest singular value (a one-sided Jacobi on the system itself), with the sign that makes the summed
 *    depth P_3 . Xh of the six samples positive.  Its left 3 x 3 block M = U S W^T gives R = U W^T, the column of the smallest
 *    singular value turned over where det M < 0 so that det R = +1; scale = the mean singular value, t = P_4 / scale, and the centre
 *    is c = m - R^T t / s.  Void: a singular value of M that is not > 0, a pose that is not finite, or a sample point at
 *    z_cam <= 1e-9 under the pose.
 * 5. The score of a hypothesis over all participating slots, with the projection of mpl_refine_cameras, lens included:
 *    count = #{in front and |r|^2 <= threshold^2}, cost = sum w min(|r|^2, threshold^2), where a point that is not in front costs
 *    w threshold^2; summed over the slots in their order, so the bits do not depend on the grid.  A void hypothesis scores (0, +inf).
 * 6. The winner has the most inliers, then the lowest cost, then the lowest h.
 * Outputs per view: out_cams (V,16), the intrinsics as given with the winner's pose; out_inliers (B,V,J) floats 0 / 1, the
 * winner's within-threshold set; out_count (V) its size; out_best (V) the winner, -1 where every hypothesis is void; out_error (V)
 * the plain root-mean-square of |r| in pixels over the inliers; out_status (V) bytes:
 *   0 located;
 *   2 passed through: bit v of fixed_mask is set; the record is returned bit for bit, out_best is -1, and inliers, count and error
 *     are those of the given pose (count 0 and error NaN where it projects nothing within the threshold);
 *   3 invalid: fewer than 6 observations take part, no hypothesis is valid, the winner has fewer than 6 inliers, or the intrinsics
 *     are not finite; the record is returned as given, error is NaN, count 0 and the inliers 0.
 * out_poses (V,hypotheses,12): R row-major, then the centre, NaN for a void hypothesis; out_scores (V,hypotheses,2): count, cost.
 * Every hypothesis of a view that is fixed or has fewer than 6 participating observations is void.
 * workspace: mpl_locate_cameras_workspace_bytes(batch, views, joints) device bytes (the participating observations of every view).
 * Three launches -- observations, hypotheses (one lane each), winners --, fp64, no atomics, every sum in a fixed order: identical
 * bits from run to run.  Stream-ordered, never synchronises; neither looks at nor sets the device error word.  out_cams may be
 * cams_dev.
 * MPL_E_INVALID: points, pixels, cams_dev, keys or an output NULL, a size that is not positive or beyond the limits;
 * MPL_E_UNSUPPORTED: a threshold that is not finite and > 0, hypotheses outside [1, 65536]; MPL_E_WORKSPACE: no workspace or too
 * small a one -- in this order, before any launch. */
size_t mpl_locate_cameras_workspace_bytes(int batch, int views, int joints); /* 0 outside the limits */
int mpl_locate_cameras(const float *points, const float *pixels, const float *conf, const double *cams_dev, const double *dist_dev,
                       int batch, int views, int joints, double threshold, int hypotheses, const unsigned long long *keys,
                       unsigned fixed_mask, void *workspace, size_t workspace_bytes, double *out_cams, float *out_inliers,
                       int *out_count, int *out_best, double *out_error, unsigned char *out_status, double *out_poses,
                       double *out_scores, void *stream);

/* ---- the relative pose of two views from their detections alone, csrc/relative_pose.hip with csrc/five_point.hpp: robust
 * five-point solver.  mpl_locate_cameras needs 3D points; mpl_relative_pose is the step before it, for a rig of which nothing is
 * known but the intrinsics: per pair of views (a, b), `hypotheses` five-point solutions, every candidate scored over all
 * correspondences of the pair.  pixels (B,V,J,2), conf (B,V,J) or NULL, cams_dev (V,16) -- only fx fy cx cy are read, the pose
 * fields may be NaN --, dist_dev (V,5) or NULL; pairs: HOST array (n_pairs,2) of view indices, a != b, n_pairs <= MPL_MAX_VIEWS;
 * views <= MPL_MAX_VIEWS, joints <= 64, batch * views * joints and batch * n_pairs * joints <= 2^30.  The convention is
 * x_b = R x_a + t with |t| = 1 (the length of the baseline cannot be seen).  The reference has no such step.  One definition for
 * the device and for the float64 restatement of the tests:
 * 1. Slot n = b * joints + j, N = batch * joints.  It takes part in pair (a, b) when in both views the weight is finite and > 0,
 *    the pixel is finite and goes back through the lens (the inverse above succeeds), and both views' intrinsics are finite.  Its
 *    weight is w = conf_a * conf_b (1 without conf); u_a, u_b are the undistorted pixels, y = ((u0 - cx) / fx, (u1 - cy) / fy) their
 *    normalised coordinates.  A pair is usable with at least 5 participating slots.
 * 2. Hypothesis h of pair p draws five distinct participating slots by the scheme of step 3 of mpl_locate_cameras: slot k, attempt a
 *    (0 .. 15) takes n = floor(draw(keys[p], (h * 5 + k) * 16 + a) * N); the first attempt that participates and is not already
 *    chosen is kept; sixteen failures make the hypothesis void.  keys: HOST array of n_pairs stream keys (Python:
 *    detrng._stream_key(seed, "relative_pose", lane=p)).
 * 3. The candidates are all real E with d_b^T E d_a = 0 on the five samples (d = (y0, y1, 1)), det E = 0 and
 *    2 E E^T E - tr(E E^T) E = 0.  The 5 x 9 system has the rows kron(d_b, d_a); its null space comes from a one-sided Jacobi on
 *    the system itself (the four shortest columns of A V), and X, Y, Z, W of E = x X + y Y + z Z + W are the columns of the
 *    projector on it at the four largest entries of its diagonal (descending, the lowest index among equals), made orthonormal in
 *    that order by Gram-Schmidt with every projection taken twice: a basis that does not depend on how the null space was found.
 *    The ten cubics in the 20 monomials of degree <= 3
 *    are eliminated by Gauss-Jordan with partial pivoting on the columns x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy; the rows
 *    <x^2 z> - z <x^2>, <y^2 z> - z <y^2>, <xyz> - z <xy> form a 3 x 3 polynomial matrix B(z) with B(z) (x, y, 1)^T = 0 (Nister).
 *    The real roots of det B(z), of degree 10, are counted and isolated by a Sturm chain, bisected and polished by Newton, in
 *    ascending order; (x, y, 1) is the cross product of the two rows of B(z) that make the longest one, and (x, y, z) is then
 *    polished by three Gauss-Newton steps on the ten cubics themselves (B(z) loses its rank by two where two candidates have
 *    nearly the same z).  `roots` of a hypothesis is the number of real roots.
 *    The pose of a candidate: E = U diag(s) V^T by the 3 x 3 Jacobi of mpl_locate_cameras with U, V
 *    proper, R in {U W V^T, U W^T V^T}, t = +-u_3, in that order; the first combination that puts all five samples at a depth
 *    > 1e-9 in both cameras is kept, the depths (l_a, l_b) of l_a R d_a - l_b d_b = -t by its 2 x 2 normal equations; none doing so
 *    makes the candidate void.
 * 4. The score of a candidate over all participating slots in their order: the signed Sampson distance in pixels on the
 *    undistorted pixels, d = u_b^T F u_a / sqrt((F u_a)_0^2 + (F u_a)_1^2 + (F^T u_b)_0^2 + (F^T u_b)_1^2) with
 *    F = K_b^-T [t]x R K_a^-1; count = #{d^2 <= threshold^2}, cost = sum w min(d^2, threshold^2).  A hypothesis keeps its best
 *    candidate: most inliers, then the lowest cost, then the lowest root.  A hypothesis without a valid candidate scores (0, +inf).
 * 5. The winner has the most inliers, then the lowest cost, then the lowest h.
 * The draws are keyed by the pair's index p, not by its views: the pairs (0,1) and (1,0) of one call draw different samples, and
 * only as pair 0 of a call each do they see the same hypotheses (then R_10 = R_01^T, t_10 = -R_01^T t_01 hypothesis by hypothesis).
 * Outputs per pair: out_rotation (P,3,3) row-major and out_direction (P,3), the winner's R and t; out_cams (P,2,16): record 0 is
 * view a with R = I and centre 0, record 1 is view b with R and the centre -baseline * R^T t, the intrinsics as given;
 * out_inliers (B,P,J) floats 0 / 1, the winner's within-threshold set; out_count (P) its size; out_best (P) the winner, -1 where
 * every hypothesis is void; out_error (P) the root-mean-square of |d| in pixels over the inliers; out_status (P) bytes:
 *   0 located: the winner has at least 6 inliers, one more than a sample fits by construction;
 *   3 invalid: fewer than 5 slots take part, no hypothesis is valid, the winner has fewer than 6 inliers, or the intrinsics of a
 *     view are not finite; rotation, direction and the pose fields of both records are NaN, error is NaN, count 0, the inliers 0.
 * out_poses (P,hypotheses,12): R row-major, then t, NaN for a void hypothesis; out_scores (P,hypotheses,2): count, cost;
 * out_roots (P,hypotheses) ints.
 * workspace: mpl_relative_pose_workspace_bytes(batch, n_pairs, joints) device bytes (the correspondences of every pair).
 * Three launches -- correspondences, hypotheses (one lane each), winners --, fp64, no atomics, every sum in a fixed order:
 * identical bits from run to run.  Stream-ordered, never synchronises; neither looks at nor sets the device error word.
 * MPL_E_INVALID: pixels, cams_dev, pairs, keys or an output NULL, a size that is not positive or beyond the limits, a pair that is
 * not two distinct views; MPL_E_UNSUPPORTED: a threshold or a baseline that is not finite and > 0, hypotheses outside [1, 65536];
 * MPL_E_WORKSPACE: no workspace or too small a one -- in this order, before any launch. */
size_t mpl_relative_pose_workspace_bytes(int batch, int pairs, int joints); /* 0 outside the limits */
int mpl_relative_pose(const float *pixels, const float *conf, const double *cams_dev, const double *dist_dev, int batch, int views,
                      int joints, const int *pairs, int n_pairs, double threshold, int hypotheses, const unsigned long long *keys,
                      double baseline, void *workspace, size_t workspace_bytes, double *out_rotation, double *out_direction,
                      double *out_cams, float *out_inliers, int *out_count, int *out_best, double *out_error,
                      unsigned char *out_status, double *out_poses, double *out_scores, int *out_roots, void *stream);

/* ---- the polish of a relative pose, csrc/refine_relative_pose.hip: Levenberg-Marquardt on the 5 unknowns of (R, t), |t| = 1, over
 * the signed Sampson distances d of step 4 of mpl_relative_pose, from the pose it is given (rotation (P,3,3), direction (P,3)).  It is
 * the loop of mpl_refine_cameras -- lambda from 1e-3, divided by 10 after a trial that lowers the cost strictly and multiplied by 10
 * after one that does not, the statuses, the limits -- on E(R, t) = sum w rho(d^2), rho plain or Huber as in mpl_refine_points
 * (huber in pixels; <= 0 or NaN: plain).  Alternating bundle adjustment is no substitute: it crawls along the two-view valley.
 * Participation and weights: those of step 1 of mpl_relative_pose, w = conf_a * conf_b, times weight[b, p, j] where `weight` (B,P,J)
 * is given (finite and > 0 to take part): the inlier mask of mpl_relative_pose is such a tensor.  conf, weight, dist_dev may be NULL.
 * Trial: R' = exp([w]x) R (Rodrigues, as mpl_refine_cameras), t' = normalise(t + d1 e1 + d2 e2), delta = (w, d1, d2); e1 =
 * normalise(t x axis_k) with k the coordinate of t of the smallest magnitude (the lowest among equals), e2 = t x e1.
 * Jacobian, analytic: with a = K_a^-1 u_a, b = K_b^-1 u_b and E = [t]x R, d = n / s, n = b^T E a, s^2 = (E a)_0^2 / fx_b^2 +
 * (E a)_1^2 / fy_b^2 + (E^T b)_0^2 / fx_a^2 + (E^T b)_1^2 / fy_a^2 = |g|^2; along a direction E' of E the derivative is
 * n' / s - n (g . g') / s^3; the five directions are [t]x [e_k]x R (k = 0, 1, 2), [e1]x R and [e2]x R.  H = sum w' J J^T,
 * g = sum w' J d with the IRLS weights; (H + lambda diag H) delta = -g by an unpivoted Cholesky factorisation.
 * After a trial, accepted or not: converged when max |delta| <= step_tolerance; else capped when lambda > 1e12 or after
 * max_iterations trials.
 * Outputs per pair: out_rotation, out_direction the final pose; out_cams (P,2,16) the two records of mpl_relative_pose under it;
 * out_error = sqrt(sum w d^2 / sum w) there, in both modes; out_cost0, out_cost = E at the given and the final pose, out_cost <=
 * out_cost0; out_used the correspondences that take part; out_iterations the trials; out_status bytes:
 *   0 converged;  1 capped;
 *   2 passed through: max_iterations == 0 or fewer than 6 correspondences take part; the pose is returned bit for bit, error and
 *     costs are computed, out_cost == out_cost0;
 *   3 invalid: the given pose or the intrinsics are not finite, or nothing takes part; the pose is returned as given, the pose fields
 *     of the records, error and costs are NaN.
 * out_cost0, out_cost, out_used, out_iterations, out_status may be NULL.  One launch, one workgroup per pair, fp64 sums in a fixed
 * order, no atomics: identical bits from run to run.  Stream-ordered, never synchronises.
 * MPL_E_INVALID: pixels, cams_dev, pairs, rotation, direction or one of the first four outputs NULL, a size beyond the limits of
 * mpl_relative_pose, a pair that is not two distinct views; MPL_E_UNSUPPORTED: max_iterations outside [0, 1000], a step_tolerance
 * that is negative or not finite, a baseline that is not finite and > 0 -- before any launch. */
int mpl_refine_relative_pose(const float *pixels, const float *conf, const float *weight, const double *cams_dev,
                             const double *dist_dev, int batch, int views, int joints, const int *pairs, int n_pairs,
                             const double *rotation, const double *direction, double huber, int max_iterations,
                             double step_tolerance, double baseline, double *out_rotation, double *out_direction, double *out_cams,
                             double *out_error, double *out_cost0, double *out_cost, int *out_used, int *out_iterations,
                             unsigned char *out_status, void *stream);

/* ---- refinement of whole poses under bone-length constraints, csrc/refine_poses.hip.  mpl_refine_points moves every joint on its
 * own; here the joints of a pose are one body on a tree with bones of known length.  Per pose, from the pose it is given,
 *   E(X) = sum_{v,j} w_vj rho(|proj_v(X_j) - px_vj|^2) + bone_weight * sum_{live bones j} ((|X_j - X_p(j)| - L_j) / L_j)^2
 * is minimised over the joints that take part.  The first sum is the cost of mpl_refine_points to the letter (arguments, layouts,
 * limits, projection, lens, weights, view participation, rho and the IRLS weights), in px^2; the bone residual is relative, so
 * bone_weight is px^2 per unit of relative length error whatever the world unit, and the bone term is always quadratic.  The
 * reference has no such step (lib/multiviews/pictorial.py uses limb_length on a grid; mpl_rpsm is that search).
 * limb: device float32, indexed by the child joint, the root's entry not read; limb_stride 0: one row (J,) for every pose, else
 * (B,J) rows limb_stride >= joints apart.  parents: host, `joints` ints, -1 for the one root (as mpl_rpsm takes them).
 * Participation: a bone is live when both its ends have a finite given point and a view that takes part, and L_j is finite and > 0
 * (a NaN length switches a bone off).  A joint takes part when its given point is finite and it is seen by two views that take
 * part, or by one and is an end of a live bone.  A joint that takes no part is returned bit for bit, its error is NaN and its views
 * and bones count nowhere.
 * Iteration: Levenberg-Marquardt on the 3 J' unknowns with the schedule and constants of mpl_refine_points.  H has one 3x3 block per
 * joint (sum w' J^T J plus c u u^T of every live bone at the joint, u the unit vector child - parent, c = bone_weight / L^2) and
 * the block -c u u^T per live bone; g likewise (a live bone with |d| = 0 contributes its residual and a zero gradient).
 * (H + lambda diag H) delta = -g is solved on the tree, children eliminated before their parents, without fill-in, each 3x3 block
 * by an unpivoted L D L^T (a pivot that is <= 0 or not finite gives a NaN step, which no trial survives).  A trial is accepted only
 * if it lowers E strictly and leaves every joint that takes part at z_cam > 1e-9 in its views that take part: out_cost <= out_cost0.
 * After a trial, accepted or not: converged when max |delta| <= step_tolerance * z_min, z_min the smallest such depth of the pose
 * at the accepted pose; else capped when lambda > 1e12 or after max_iterations trials.  lambda, the trials and the status belong
 * to the pose.
 * Outputs: out_points (B,J,3); out_error (B,J) the plain weighted RMS of |r_v| in pixels per joint as in mpl_refine_points, NaN for
 * a joint that takes no part; out_bone_error (B,J) = |d| - L in world units at the result, NaN at the root and at a bone that is
 * not live; out_cost0, out_cost (B) = E at the given and the final pose in the mode of the call; out_iterations (B) the trials;
 * out_status (B) bytes:
 *   0 converged;  1 capped (a pose that stays underdetermined, such as one seen by a single camera, may end here);
 *   2 passed through: max_iterations == 0 or no joint takes part; the points are returned bit for bit and everything is scored
 *     (with no joint taking part the costs are 0 and every error is NaN);
 *   3 invalid: a joint that takes part is at z_cam <= 1e-9 in a view that takes part at the given pose; every output of the pose
 *     is NaN.  A statement about the pose: no device error, and no other pose is touched.
 * conf, dist_dev, out_bone_error, out_cost0, out_cost, out_iterations and out_status may be NULL.
 * One launch, one wave per pose, lane j owning joint j; fp64 on the fp32 tensors, every output rounded once, the children of a
 * joint summed in index order, the sums over the pose reduced in a fixed order, no atomics: identical bits from run to run and
 * from batching to batching.  The trial count is bounded by max_iterations whatever the data.  Stream-ordered, never synchronises;
 * neither looks at nor sets the device error word.
 * Refusals, in this order and before any device query: MPL_E_INVALID: limb or parents NULL; then those of mpl_refine_points;
 * MPL_E_INVALID: a limb_stride that is neither 0 nor >= joints; MPL_E_UNSUPPORTED: a bone_weight that is negative or not finite;
 * MPL_E_INVALID: parents that are not one tree (not exactly one -1, an entry that is no other joint, a cycle). */
int mpl_refine_poses(const float *points, const float *pixels, const float *conf, const double *cams_dev, const double *dist_dev,
                     const float *limb, long long limb_stride, const int *parents, int batch, int views, int joints, double huber,
                     double bone_weight, int max_iterations, double step_tolerance, float *out_points, float *out_error,
                     float *out_bone_error, double *out_cost0, double *out_cost, int *out_iterations, unsigned char *out_status,
                     void *stream);

/* ---- temporal smoothing of pose tracks, csrc/smooth_tracks.hip.  Every estimator above works on one frame; this call works along
 * the time axis of a batch in frame order.  points (T,J,3) float32 are the poses of n_segments sequences, frame after frame;
 * segments (host, n_segments ints >= 1 that sum to frames) are their lengths and seg_offsets_dev (device, n_segments + 1 int32) the
 * prefix sums of that list, 0 first and `frames` last.  A track is one joint of one segment; no term crosses a segment boundary.
 * Participation: frame t of a track takes part when its three coordinates are finite and its weight (weight (T,J) float32, NULL:
 * all ones) is finite and > 0, the rule of takes_part; everything else is a gap.
 * Cost, per track, Y the given points, T the segment's length:
 *   E(X) = sum_{t takes part} w_t rho(|X_t - Y_t|^2) + smoothness * sum_t |D^order X|_t^2
 * D^1 X_t = X_t+1 - X_t (t = 0 .. T-2), D^2 X_t = X_t+1 - 2 X_t + X_t-1 (t = 1 .. T-2); rho(s) = s, or with huber = h > 0 (world
 * units, on the 3D distance) s up to h^2 and 2 h sqrt(s) - h^2 beyond; a huber that is <= 0 or not finite is the plain mode.  The
 * three axes share the weights and so one matrix.
 * Plain mode: one solve of (W + smoothness D^T D) X = W Y, status 0, iterations 1, cost0 = cost = E(X).
 * Huber mode: iteratively reweighted least squares.  Solve k+1 is the same system with w'_t = w_t min(1, h / |X^k_t - Y_t|), the
 * first with w' = w; cost0 = E after the first solve.  extent = the largest over the three axes of (max - min of Y over the frames
 * that take part).  After the first solve: converged if extent == 0.  Then, until stopped: capped (1) if `iterations` ==
 * max_iterations; solve; if E did not fall strictly, the earlier iterate is kept and the track has converged (0); else the new
 * iterate is taken, and the track has converged (0) if max_t |X^k+1_t - X^k_t|_inf <= step_tolerance * extent, over all frames.
 * out_cost <= out_cost0 by construction.
 * Passed through (2): max_iterations == 0, or fewer than `order` frames take part (the system is singular).  The points are
 * returned bit for bit, the residual is 0 at frames that take part, both costs are 0 and iterations is 0.
 * Status 3 (LM_INVALID) is never written: every track either has a positive definite system or passes through, and no input
 * value makes a track invalid (a smoothness so large that w + smoothness c rounds the weights away still leaves an SPD band).
 * Outputs, every frame of every track written: out_points (T,J,3) the minimiser, gaps included (a gap is interpolated by the
 * penalty, linearly at order 1 and by a cubic at order 2, and extrapolated by its null space: constant, straight line);
 * out_residual (T,J) = |X_t - Y_t|, NaN at gaps; out_irls (T,J) = min(1, h / |X_t - Y_t|) at the returned points, 1 in the plain
 * mode and where a track passed through, 0 at gaps; out_cost0, out_cost (S,J) float64; out_iterations (S,J) the solves made;
 * out_status (S,J) bytes.  out_points64 (T,J,3) float64, may be NULL: the points before their rounding.
 * Method: one wave (MPL_SMOOTH_LANES lanes) per track, grid (n_segments, joints).  A segment of at most MPL_SMOOTH_SINGLE_MAX
 * frames is solved by one lane (a pentadiagonal L D L^T).  A longer one is cut into blocks of
 * max(MPL_SMOOTH_CHUNK_MIN, ceil(T / MPL_SMOOTH_LANES)) frames, one per lane -- so the block length grows beyond
 * MPL_SMOOTH_CHUNK_MIN * MPL_SMOOTH_LANES frames -- with the last two frames of every block but the last as separators: the lanes
 * factor their interiors, lane 0 solves the Schur complement on the separators in LDS, the lanes back-substitute.  No lane walks
 * a track longer than MPL_SMOOTH_SINGLE_MAX frames.  Factors and iterates always live in the workspace (there is no LDS-resident
 * form, hence no third threshold).  fp64 on the fp32 tensors, every output rounded once, sums in a fixed order, no atomics: the
 * same bits from run to run, and the bits of a track do not depend on what else shares the call.
 * workspace: mpl_smooth_tracks_workspace_bytes(frames, joints, n_segments) device bytes, 8-byte aligned.
 * flags: 0, or MPL_SMOOTH_F_SINGLE_LANE, which sends every track to the one-lane form and exists in -DMPL_LAB builds only
 * (MPL_E_UNSUPPORTED otherwise): the measurement of what the split buys.
 * Stream-ordered, never synchronises; neither looks at nor sets the device error word.  One launch.
 * Refusals, before any launch: MPL_E_INVALID: a NULL pointer (weight and out_points64 excepted), frames outside
 * 1 .. MPL_SMOOTH_MAX_FRAMES, joints outside 1 .. MPL_SMOOTH_MAX_JOINTS, n_segments outside 1 .. frames, a segment outside
 * 1 .. MPL_SMOOTH_MAX_SEGMENT, segments that do not sum to frames, an order other than 1 or 2, an unknown flag;
 * MPL_E_UNSUPPORTED: a smoothness that is not finite and > 0, max_iterations outside 0 .. 1000, a step_tolerance that is negative
 * or not finite; MPL_E_WORKSPACE: workspace NULL, misaligned or too small.  The kernel trusts seg_offsets_dev to be the prefix
 * sums of `segments`; a track whose two offsets do not describe 1 .. MPL_SMOOTH_MAX_SEGMENT frames inside the tensors is left
 * unwritten. */
#define MPL_SMOOTH_LANES 64
#define MPL_SMOOTH_SINGLE_MAX 32        /* up to here one lane solves the track */
#define MPL_SMOOTH_CHUNK_MIN 8          /* the shortest block of a split track: six interior frames and two separators */
#define MPL_SMOOTH_MAX_SEGMENT 65536
#define MPL_SMOOTH_MAX_FRAMES (1 << 24)
#define MPL_SMOOTH_MAX_JOINTS 64
#define MPL_SMOOTH_WS_DOUBLES 18        /* workspace planes per frame and joint: 3 factor, 2 column, 3 right side, 2 x 3 iterate, 4 input */
#define MPL_SMOOTH_F_SINGLE_LANE 1u
size_t mpl_smooth_tracks_workspace_bytes(long long frames, int joints, int n_segments); /* 0 outside the limits */
int mpl_smooth_tracks(const float *points, const float *weight, const int *segments, const int *seg_offsets_dev, int n_segments,
                      long long frames, int joints, double smoothness, int order, double huber, int max_iterations,
                      double step_tolerance, unsigned flags, void *workspace, size_t workspace_bytes, float *out_points,
                      float *out_residual, float *out_irls, double *out_cost0, double *out_cost, int *out_iterations,
                      unsigned char *out_status, double *out_points64, void *stream);

/* ---- Procrustes alignment of predicted poses onto their targets, csrc/procrustes.hip: the transform behind PA-MPJPE (Protocol
 * 2), in place of lib/utils/pose_utils.py:61-143 PoseUtils.procrustes (a numpy port of MATLAB's procrustes, one 3x3 SVD per pose
 * on the host, which would force all_preds back to the host).  One launch aligns `batch` poses: target A and prediction B, both
 * (batch,joints,3); row vectors as in the reference, Z = scale * B @ R + translation.
 * Participation: the joints of `sel` (host array of n_sel ints in [0, joints), at most 64, NULL = all joints in order; an entry
 * listed twice counts twice, as A[sel] would), restricted by `conf` (batch,joints; NULL = all): a joint with conf <= 0 or a
 * non-finite conf does not take part -- the conf_3d <= 0 mask of evaluate().  scale3 / offset3 (host float[3], NULL = identity):
 * the room de-normalisation x * scale + offset, applied to BOTH tensors on load (a per-axis scale is no similarity: it has to
 * happen before the fit); everything below, Z included, is in the de-normalised frame.
 * Per pose, over the joints that take part (:88-109): A_bar, B_bar the means, A0, B0 the centred points, ssX = sum |A0|^2, ssY =
 * sum |B0|^2, M = A0^T B0 / sqrt(ssX ssY) = U diag(s) V^T (s descending), R = V U^T, S = sum s.
 * reflection (:111-119): 0 "best", R as the SVD gives it; 1 forced off: if det R < 0 the last column of V and s[2] change sign;
 * 2 forced on: the same if det R > 0.  scaling != 0 (:122-130): scale = S sqrt(ssX / ssY); scaling == 0 (:131-134): scale = 1.
 * In both, aligned = scale * (B - B_bar) R + A_bar for ALL joints of the pose (taking part or not) and translation = A_bar - scale
 * * B_bar R (:139).  d = sum |Z - A|^2 / ssX over the joints that took part, summed on the points in a second pass: the
 * reference's 1 - S^2 (:127, :133) is the same number and cancels where the fit is good.
 * Outputs: aligned (batch,joints,3), d (batch), rotation (batch,3,3) row-major, scale (batch), translation (batch,3); d,
 * rotation, scale and translation may be NULL, aligned only if d is not.  fp64 arithmetic on the fp32 inputs (the SVD a one-sided
 * Jacobi on M itself), one rounding into the fp32 outputs, no atomics: identical bits from run to run and from batching to batching.
 * Degenerate input is a statement about that pose, not an error: fewer than 3 joints taking part, ssX or ssY zero or not finite,
 * or collinear points (s[1] <= 1e-12 s[0]) make every output of the pose NaN; its neighbours are not affected.
 * The one deviation: coplanar points (s[2] <= 1e-12 s[0]), where numpy's "best" returns whichever sign its SVD happens to
 * produce and both fit equally well; here U and V are completed by cross products and R is the proper rotation (det R = +1).
 * MPL_E_INVALID: pred / target NULL, aligned and d both NULL, a non-positive size, a sel entry outside [0, joints), reflection
 * outside 0..2; MPL_E_UNSUPPORTED: joints > 64, n_sel > 64, batch * joints > 2^30 -- before any launch.  Like the geometry calls
 * it neither looks at nor sets the device error word. */
int mpl_procrustes_align(const float *pred, const float *target, const float *conf, const int *sel, int n_sel,
                         const float *scale3, const float *offset3, int scaling, int reflection, int batch, int joints,
                         float *aligned, float *d, float *rotation, float *scale, float *translation, void *stream);

/* ---- output-side epilogue (the step right after the path): what validate() does on the host
 * with `output.clone().cpu().numpy()` -- room de-normalisation x*scale+offset (function_mpl.py:476-488, host float[3]
 * arrays, NULL = identity) and the MPJPE family: loss.py:39-57 / :110-124 (mean Euclidean error, optional (B,J)
 * weights, per-axis mean |error|, on the RAW tensors) and evaluate.py:91-125 (per-joint absolute and root-relative
 * PJPE with np.nansum semantics, per-axis distances with np.nanmean semantics, on the de-normalised tensors).
 * result (device, mpl_pose_metrics_size(J) floats): [0] loss, [1..3] loss per axis, [4..4+J) pjpe_abs, [4+J] mpjpe_abs,
 * [5+J..5+2J) pjpe_rel, [5+2J] mpjpe_rel, then dist (J x 3), dist_mean (3).  1 <= joints <= 64. */
int mpl_pose_metrics_size(int joints);
int mpl_pose_metrics(const float *output, const float *target, const float *weight, int batch, int joints,
                     const float *scale3, const float *offset3, float *result, void *stream);
/* The same with config.NOT_CONSIDER_SOME_KP_IN_EVAL (evaluate.py:101-104, :110-113): bit j of not_consider_mask set = joint j is
 * deleted from the two MEANS over joints (mpjpe_abs, mpjpe_rel); the per-joint errors are reported unchanged.  The mask has 32 bits:
 * it can name joints 0..31 only, joints 32..63 of a larger skeleton always count. */
int mpl_pose_metrics_ex(const float *output, const float *target, const float *weight, int batch, int joints,
                        const float *scale3, const float *offset3, uint32_t not_consider_mask, float *result, void *stream);

/* ---- device-resident evaluator of a whole validation run (csrc/evaluate.hip; the second half of rank f3): everything
 * validate() does on the host after `model(...)`, accumulated on the device batch by batch and read back once.  Every entry
 * point is stream-ordered and never synchronises; sums are fp64 and folded in a fixed order (bitwise reproducible runs).
 * Replaces, per batch: function_mpl.py:387-399 (criterion, 4 x .item(), AverageMeter weighted by len(input) * batch),
 * :474-494 (D2H copy, room de-normalisation, all_preds / all_gts / all_3d_confs); per run: :612-634 and evaluate() :670-785
 * (OUTPUT_IN_METER factor, relative mode, `conf_3d <= 0` NaN mask, calc_mpjpe / calc_distance_per_dim of evaluate.py:91-125,
 * the per-action breakdown); criteria loss.py:39-57 (MPJPE, LOSS.WEIGHT_AXIS :55-56), :59-104 (L1, MSE), :110-124
 * (Weighted_MPJPE), :127-146 (MPJPE_KADKHODA).
 * State: mpl_eval_state_bytes(n_sel, n_groups) bytes of device memory (0 = shape refused), 8-byte aligned, cleared by
 * mpl_eval_reset.  n_sel = joints of the selection `u` (all_preds[:, u, :], <= 64, entry 0 is the root), n_groups = 1 +
 * caller's classes (group 0 = all samples; <= MPL_EVAL_MAX_GROUPS).
 * mpl_eval_accumulate: one batch.  output/target (B,J,3); x1/x2 (B,J,3) the two intermediate poses of the kadkhod head
 * (MPJPE_KADKHODA only); weight (B,J) (Weighted_MPJPE, MPJPE with weight_axis); conf_3d (B,J) optional, indexed through the
 * selection like the poses; group (B) int32 optional when n_groups == 1: a sample counts in group 0 and, when 1 <= id <
 * n_groups, in its own.  keep_pred/keep_tgt (both or neither): (keep_capacity,J,3) device buffers that receive the batch's
 * de-normalised poses at the run's sample offset (rows beyond the capacity are dropped).  MPJPE with weight_axis follows the
 * broadcast of loss.py:56 ((B,J,1) * (B,J): defined for B == 1, J == 1 or B == J only, MPL_E_INVALID otherwise; B <= 64).
 * While the device's error word is set the batch adds nothing and the state is marked poisoned: every report is NaN.
 * mpl_eval_report: report (device, mpl_eval_report_size doubles): [0] loss, [1..3] loss per axis (AverageMeter.avg),
 * [4] samples fed, [5] poisoned, [6..7] 0; then for pass p (0 absolute, 1 relative) and group g, at 8 + (p * n_groups + g) *
 * (4 * n_sel + 5): pjpe[n_sel], mpjpe, dist[n_sel][3], dist_mean[3], samples of the group (0: the fields are NaN).  Bit k of
 * not_consider_mask deletes SELECTED joint k from mpjpe (np.delete semantics, evaluate.py:101-104); all 64 joints can be named.
 * MPL_E_INVALID: bad arguments; MPL_E_UNSUPPORTED: more than 64 joints or MPL_EVAL_MAX_GROUPS groups -- before any launch. */
#define MPL_EVAL_MAX_GROUPS 32
enum { MPL_CRIT_MPJPE = 0, MPL_CRIT_WEIGHTED_MPJPE = 1, MPL_CRIT_L1 = 2, MPL_CRIT_MSE = 3, MPL_CRIT_MPJPE_KADKHODA = 4 };
typedef struct mpl_eval_options {
    int32_t criterion;       /* MPL_CRIT_* */
    int32_t has_weight_axis; /* LOSS.WEIGHT_AXIS is not None (MPJPE, L1, MSE) */
    float weight_axis[3];
    float scale[3];          /* room de-normalisation x * scale + offset (identity: 1, 0) */
    float offset[3];
    float metre_factor;      /* 100 when DATASET.OUTPUT_IN_METER, else 1 */
    int32_t n_views;         /* len(input): the AverageMeter weight of a batch is n_views * B */
    int32_t n_sel;
    int32_t n_groups;
    uint8_t sel[64];         /* the selection `u`: source joint of selected joint k */
} mpl_eval_options;
size_t mpl_eval_state_bytes(int n_sel, int n_groups);
int mpl_eval_reset(void *state, int n_sel, int n_groups, void *stream);
int mpl_eval_accumulate(void *state, const mpl_eval_options *opt, const float *output, const float *x1, const float *x2,
                        const float *target, const float *weight, const float *conf_3d, const int32_t *group, int batch,
                        int joints, float *keep_pred, float *keep_tgt, long long keep_capacity, void *stream);
int mpl_eval_report_size(int n_sel, int n_groups);
int mpl_eval_report(const void *state, int n_sel, int n_groups, uint64_t not_consider_mask, double *report, void *stream);

/* ---- fp16x2 split-operand engine (csrc/h2_gemm.hip): "fp32" precision of MultiView_MPL (the default).
 * mpl_pack_h2: derived operand of one nn.Linear (W (N,K) row-major, bias (N)), optionally with the LayerNorm in front of it
 * folded in (ln_w, ln_b of length K, or both NULL).  dst: mpl_pack_h2_bytes(N, K) bytes (0 = the shape has no layout:
 * N % 136 == 0, K % 544 == 0 required; with a LayerNorm folded in also K <= 1088: K in {544, 1088}).
 * mpl_ln_linear_h2: y[M,N] = epi(LN?(x) W^T + b) from that operand -- the unit-test entry of one GEMM (the forward runs all
 * GEMMs of a stack in ONE launch, mpl_block_stack); has_ln: x is normalised with eps (stats: 2 * M * K/136 floats of
 * scratch); else x is packed with its measured amax.  workspace: mpl_ln_linear_h2_workspace_bytes(M, K). */
size_t mpl_pack_h2_bytes(int N, int K);
int mpl_pack_h2(const float *W, const float *bias, const float *ln_w, const float *ln_b, int N, int K, uint16_t *dst,
                void *stream);
/* Static activation scales.  A LayerNorm operand stores, per output column n, the power of two so_n that brings the data-free
 * bound of |out_n| (sqrt(K) |gamma o W_n|_2 + |bias_n + beta . W_n|) to the top of the fp16 window; the GEMM epilogue that hands
 * column n on as a packed operand (attention output: a convex combination of v rows; GELU output: |gelu(t)| <= |t|) multiplies
 * by so_n.  mpl_pack_h2_out_scale returns the DEVICE address of so[N] inside such an operand.  The Linear that consumes those
 * columns (proj after qkv's v columns, fc2 after fc1: multiview_mpl.py:65, :35) is packed with mpl_pack_h2_scaled: W_nk is stored
 * as W_nk / in_scale_k (exact), so operands are equilibrated per channel and one outlier channel costs no other channel
 * resolution.  in_scale: K powers of two on the device. */
int mpl_pack_h2_scaled(const float *W, const float *bias, const float *in_scale, int N, int K, uint16_t *dst, void *stream);
const float *mpl_pack_h2_out_scale(const uint16_t *operand, int N, int K);
size_t mpl_ln_linear_h2_workspace_bytes(int M, int K);
int mpl_ln_linear_h2(const float *x, int M, int K, int has_ln, float eps, const uint16_t *W2, int N, int epilogue,
                     const float *residual, float *y, float *stats, void *workspace, size_t workspace_bytes, void *stream);

/* ---- device-side failures.  The block stack runs as ONE persistent launch whose workgroups hand operands to each
 * other (h2_phase.hpp); it needs all its workgroups resident, i.e. the device to itself for the duration of the launch
 * (single tenant: launches of this library on different streams of one process are serialised by the library, other
 * processes on the same GPU are not).  A workgroup whose wait for a partner runs out (~10 s) never goes on with stale
 * operands: it sets a sticky per-device error word, the poses of that call are NaN, and EVERY later call on the device
 * returns MPL_E_DEVICE until mpl_device_error_clear() -- the reference's convention for a failed forward is a Python
 * exception (SURVEY.md 8b "Error convention"), which is what the binding turns this into.
 * mpl_device_error(dev): the word, 0 = no failure (dev < 0: the current device); no synchronisation, reads pinned memory.  Values:
 *   1 (bit 0) = lost hand-off / operands packed against other scales (above);
 *   2 (bit 1) = the split-operand SPT engine met a confidence-weighted attention row (confidence_as_attention_uncertainty_weight,
 *       reference multiview_mpl.py:61-62: the softmax rows are multiplied by the caller's `conf`, which is DATA) beyond the
 *       fp16 window its static scales assume: that sequence's poses are NaN -- never a saturated, plausible-looking pose --
 *       and the caller is pointed at the native-fp32 engine (MPL precision "fp32_mfma"), which has no window.
 *       Only a FINITE row beyond the window is reported.  A NaN or infinite keypoint or confidence (a missing detection) is
 *       the caller's data: the reference answers it with NaN poses for that sample, so does every engine here -- that
 *       sample NaN in every element, every other sample of the batch bit for bit what it is without it -- and the word
 *       stays 0 (tests/test_nonfinite_gpu.py).
 * mpl_x3_spin_limit(v): test hook.  v & 0xff = log2 of the polls before a wait counts as lost (default 23 ~ 10 s);
 * v >> 8 = fault injection: when > 0, one workgroup of the next launches deserts its team before that GEMM phase, so
 * that the failure path can be exercised deterministically (tests/test_failures_gpu.py). */
int mpl_device_error(int device);
int mpl_device_error_clear(int device);
int mpl_x3_spin_limit(int log2_polls);

/* Measurement aid (bench.py roofline leg): between start and stop every kernel launched by this
 * library on ANY stream is bracketed by a hipEvent pair recorded on that same stream.  stop()
 * synchronises the events and returns, per kernel kind, the summed device time (ms) and the launch
 * count.  Process-global and not thread safe; never enabled on the product path. */
#define MPL_K_SPT 0
#define MPL_K_ROW_STATS 1
#define MPL_K_GEMM 2
#define MPL_K_ATTENTION 3
#define MPL_K_FUSE_HEAD 4
#define MPL_K_PACK 5 /* derived-operand builders: mpl_pack_h2*, mpl_spt_pack, mpl_d32_pack, mpl_pack_bf16(_any) */
#define MPL_K_COUNT 6
int mpl_profile_start(void);
int mpl_profile_stop(float *kind_ms, int *kind_launches, int n_kinds);

#ifdef __cplusplus
}
#endif
#endif /* MPL_HIP_H_ */

/*
 * lamp_hip.h -- C ABI of liblamp_hip.so, the MI355X (gfx950) native library behind the
 * LaMP label-graph message-passing forward path.
 *
 * The reference (QData/LaMP) is pure Python on PyTorch: it owns no native code and no FFI.  The
 * "FFI for this path" is therefore the set of nn.Module.forward methods on the path; each entry
 * point below replaces one of them and cites it (paths relative to the reference root).  The
 * Python side (lamp_amd/_native.py) binds these with ctypes and raw data_ptr()s; INTEGRATION.md
 * shows the stub.
 *
 * Conventions
 *   - plain C99 types only; no torch / HIP types in signatures (a stream is a void* holding a
 *     hipStream_t; NULL = the default stream).
 *   - all tensors are fp32, row-major, device-resident; indices are int64; masks are uint8.
 *   - mask convention everywhere (as in the reference): NONZERO = BLOCKED.
 *   - the caller owns every byte: inputs, outputs, weights, workspace.  The library never
 *     allocates or frees device memory and keeps no pointer after return.
 *   - every call only enqueues work on `stream` (asynchronous w.r.t. the host) and is re-entrant and
 *     thread-safe for distinct streams / devices (one host thread per device, as nn.DataParallel runs
 *     its replicas, works); the device is the one current for the calling thread.
 *   - no library state that results depend on: the process-wide data are lazily initialised, immutable per-device
 *     kernel attributes, one atomic launch counter (the tag of lamp_forward's plan hand-off granules: it only has
 *     to differ from launch to launch) and -- for diagnostics, mutex-protected -- the lamp_prof_* event records.
 *   - return value: 0 = ok, > 0 = a hipError_t from a launch, < 0 = lamp_status below.  Nothing
 *     throws or aborts across the boundary.  NaN produced by fully masked attention rows is data,
 *     not an error (reference behaviour).
 */
#ifndef LAMP_HIP_H
#define LAMP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the entry points declared here are its ONLY dynamic symbols. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define LAMP_HIP_ABI_VERSION 5   /* 5: lamp_model grows (enc0_emb_w1 / enc0_pos_w1, label_csr); 4: + lamp_gemm_grouped, lamp_{ffn,mha}_train_fwd / _bwd */

typedef void* lamp_stream_t; /* hipStream_t */

enum lamp_status {
    LAMP_OK = 0,
    LAMP_E_DIMS = -1,        /* non-positive or inconsistent dimensions */
    LAMP_E_ALIGN = -2,       /* pointer / leading dimension not 16-byte aligned where required */
    LAMP_E_WORKSPACE = -3,   /* workspace too small */
    LAMP_E_UNSUPPORTED = -4, /* valid request this build has no kernel for (e.g. d_k not a multiple of 4) */
    LAMP_E_NULL = -5         /* required pointer is NULL */
};

/* Attention mask descriptor.  One code path covers the reference's three mask uses:
 *   key padding  (lamp/utils.py:26-34)      : U8, stride_q = 0, stride_b = lk      [B, lk]
 *                                             or KEY_TOKENS_I64 straight from src_seq
 *   label graph  (lamp/Decoders.py:109-116) : U8, stride_b = 0, stride_q = lk      [lq, lk]
 *   arbitrary    (module-level callers)     : U8, stride_b = lq*lk, stride_q = lk  [B, lq, lk]
 * The same mask is applied to every head (lamp/SubLayers.py:102 repeats it n_head times). */
enum lamp_mask_kind {
    LAMP_MASK_NONE = 0,
    LAMP_MASK_U8 = 1,            /* uint8, nonzero = blocked; element (b,q,k) at ptr[b*stride_b + q*stride_q + k] */
    LAMP_MASK_KEY_TOKENS_I64 = 2, /* int64 token ids [B, stride_b]; key k of sample b is blocked iff token == 0 (PAD) */
    LAMP_MASK_BITS_U32 = 3,       /* bit-packed rows: uint32 words, element (b,q,k) = bit (k & 31) of word
                                     ptr[b*stride_b + q*stride_q + (k >> 5)] (strides in words), 1 = blocked; bits
                                     past lk are ignored.  One 4-byte load covers a whole 32-key tile of a row. */
    LAMP_MASK_BIAS_F32 = 4        /* not a mask but an additive fp32 score bias (the weighted label graph): element (b,q,k) at
                                     ptr[b*stride_b + q*stride_q + k] (strides in floats) is added to the scaled score before
                                     the softmax, S = <q, k> / temperature + bias; -inf = blocked, exactly as a masked entry (a
                                     row of -inf comes out NaN, only that row); +inf and NaN are the caller's error.  stride_b
                                     == 0: shared over the batch; heads always share it.  softmax(s + log w) = w exp(s) / sum w
                                     exp(s): a bias of log w re-weights the attention by w.  A constant to the backward
                                     entries, which take no bias (dS = softmax backward of the saved map); a caller that trains
                                     the bias reduces that dS itself (lamp_attn_bias_bwd).  ptr 16-byte
                                     aligned, stride_q % 4 == 0 and stride_b % 4 == 0 (a lane fetches its four consecutive keys
                                     with one 16-byte load; every row is readable up to the next multiple of 4 floats), else
                                     LAMP_E_ALIGN.  Served by every entry that takes a lamp_mask (csrc/attention_bias.hip;
                                     d_k or d_v > 128: the general kernel), in all three output modes.  LAMP_E_UNSUPPORTED,
                                     before any launch: act == LAMP_ATTN_SIGMOID, a tile_list, LAMP_MASK_SPARSE_ROWS,
                                     LAMP_MASK_SELF_RAGGED, or packed K / V with per-sample key counts (which only a key-token
                                     mask brings today, so no entry can combine the two). */
};

/* lamp_mask.flags */
#define LAMP_MASK_SPARSE_ROWS 1  /* a SHARED bit-packed mask (kind BITS_U32, stride_b == 0) whose rows allow only a small fraction
                                    of the keys, with no block structure to skip (an unstructured label graph): the library may
                                    compute the allowed (query, key) pairs only (csrc/attention_sparse.hip) instead of visiting every
                                    key tile.  Set by the caller from the mask's density (lamp_amd/Decoders.py); exact either way. */

#define LAMP_MASK_SELF_RAGGED 2  /* the call is a self-attention over ragged rows padded to a common length (the live encoder,
                                    lamp_fwd_options): queries are padded as far as keys, so lq says nothing about the sample.
                                    The kernel is then chosen without looking at lq or lk (always csrc/attention_small.hip, whose
                                    key split follows each sample's own key count; one share when the mask brings no key counts):
                                    a sample's bits do not depend on how far its batch was padded.  Heads wider than 128
                                    (d_k or d_v > 128) run the general kernel whatever the flag says: the guarantee ends there. */

typedef struct lamp_mask {
    int32_t kind;
    int32_t flags;               /* LAMP_MASK_SPARSE_ROWS | LAMP_MASK_SELF_RAGGED, or 0 */
    const void* ptr;
    int64_t stride_b;
    int64_t stride_q;
    /* Optional sparsity hint for a SHARED mask (stride_b == 0): for every block of 32 query rows, the list of
     * 32-key tiles that contain at least one unblocked entry -- int32 rows of length tile_list_stride:
     * [count, tile_0, tile_1, ...] in ascending order.  Tiles not listed are skipped entirely (exact: their
     * probabilities are 0).  NULL = visit every tile.  Ignored when attention maps are written.  This is the
     * label graph's block structure (lamp/Decoders.py:109-113) handed to the kernel once per model. */
    const int32_t* tile_list;
    int64_t tile_list_stride;
    int64_t allowed_pairs;       /* with LAMP_MASK_SPARSE_ROWS: number of unblocked (query, key) entries of the shared mask (the
                                    work the pair kernel executes: lamp_prof_* counts 2 * allowed_pairs * (d_k + d_v) FLOP per
                                    (sample, head) for it); 0 = unknown */
} lamp_mask;

/* Element strides of the four attention operands, so that one kernel serves both the
 * reference's head-major (h*B, l, d_k) batches (lamp/SubLayers.py:96-98) and the fused
 * [B, l, h*d_k] projections written by lamp_mha_fwd without any permute copy. */
typedef struct lamp_attn_layout {
    int64_t q_b, q_h, q_r;
    int64_t k_b, k_h, k_r;
    int64_t v_b, v_h, v_r;
    int64_t o_b, o_h, o_r;
} lamp_attn_layout;

/* Weights of one MultiHeadAttention (lamp/SubLayers.py:46-74), in nn.Linear's native [out, in] layout. */
typedef struct lamp_mha_weights {
    const float* w_qs; /* [n_head*d_k, d_model] */
    const float* w_ks; /* [n_head*d_k, d_model] */
    const float* w_vs; /* [n_head*d_v, d_model] */
    const float* fc;   /* [d_model, n_head*d_v]; NULL when n_head == 1 (lamp/SubLayers.py:72-74) */
    const float* ln_g; /* [d_model] */
    const float* ln_b; /* [d_model] */
    int32_t n_head;
    int32_t present;   /* 0 = this attention block does not exist (no_dec_self_att) */
} lamp_mha_weights;

/* Weights of one PositionwiseFeedForward (lamp/SubLayers.py:125-131); Conv1d(k=1) weights
 * [out, in, 1] are read as [out, in]. */
typedef struct lamp_ffn_weights {
    const float* w1;   /* [d_inner, d_model] */
    const float* b1;   /* [d_inner] */
    const float* w2;   /* [d_model, d_inner] */
    const float* b2;   /* [d_model] */
    const float* ln_g; /* [d_model] */
    const float* ln_b; /* [d_model] */
} lamp_ffn_weights;

typedef struct lamp_enc_layer {  /* lamp/Layers.py:9-20 */
    lamp_mha_weights slf_attn;   /* dead compute unless attention maps are requested */
    lamp_ffn_weights pos_ffn;
} lamp_enc_layer;

typedef struct lamp_dec_layer {  /* lamp/Layers.py:22-48 */
    lamp_mha_weights enc_attn;
    lamp_ffn_weights pos_ffn1;
    lamp_mha_weights slf_attn;   /* .present == 0 under no_dec_self_att */
    lamp_ffn_weights pos_ffn2;
} lamp_dec_layer;

/* Optional, weights-only: the three weight matrices of one decoder sub-chain -- the attention's output projection `fc`
 * (lamp/SubLayers.py:110) and the feed-forward block's w_1 / w_2 that follows it (lamp/SubLayers.py:133-142) -- rearranged
 * by lamp_pack_weight into the order the fused chain launch streams them.  Like dec0_query below they depend on weights
 * only: a caller may build them once per weight version.  Results are bit-identical with and without them. */
typedef struct lamp_chain_pack {
    const float* fc;  /* lamp_pack_weight(fc [d_model, n_head*d_v], format 0) */
    const float* w1;  /* lamp_pack_weight(w_1 [d_inner, d_model], format 0) */
    const float* w2;  /* lamp_pack_weight(w_2 [d_model, d_inner], format 0) */
    const float* fc4; /* the same three in format 1 (panels of 4 / 8 / 12 rows: batches whose B * n_labels rows would */
    const float* w14; /* leave CUs without a sixteen-row panel); either trio may be NULL */
    const float* w24;
} lamp_chain_pack;

/* The whole graph-encoder / graph-decoder model (lamp/Models.py:18-94).  Host-side struct of
 * device pointers; enc_layers / dec_layers are host arrays. */
typedef struct lamp_model {
    int32_t n_src_vocab, n_position, n_labels;
    int32_t d_model, d_inner, d_k, d_v;
    int32_t n_layers_enc, n_layers_dec;
    int32_t label_mask_flags;   /* lamp_mask.flags of the label graph (LAMP_MASK_SPARSE_ROWS), 0 otherwise */
    const float* src_word_emb;  /* [n_src_vocab, d_model]  encoder.src_word_emb.weight */
    const float* position_enc;  /* [n_position, d_model] or NULL (no_enc_pos_embedding) */
    const float* tgt_word_emb;  /* [n_labels, d_model]     decoder.tgt_word_emb.weight */
    const float* w_out;         /* [n_labels, d_model]     tgt_word_proj.linear.weight */
    const uint8_t* label_mask;  /* [n_labels, n_labels] nonzero = blocked, or NULL ('none').  Under LAMP_FWD_LABEL_BIAS
                                   (lamp_fwd_options.flags): a const float* score bias instead, see there */
    const uint32_t* label_mask_bits; /* optional bit-packed copy of label_mask (LAMP_MASK_BITS_U32 rows of
                                        ceil(n_labels/32) words); used instead of the byte mask when given */
    const int32_t* label_tiles; /* optional active-tile list of label_mask (see lamp_mask.tile_list), row stride
                                   ceil(n_labels/32) + 1; NULL = dense */
    const lamp_enc_layer* enc_layers;
    const lamp_dec_layer* dec_layers;
    /* Optional: decoder layer 0's enc-attention query, tgt_word_emb . w_qs^T  [n_labels, n_head*d_k].  It
     * depends on weights only (the decoder input is the label table for every sample, lamp/Decoders.py:
     * 132-134), so a caller may compute it once per weight version (lamp_linear_fwd) and
     * pass it here; NULL = lamp_forward projects it on every call. */
    const float* dec0_query;
    /* Optional: host array of 2 * n_layers_dec packs -- entry 2 i: layer i's (enc_attn.fc, pos_ffn1), entry 2 i + 1: its
     * (slf_attn.fc, pos_ffn2); entries with NULL members, or a NULL array, leave that sub-chain on the native layouts. */
    const lamp_chain_pack* chain_packs;
    /* Optional (both or neither; ABI 5): encoder layer 0's first FFN matrix folded into the embedding tables.  The token /
     * position gather of lamp/Encoders.py:66,75 is a one-hot product, so relu((Emb[tok] + Pos[p]) W1^T + b1) of
     * lamp/SubLayers.py:135 equals relu(enc0_emb_w1[tok] + enc0_pos_w1[p]) with the weights-only tables
     *   enc0_emb_w1 [n_src_vocab, d_inner] = src_word_emb . W1^T            (+ b1 when position_enc is NULL)
     *   enc0_pos_w1 [n_position, d_inner]  = position_enc . W1^T + b1       (NULL when position_enc is NULL)
     * of enc_layers[0].pos_ffn (a caller builds them once per weight version with lamp_linear_fwd).  lamp_forward then
     * gathers that layer's hidden rows beside the embedded rows and does not launch its first GEMM: a re-association, so
     * results differ from the unfolded route in the last bits (not bit-identical, well inside 1e-4).  NULL = unfolded. */
    const float* enc0_emb_w1;
    const float* enc0_pos_w1;
    int64_t label_mask_allowed; /* lamp_mask.allowed_pairs of the label graph (with LAMP_MASK_SPARSE_ROWS), else 0 */
} lamp_model;

/* Optional extra outputs of lamp_forward (return_attns / int_preds, lamp/Models.py:127-135).
 * Any pointer (or the whole struct) may be NULL.  Attention maps are (n_head*B, lq, lk) with
 * index head*B + b, exactly the reference's layout. */
typedef struct lamp_aux {
    float* const* enc_self_attn; /* n_layers_enc pointers, each (h*B, T, T) */
    float* const* dec_self_attn; /* n_layers_dec pointers, each (h2*B, L, L) */
    float* const* dec_enc_attn;  /* n_layers_dec pointers, each (h*B, L, T) */
    float* const* int_preds;     /* lamp/Models.py:128-133: one (B, L) per intermediate output but the last */
    int32_t n_int_preds;
    int32_t reserved;
} lamp_aux;

/* ---- library ------------------------------------------------------------------------------ */
int lamp_version(void);                 /* LAMP_HIP_ABI_VERSION the library was built with */
const char* lamp_strerror(int status);  /* text for lamp_status / hipError_t values */

/* ---- building blocks ---------------------------------------------------------------------- */

/* nn.Linear / XavierLinear / Conv1d(k=1) (lamp/SubLayers.py:7-13, 91-93, 110, 127-128):
 *   C[M,N] = act(A[M,K] . W[N,K]^T + bias[N]) + residual[M,N]      (bias, residual may be NULL)
 * lda/ldw/ldc/ldr are leading dimensions in elements; K, lda, ldw must be multiples of 4.
 * Limits (this entry, lamp_linear_prec_fwd and lamp_linear_packed_fwd): M is 64-bit and A, residual and C may be of any
 * size; inside one tile the byte offsets are 32-bit: max(lda, ldw, ldc) * max(BM, BN) * 4 < 0x7fffffff and ldr * BM * 4 < 0x7fffffff for
 * the tile the launch picks (BM, BN <= 128: every leading dimension up to 4194300 is served by every tile), else LAMP_E_UNSUPPORTED. */
int lamp_linear_fwd(const float* A, int64_t M, int32_t K, int64_t lda,
                    const float* W, int32_t N, int64_t ldw, const float* bias,
                    const float* residual, int64_t ldr, int32_t relu,
                    float* C, int64_t ldc, lamp_stream_t stream);

/* lamp_linear_fwd at a chosen matmul precision.  gfx950 has no TF32 and its fp32 matrix pipe runs at 1/16 of the bf16 one, so the
 * "treat each float32 as the sum of three bfloat16 numbers" of torch.set_float32_matmul_precision('high') is the one reduced
 * precision this chip offers an fp32 GEMM (csrc/gemm_split.hip).  Operands and result stay fp32 in memory; each operand tile is
 * split on the fly into h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), and per 32-wide k-chunk the products are summed in fp32,
 * smallest first, in a fixed order:
 *   LAMP_PREC_FP32    lamp_linear_fwd, bit for bit
 *   LAMP_PREC_BF16X3  a_m w_h + a_h w_m + a_h w_h                                   (|error| <= 2^-14 sum_k |a_k w_k| at K <= 512)
 *   LAMP_PREC_BF16X6  a_l w_h + a_h w_l + a_m w_m + a_m w_h + a_h w_m + a_h w_h     (fp32-class error)
 * Any other value: LAMP_E_UNSUPPORTED.  Same shapes as lamp_linear_fwd (no shape falls back to the fp32 kernel).  An output
 * element's bits depend on (K, precision) only -- never on M, N, the tile or the grid -- and rows are independent.  The one
 * semantic deviation: an inf operand gives NaN (inf - inf in the split) where fp32 arithmetic gives inf. */
#define LAMP_PREC_FP32 0
#define LAMP_PREC_BF16X3 1
#define LAMP_PREC_BF16X6 2
int lamp_linear_prec_fwd(const float* A, int64_t M, int32_t K, int64_t lda,
                         const float* W, int32_t N, int64_t ldw, const float* bias,
                         const float* residual, int64_t ldr, int32_t relu,
                         float* C, int64_t ldc, int32_t precision, lamp_stream_t stream);

/* lamp_linear_fwd for 1 <= n_seg <= 4 weight matrices W[s] [N, K] that share A, one launch: C[s] = act(A . W[s]^T + bias[s]) (+ residual;
 * meaningful with one segment), bit for bit what n_seg calls of lamp_linear_fwd give.  W, C: host arrays of n_seg device pointers;
 * bias: such an array with nullable entries, or NULL.
 *   W_pack (nullable; host array of n_seg nullable entries): lamp_pack_weight(W[s], N, K, ldw, format 0).  When every segment has
 *     one, N % 16 == 0, K % 32 == 0 and C / bias / residual can move as 16-byte accesses, the launch loads its weight fragments
 *     straight from the packs wherever launch_gemm picks a one-wave-row tile (csrc/gemm.hip, the packed-W tiles: by tile counts);
 *     otherwise the packs are ignored.
 *     Same bits either way.
 *   m_dev (nullable): the live row count in device memory; rows at and past min(*m_dev, M) are neither computed nor written
 *     (M then only sizes the launch).
 * A pack is read through one 31-bit descriptor: with (N + 64) * K * 4 >= 0x7fffffff the packs are ignored (same bits). */
int lamp_linear_packed_fwd(const float* A, int64_t M, int32_t K, int64_t lda, const float* const* W, const float* const* W_pack,
                           int32_t n_seg, int32_t N, int64_t ldw, const float* const* bias, const float* residual, int64_t ldr,
                           int32_t relu, float* const* C, int64_t ldc, const int32_t* m_dev, lamp_stream_t stream);

/* nn.LayerNorm over the last dim, biased variance, eps inside the sqrt (lamp/SubLayers.py:68,130).
 * y may alias x.  d must be a multiple of 4, d <= 4096.  Rows are indexed in 64 bits (M * d may pass 2^31 elements); one wave per
 * row, four rows per workgroup: (M + 3) / 4 > 0x7fffffff is LAMP_E_DIMS (so for every row kernel below that takes a row count). */
int lamp_layernorm_fwd(const float* x, int64_t M, int32_t d, const float* gamma, const float* beta,
                       float eps, float* y, lamp_stream_t stream);

/* ScaledDotProductAttention.forward (lamp/SubLayers.py:27-43), eval mode:
 *   S = (Q K^T) * inv_temperature ; S[blocked] = -inf ; P = softmax_k(S) ; O = P V
 * for B samples x H heads.  `attn` (nullable) receives P as (H*B, lq, lk), index head*B + b.
 * A fully blocked row yields NaN in O and P, as in the reference.  d_k, d_v multiples of 4; up to 128 the fused
 * single-kernel path runs, beyond that a general three-launch path (S = QK^T, masked softmax, PV) that keeps its
 * scores in `attn` -- which must then be given (LAMP_E_WORKSPACE otherwise).
 * Limits (every lamp_sdpa_* / lamp_mha_* entry): B * H and with them Q, K, V, out and attn may be of any size (slice offsets are 64-bit);
 * inside ONE (sample, head) slice the byte offsets are 32-bit: lq * q_r * 4, lk * k_r * 4, lk * v_r * 4, lq * stride_q + lk bytes of a
 * u8 mask (x 4 for bit-packed words) and (lq * stride_q + lk + 3) * 4 of a bias must each stay below 0x7fffffff, else LAMP_E_UNSUPPORTED. */
int lamp_sdpa_fwd(const float* q, const float* k, const float* v, float* out, float* attn,
                  int32_t B, int32_t H, int32_t lq, int32_t lk, int32_t d_k, int32_t d_v,
                  float inv_temperature, const lamp_mask* mask, const lamp_attn_layout* layout,
                  lamp_stream_t stream);

/* Same outputs as lamp_sdpa_fwd with attn != NULL, at the speed of the map-less kernel: one pass over the keys writes
 * the scaled scores into `attn` and every row's log2-sum-exp into `lse` [(H*B) * lq] (caller-provided, also an
 * output), then `attn` is normalised in place by a second launch.  The maps agree with lamp_sdpa_fwd's exact
 * two-pass softmax to rounding; a fully blocked row is NaN in both.  The training forward uses this (the maps are
 * the backward pass's input); a mask's tile list is ignored (every tile is visited).
 * `lse`, index (head*B + b) * lq + q: log2 of the row's sum of exp(scaled, masked score), i.e. logsumexp / ln 2, so that
 * attn = exp2(score * log2(e) - lse).  A fully blocked row (every key masked, or a sample whose keys are all padding) has an
 * empty sum: its lse is -inf (log2f(0), no NaN), and exp2(-inf - -inf) is what makes its map row NaN.  Both kernels the call
 * can reach write it so (tests/test_attention_train_routes_gpu.py pins the value). */
int lamp_sdpa_fwd_fast_maps(const float* q, const float* k, const float* v, float* out, float* attn, float* lse,
                            int32_t B, int32_t H, int32_t lq, int32_t lk, int32_t d_k, int32_t d_v,
                            float inv_temperature, const lamp_mask* mask, const lamp_attn_layout* layout,
                            lamp_stream_t stream);

/* The activation of an attention block (the reference's attn_type, lamp/SubLayers.py:17-25, config_args.py:49). */
#define LAMP_ATTN_SOFTMAX 0
#define LAMP_ATTN_SIGMOID 1

/* lamp_sdpa_fwd with the activation as an argument.  act == LAMP_ATTN_SOFTMAX: lamp_sdpa_fwd itself, bit for bit.
 * act == LAMP_ATTN_SIGMOID -- ScaledDotProductAttention(attn_type='sigmoid'), lamp/SubLayers.py:17-25,39:
 *   S = (Q K^T) * inv_temperature ; P = sigmoid(S), P[blocked] = sigmoid(-inf) = 0 exactly ; O = P V
 * There is no row normalisation: a fully blocked row is 0 in O and P, not NaN.  `attn` (nullable) receives P in the same
 * single pass; out and v may both be NULL with attn given (maps only).  d_k, d_v multiples of 4 (else LAMP_E_UNSUPPORTED); up
 * to 128 one fused kernel serves every shape, beyond that the general three-launch path with the scores in `attn` (required
 * then).  Any other act: LAMP_E_UNSUPPORTED. */
int lamp_sdpa_act_fwd(const float* q, const float* k, const float* v, float* out, float* attn,
                      int32_t B, int32_t H, int32_t lq, int32_t lk, int32_t d_k, int32_t d_v,
                      float inv_temperature, int32_t act, const lamp_mask* mask, const lamp_attn_layout* layout,
                      lamp_stream_t stream);

/* lamp_mha_fwd with the activation of its attention as an argument (MultiHeadAttention(attn_type=...), lamp/SubLayers.py:
 * 65-75): act == LAMP_ATTN_SOFTMAX is lamp_mha_fwd, bit for bit; LAMP_ATTN_SIGMOID computes P = sigmoid(S) with blocked
 * entries exactly 0 (a fully blocked row contributes 0, not NaN) as lamp_sdpa_act_fwd does.  Same workspace. */
int lamp_mha_act_fwd(const float* xq, const float* xkv, int32_t B, int32_t lq, int32_t lk,
                     int32_t d_model, int32_t d_k, int32_t d_v, const lamp_mha_weights* w, int32_t act,
                     const lamp_mask* mask, float* out, float* attn,
                     void* workspace, size_t workspace_bytes, lamp_stream_t stream);

/* MultiHeadAttention.forward (lamp/SubLayers.py:77-121), eval mode:
 *   out = LayerNorm( concat_heads(SDPA(xq Wq^T, xkv Wk^T, xkv Wv^T)) Wfc^T + xq )
 * xq [B, lq, d_model], xkv [B, lk, d_model] (may alias xq), out [B, lq, d_model];
 * attn nullable (n_head*B, lq, lk).  Workspace: lamp_mha_workspace_bytes(). */
size_t lamp_mha_workspace_bytes(int32_t B, int32_t lq, int32_t lk, int32_t d_model, int32_t n_head,
                                int32_t d_k, int32_t d_v);
int lamp_mha_fwd(const float* xq, const float* xkv, int32_t B, int32_t lq, int32_t lk,
                 int32_t d_model, int32_t d_k, int32_t d_v, const lamp_mha_weights* w,
                 const lamp_mask* mask, float* out, float* attn,
                 void* workspace, size_t workspace_bytes, lamp_stream_t stream);

/* PositionwiseFeedForward.forward (lamp/SubLayers.py:133-142), eval mode:
 *   out = LayerNorm( relu(x W1^T + b1) W2^T + b2 + x ),  x/out [M, d_model] (out may alias x).
 * Workspace: M * d_inner floats. */
size_t lamp_ffn_workspace_bytes(int64_t M, int32_t d_model, int32_t d_inner);
int lamp_ffn_fwd(const float* x, int64_t M, int32_t d_model, int32_t d_inner,
                 const lamp_ffn_weights* w, float* out,
                 void* workspace, size_t workspace_bytes, lamp_stream_t stream);

/* GraphEncoder's input stage (lamp/Encoders.py:66,75): out[t,:] = emb[src_seq[t],:] (+ pos[src_pos[t],:]).
 * An index outside its table writes NaN into that row (PyTorch would raise; a kernel cannot).  n_tokens * d_model may pass 2^32 bytes
 * (64-bit row offsets; lamp_embed_bwd and lamp_embed_bwd_ordered likewise); (n_tokens + 3) / 4 > 0x7fffffff is LAMP_E_DIMS. */
int lamp_embed_fwd(const int64_t* src_seq, const int64_t* src_pos, int64_t n_tokens,
                   const float* emb, int32_t n_vocab, const float* pos_table, int32_t n_position,
                   int32_t d_model, float* out, lamp_stream_t stream);

/* Label read-out (lamp/Models.py:124-126): logits[b,i] = <y[b,i,:], w_out[i,:]>, i.e. the diagonal
 * of y . w_out^T without forming the (B, L, L) product.  B * L * d_model may pass 2^32 bytes (64-bit row offsets);
 * (B * L + 3) / 4 > 0x7fffffff is LAMP_E_DIMS. */
int lamp_diag_logits_fwd(const float* y, const float* w_out, int32_t B, int32_t L, int32_t d_model,
                         float* logits, lamp_stream_t stream);

/* Post-processing of the evaluation loop (test.py:49-51), the step right after the hot path:
 *   probs[b,i]  = sigmoid(logits[b,i])                                   (probs nullable)
 *   row_loss[b] = sum_i  max(x,0) - x*z + log1p(exp(-|x|)),  x = logits[b,i], z = targets[b,i]
 * i.e. F.binary_cross_entropy_with_logits summed per row (row_loss and targets nullable together);
 * the 'mean' reduction is sum(row_loss) / (n_rows * L). */
int lamp_sigmoid_bce_fwd(const float* logits, const float* targets, int64_t n_rows, int32_t L,
                         float* probs, float* row_loss, lamp_stream_t stream);

/* Prior label graph, the input of label_mask='prior' (utils/data_loader.py:37-47), built on the device from
 * the train split's label sets in CSR form: label_ids[offsets[s] .. offsets[s+1]) are the 0-based label
 * indices of sample s (target-vocabulary ids minus the 4 special tokens, BOS/EOS stripped).
 *   adj     [L, L] float: 1 where i == j or labels i and j share a sample, else 0  (the reference's matrix)
 *   blocked [L, L] u8, nullable: the decoder self-attention mask derived from it (lamp/Decoders.py:105-113;
 *           no row of adj is empty because of the diagonal), 1 = blocked = (adj == 0).
 * Ids outside [0, L) are skipped (the reference would index out of range); validate on the host. */
int lamp_prior_graph_build(const int64_t* label_ids, const int64_t* offsets, int64_t n_samples, int32_t L,
                           float* adj, uint8_t* blocked, lamp_stream_t stream);

/* Weights-only repack for lamp_model.chain_packs: W [N, K] (leading dimension ldw; nn.Linear / Conv1d(k=1) layout) ->
 * packed [N * K] floats in the order a chain kernel streams them (exact copy of the values, no arithmetic):
 *   format 0: per block of 16 output rows and 32 k the 16x16x4 MFMA fragments lane by lane (N % 16 == 0, K % 32 == 0);
 *   format 1: per block of 64 output rows and 16 k, four k per row and load (N % 64 == 0, K % 16 == 0).
 * 16-byte aligned pointers. */
int lamp_pack_weight(const float* W, int32_t N, int32_t K, int64_t ldw, int32_t format, float* packed, lamp_stream_t stream);

/* ---- backward-pass building blocks (training through train.py:36-48) ------------------- */

/* General strided, batched GEMM:   C_z[m, n] (+)= alpha * sum_k A_z(m, k) * B_z(n, k),   z = (z0, z1),
 *   A_z(m, k) = A[z0*a_batch0 + z1*a_batch1 + m*a_row_stride + k*a_col_stride]   (B likewise with n),
 *   C_z[m, n] = C[z0*c_batch0 + z1*c_batch1 + m*ldc + n].
 * For each operand one of (row_stride, col_stride) must be 1, which covers every product of the backward pass
 * without a transpose copy: dX = dY.W, dW = dY^T.X, dP = dO.V^T, dV = P^T.dO, dQ = dS.K, dK = dS^T.Q.
 * relu_mask (batch 1 only, nullable): result elements whose mask value is not > 0 are zeroed (ReLU backward).
 * accumulate != 0 adds to C.  Workspace (nullable): lamp_gemm_workspace_bytes() lets deep-K / small-output
 * products (weight gradients) split K deterministically.
 * Limits: the batch strides and m * row_stride are 64-bit (an operand may pass 2^32 bytes through M or the batch); inside one 64-row tile
 * the byte offsets are 32-bit: (64 * ld + K) * 4 for a k-contiguous operand, K * ld * 4 for a k-strided one, 64 * ldc * 4 and
 * 64 * ld_mask * 4 must each stay below 0x7fffffff, else LAMP_E_UNSUPPORTED; batch0 * batch1 <= 65535, else LAMP_E_DIMS.
 * lamp_gemm_grouped validates every description before its launch: one description beyond a limit refuses the call, no C is written. */
typedef struct lamp_gemm_desc {
    const float* A;
    const float* B;
    float* C;
    int32_t M, N, K;
    int32_t batch0, batch1;
    int32_t accumulate;
    int64_t a_row_stride, a_col_stride, a_batch0, a_batch1;
    int64_t b_row_stride, b_col_stride, b_batch0, b_batch1;
    int64_t ldc, c_batch0, c_batch1;
    const float* relu_mask;
    int64_t ld_mask;
    float alpha;
    int32_t reserved;
} lamp_gemm_desc;
size_t lamp_gemm_workspace_bytes(int32_t M, int32_t N, int32_t K, int32_t batch);
int lamp_gemm(const lamp_gemm_desc* d, void* workspace, size_t workspace_bytes, lamp_stream_t stream);

/* n independent lamp_gemm products in ONE launch (descs: host array; batch0 = batch1 = 1, relu_mask NULL, the same operand
 * form -- which of A / B is k-contiguous -- in all of them, distinct C).  No K split, no workspace: every 64 x 64 output
 * tile accumulates k in ascending order, so the results are those of lamp_gemm without workspace, whatever the grouping.
 * Meant for the weight gradients of a whole backward pass (train.py:40 `loss.backward()`: dW = dY^T.X of every nn.Linear /
 * Conv1d(k=1) on the path, lamp/SubLayers.py:60-64,129-130), which are off the critical path of the data gradients and fill
 * the chip together where each alone would need a K split.  Order descs deepest K first. */
int lamp_gemm_grouped(const lamp_gemm_desc* descs, int32_t n, lamp_stream_t stream);

/* ---- training-mode sub-layers, ONE call each ------------------------------------------------------------------
 * The launches that lamp_amd/training.py's autograd functions would issue one Python round trip at a time (a reuters
 * training step is ~190 launches and was bound by the issuing thread, not the device), issued by the library.  Same
 * kernels, same order, same bits as the per-launch route.  All buffers are the caller's ([rows, cols] row-major, fp32):
 * "saved" ones must live until the matching backward call, gradients of weights may be NULL = the caller computes them
 * later from the buffers this call leaves behind (lamp_gemm_grouped). */

/* Second stage of a column reduction (LayerNorm-parameter and bias gradients of `loss.backward()`, train.py:40 -- what autograd
 * computes for nn.LayerNorm / Conv1d biases in lamp/SubLayers.py:64,129-131): out[c] = sum over n_partials rows of
 * partial[p * n_total + c], c < n_total, in a fixed order; columns [i * n_seg, (i + 1) * n_seg) go to out[i] (n_total <= 3 n_seg).
 * lamp_ffn_bwd / lamp_mha_bwd describe theirs in such jobs instead of launching them when given a `partials` buffer, so that
 * ONE lamp_reduce_partials_grouped launch can run the jobs of a whole backward pass: 17 tiny dependent launches per reuters
 * step become one.  A job's partials and outputs are the caller's buffers and must stay live until that launch. */
typedef struct lamp_reduce_job {
    const float* partial;
    int64_t n_total, n_seg;
    float* out[3];
    int32_t n_partials;
    int32_t reserved;
} lamp_reduce_job;
int lamp_reduce_partials_grouped(const lamp_reduce_job* jobs, int32_t n, lamp_stream_t stream);

/* PositionwiseFeedForward.forward in train() mode (lamp/SubLayers.py:133-142):
 *   h = relu(x W1^T + b1) [M, d_inner] (saved), o = h W2^T + b2 [M, d_model] (saved), y = LayerNorm(dropout(o) + x). */
int lamp_ffn_train_fwd(const float* x, int64_t M, int32_t d_model, int32_t d_inner, const lamp_ffn_weights* w,
                       float dropout_p, uint32_t seed, float* h, float* o, float* y, lamp_stream_t stream);
/* Its backward.  dx [M, d_model] = gradient of x; d_o [M, d_model] = gradient of o (required iff dropout_p > 0; without
 * dropout it IS dx before the last accumulation, and dW2 must then be requested here); dh [M, d_inner] = gradient of the
 * pre-ReLU hidden; dW1 [d_inner, d_model] = dh^T x and dW2 [d_model, d_inner] = d_o^T h nullable (deferred);
 * db1 [d_inner], db2, dgamma, dbeta [d_model].
 * partials (nullable, lamp_ffn_bwd_partials_bytes): when given, db1 / db2 / dgamma / dbeta are NOT final on return -- jobs[0..1]
 * describe the two reductions that finish them (see lamp_reduce_job).
 * Workspace: lamp_ffn_bwd_workspace_bytes() is the maximum over the launches the call issues -- the LayerNorm backward, the
 * column sum, and lamp_gemm_workspace_bytes() of each of its four products (dW2, dh, dW1, dx), taken from the one table the
 * call issues them from -- so every product splits K exactly as lamp_gemm does for it with its own workspace (a smaller
 * workspace is LAMP_E_WORKSPACE).  lamp_mha_bwd_workspace_bytes() likewise: the LayerNorm backward and the eight
 * single-batch products (dfc, da, dwq, dwk, dwv and the three data gradients; the per-head products take no workspace). */
size_t lamp_ffn_bwd_workspace_bytes(int64_t M, int32_t d_model, int32_t d_inner);
size_t lamp_ffn_bwd_partials_bytes(int64_t M, int32_t d_model, int32_t d_inner);
int lamp_ffn_bwd(const float* x, const float* h, const float* o, const float* dy, int64_t M, int32_t d_model,
                 int32_t d_inner, const lamp_ffn_weights* w, float dropout_p, uint32_t seed, float* dx, float* d_o, float* dh,
                 float* dW1, float* dW2, float* db1, float* db2, float* dgamma, float* dbeta, void* workspace,
                 size_t workspace_bytes, void* partials, size_t partials_bytes, lamp_reduce_job* jobs, lamp_stream_t stream);

typedef struct lamp_mha_train_desc {
    int32_t B, lq, lk, d_model, n_head, d_k, d_v;   /* d_k, d_v <= 128 */
    float inv_temperature;                          /* 1 / sqrt(d_k) (lamp/SubLayers.py:62) */
    float p_attn, p_out;                            /* dropout of the probabilities (SubLayers.py:40) and of the output (:113) */
    uint32_t seed_attn, seed_out;
} lamp_mha_train_desc;
/* MultiHeadAttention.forward in train() mode (lamp/SubLayers.py:77-121) on xq [B, lq, d_model], xk / xv [B, lk, d_model]
 * (the same pointer for both in every layer of the reference).  Saved: q [B, lq, H*d_k], k, v [B, lk, H*d_*], a [B, lq, H*d_v]
 * (concatenated head outputs, computed from the DROPPED probabilities), P [H*B, lq, lk] (softmax, index head * B + b),
 * o [B*lq, d_model] (fc output; unused when w->fc is NULL).  Pd [H*B, lq, lk] = dropout(P), required iff p_attn > 0 -- what
 * the reference returns as the attention map.  lse: H*B*lq floats of scratch.  y = LayerNorm(dropout(o) + xq). */
int lamp_mha_train_fwd(const lamp_mha_train_desc* c, const lamp_mha_weights* w, const float* xq, const float* xk,
                       const float* xv, const lamp_mask* mask, float* q, float* k, float* v, float* a, float* P, float* Pd,
                       float* lse, float* o, float* y, lamp_stream_t stream);
/* Its backward.  Outputs: dxq [B*lq, d_model]; dxk [B*lk, d_model] (+ the value branch when dxv is NULL, else dxv gets it;
 * dxk == dxq is allowed when lq == lk -- self-attention, xq and xk one tensor: dxq then holds the SUM of the three branches);
 * dgamma, dbeta.  Left behind for deferred weight gradients: d_o [B*lq, d_model] (required iff p_out > 0), dq [B*lq, H*d_k],
 * dk [B*lk, H*d_k], dv [B*lk, H*d_v]; dwq / dwk / dwv [H*d_*, d_model], dfc [d_model, H*d_v] nullable (dfc required when
 * w->fc is set and p_out == 0).  Pd: the forward's dropout(P) (saved; required iff p_attn > 0).  Scratch: da [B*lq, H*d_v]
 * (iff w->fc), dP [H*B, lq, lk].  partials (nullable, lamp_mha_bwd_partials_bytes): when given, dgamma / dbeta are NOT final on
 * return -- job[0] describes the reduction that finishes them (see lamp_reduce_job). */
size_t lamp_mha_bwd_workspace_bytes(const lamp_mha_train_desc* c);
size_t lamp_mha_bwd_partials_bytes(const lamp_mha_train_desc* c);
int lamp_mha_bwd(const lamp_mha_train_desc* c, const lamp_mha_weights* w, const float* xq, const float* xk, const float* xv,
                 const float* q, const float* k, const float* v, const float* a, const float* P, const float* Pd,
                 const float* o, const float* dy, float* dxq, float* d_o, float* da, float* dP, float* dq, float* dk, float* dv,
                 float* dxk, float* dxv, float* dgamma, float* dbeta, float* dwq, float* dwk, float* dwv, float* dfc,
                 void* workspace, size_t workspace_bytes, void* partials, size_t partials_bytes, lamp_reduce_job* job,
                 lamp_stream_t stream);

/* lamp_mha_train_fwd / lamp_mha_bwd with the activation as an argument (lamp/SubLayers.py:17-25,39-41).  LAMP_ATTN_SOFTMAX: the
 * functions above, bit for bit.  LAMP_ATTN_SIGMOID: P = sigmoid(S) with blocked entries exactly 0 (a fully blocked row is 0, not
 * NaN), written in the attention's single pass -- lse is unused and may be NULL; the backward's score gradient is
 * dS = inv_temperature * P * (1 - P) * dP, elementwise (lamp_sigmoid_attn_bwd).  Every other buffer as above. */
int lamp_mha_train_act_fwd(const lamp_mha_train_desc* c, const lamp_mha_weights* w, int32_t act, const float* xq,
                           const float* xk, const float* xv, const lamp_mask* mask, float* q, float* k, float* v, float* a,
                           float* P, float* Pd, float* lse, float* o, float* y, lamp_stream_t stream);
int lamp_mha_act_bwd(const lamp_mha_train_desc* c, const lamp_mha_weights* w, int32_t act, const float* xq, const float* xk,
                     const float* xv, const float* q, const float* k, const float* v, const float* a, const float* P,
                     const float* Pd, const float* o, const float* dy, float* dxq, float* d_o, float* da, float* dP, float* dq,
                     float* dk, float* dv, float* dxk, float* dxv, float* dgamma, float* dbeta, float* dwq, float* dwk,
                     float* dwv, float* dfc, void* workspace, size_t workspace_bytes, void* partials, size_t partials_bytes,
                     lamp_reduce_job* job, lamp_stream_t stream);

/* y = LayerNorm(dropout(x) + residual[row % residual_rows]) (residual nullable; residual_rows 0 = one residual row
 * per x row): the dropout, add & norm that closes every sub-layer (lamp/SubLayers.py:113-115,138-140), with neither
 * the dropped tensor nor the sum ever stored.  dropout_p = 0: plain add & norm; otherwise lamp_dropout's counter-based
 * mask for `seed`, element index = row * d + column. */
int lamp_layernorm_residual_fwd(const float* x, const float* residual, int64_t residual_rows, int64_t M, int32_t d,
                                const float* gamma, const float* beta, float eps, float dropout_p, uint32_t seed,
                                float* y, lamp_stream_t stream);

/* Backward of the above; z = dropout(x) + residual is recomputed from the same inputs.  Given dy it returns
 *   dz [M, d]      gradient of z, i.e. of the residual branch,
 *   dx [M, d]      gradient of x = dropout(dz) with the same mask (written only when dropout_p > 0; with p = 0 the
 *                  gradient of x is dz itself and dx may be NULL),
 *   dgamma, dbeta  [d]: sum_rows dy * zhat, sum_rows dy,
 *   dbias [d]      (nullable): sum_rows of the gradient of x -- the bias gradient of the linear map that produced x.
 * d <= 4096.  Row sums are two-stage in a fixed order (deterministic). */
size_t lamp_layernorm_bwd_workspace_bytes(int64_t M, int32_t d);
int lamp_layernorm_bwd(const float* x, const float* residual, int64_t residual_rows, int64_t M, int32_t d,
                       const float* gamma, float eps, float dropout_p, uint32_t seed, const float* dy, float* dz,
                       float* dx, float* dgamma, float* dbeta, float* dbias, void* workspace, size_t workspace_bytes,
                       lamp_stream_t stream);

/* out[n] = sum_m x[m*ldx + n]: bias gradients, and the label-table gradient (sum over the batch).  M, N and ldx are 64-bit and x may be
 * of any size; (N + 255) / 256 > 0x7fffffff is LAMP_E_DIMS (lamp_attn_bias_bwd likewise with N = lq * lk). */
size_t lamp_colsum_workspace_bytes(int64_t M, int64_t N);
int lamp_colsum(const float* x, int64_t M, int64_t N, int64_t ldx, float* out, void* workspace,
                size_t workspace_bytes, lamp_stream_t stream);

/* The gradient of a learnable LAMP_MASK_BIAS_F32 score bias shared by batch and heads.  S = Q K^T / temperature + bias, so
 *   dbias[q*ld + k] = scale * sum_{n < n_slices} dS[(n*lq + q)*lk + k]
 * with dS [n_slices, lq, lk] contiguous -- what lamp_mha_bwd / lamp_mha_act_bwd leave in their dP argument (n_slices = n_head * B)
 * and lamp_softmax_bwd writes -- and scale = 1 / inv_temperature (dS carries that factor).  bias: the forward's folded bias
 * [lq, bias_stride_q] or NULL; where it holds -inf, dbias is written as exactly 0 WHATEVER dS holds there (a fully blocked
 * row's NaN does not reach the parameter).  A NaN behind an allowed entry stays in that element.  ld >= lk; columns lk .. ld - 1
 * of dbias are not written.  Two launches, no atomics: lamp_colsum's first stage over the [n_slices, lq * lk] view, then one
 * pass that adds the partials in a fixed order -- the summation order is a function of n_slices alone, the result is
 * bit-identical from run to run.  LAMP_E_DIMS (a non-positive size, ld < lk, bias_stride_q < lk), LAMP_E_NULL (dS, dbias,
 * workspace), LAMP_E_WORKSPACE, in that order, before any launch. */
size_t lamp_attn_bias_bwd_workspace_bytes(int64_t n_slices, int32_t lq, int32_t lk);
int lamp_attn_bias_bwd(const float* dS, int64_t n_slices, int32_t lq, int32_t lk, float scale, const float* bias,
                       int64_t bias_stride_q, float* dbias, int64_t ld, void* workspace, size_t workspace_bytes,
                       lamp_stream_t stream);

/* The buffer LAMP_FWD_LABEL_BIAS / LAMP_MASK_BIAS_F32 read, from a learnable [L, ld_p] bias and the byte label mask:
 *   out[q*ld_o + k] = blocked_u8[q*L + k] ? -inf : param[q*ld_p + k]   (k < L);   0 in the pad columns L .. ld_o - 1
 * with ld_o = (L + 3) & ~3; blocked_u8 NULL = no mask.  One launch, a pure function of its inputs: a weights-only
 * precomputation that is run again whenever the parameter changed.  LAMP_E_DIMS (L <= 0, ld_p < L), LAMP_E_NULL (param, out). */
int lamp_label_bias_fold(const float* param, int64_t ld_p, const uint8_t* blocked_u8, int32_t L, float* out,
                         lamp_stream_t stream);

/* nn.Dropout in training mode (lamp/SubLayers.py:40,113,138): y[e] = keep(e, seed) ? x[e] / (1 - p) : 0 with a
 * counter-based generator -- keep(e, seed) = mix32(e, seed) >= p * 2^32 -- so the mask is a pure function of
 * (element index, seed) and is never stored: calling it again on the gradient with the same seed IS the backward
 * pass.  y may alias x.  (The stream of random numbers necessarily differs from torch's Philox stream.)  The element index is 64 bits
 * wide and both of its words are mixed in: n has no limit, and elements 2^32 .. have a mask of their own. */
int lamp_dropout(const float* x, int64_t n, float p, uint32_t seed, float* y, lamp_stream_t stream);

/* Softmax backward per row of length lk: dS = scale * P * (dP - sum_k P * dP); dS may alias dP.  rows * lk may pass 2^31 elements
 * (64-bit row offsets); (rows + 3) / 4 > 0x7fffffff is LAMP_E_DIMS. */
int lamp_softmax_bwd(const float* P, const float* dP, int64_t rows, int32_t lk, float scale, float* dS,
                     lamp_stream_t stream);

/* Backward of the sigmoid attention's activation (lamp/SubLayers.py:17-25,39), elementwise over rows * lk entries:
 *   dS = scale * P * (1 - P) * dropout_backward(dP)
 * P = 0 on blocked entries keeps their gradient at exactly 0 (no NaN anywhere).  dropout_p > 0: dP is the gradient of
 * dropout(P) and lamp_dropout's mask for (`seed`, element index = row * lk + column) is applied on load; 0: dP as it is.
 * dS may alias dP.  rows * lk has no limit (a 64-bit element index, which is also the dropout counter). */
int lamp_sigmoid_attn_bwd(const float* P, const float* dP, int64_t rows, int32_t lk, float scale, float dropout_p,
                          uint32_t seed, float* dS, lamp_stream_t stream);

/* Backward of lamp_diag_logits_fwd: dy[b,i,:] = dlogits[b,i] * w_out[i,:], dw[i,:] = sum_b dlogits[b,i] * y[b,i,:]. */
int lamp_diag_logits_bwd(const float* y, const float* w_out, const float* dlogits, int32_t B, int32_t L,
                         int32_t d_model, float* dy, float* dw, lamp_stream_t stream);

/* Backward of the embedding gather: d_emb[src_seq[t], :] += dout[t, :] (atomic adds; rows of pad_idx are skipped as
 * nn.Embedding(padding_idx) does; pass -1 for none).  d_emb must be initialised by the caller. */
int lamp_embed_bwd(const int64_t* src_seq, int64_t n_tokens, const float* dout, int32_t d_model, int32_t n_vocab,
                   int64_t pad_idx, float* d_emb, lamp_stream_t stream);

/* ---- the whole hot path ------------------------------------------------------------------- */

/* Bytes of workspace lamp_forward needs to process `micro_batch` samples of padded length T at a
 * time.  lamp_forward splits B into micro-batches of floor(workspace_bytes / bytes(1)) samples.
 * bytes(1) is also the least a call accepts: one byte less is LAMP_E_WORKSPACE before anything is launched or written. */
size_t lamp_forward_workspace_bytes(const lamp_model* m, int32_t micro_batch, int32_t T,
                                    int32_t want_attn);

/* LAMP.forward (lamp/Models.py:110-137) for encoder='graph', decoder='graph', eval mode:
 *   src_seq, src_pos int64 [B, T]  ->  logits [B, n_labels], enc_output [B, T, d_model].
 * The encoder self-attention, whose output the reference discards (lamp/Layers.py:16-18), is
 * computed only when aux->enc_self_attn is given.
 * Ragged batches (utils/data_loader.py:261-279 pads to the longest document): PAD positions are not computed.  The call's
 * first kernel counts each sample's extents on the device; the encoder runs on the packed non-PAD rows plus ONE shared PAD
 * row (every PAD position of lamp/Encoders.py:64-79 holds the same row-wise result), and the enc-dec attention stops at
 * each sample's last non-PAD key (keys past it are exactly masked, lamp/utils.py:26-34).  enc_output is still the padded
 * [B, T, d_model] tensor the reference returns, PAD positions included, and a sample's outputs do not depend on T, on
 * B or on the micro-batch split, bit for bit. */
int lamp_forward(const lamp_model* m, const int64_t* src_seq, const int64_t* src_pos,
                 int32_t B, int32_t T, float* logits, float* enc_output, const lamp_aux* aux,
                 void* workspace, size_t workspace_bytes, lamp_stream_t stream);

/* Options of lamp_forward_opts / lamp_onehot_forward_opts.  NULL, or a zeroed struct, is lamp_forward as it is.
 *   enc_self_attn != 0: the encoder's self-attention is LIVE -- the feature->feature step of the published model.  The
 *     reference computes the block and then overwrites its output (lamp/Layers.py:16-18: `enc_output = pos_ffn(enc_input)`);
 *     with this flag a layer is  h, attn = slf_attn(x, x, x, mask);  out = pos_ffn(h)  instead.  The encoder then runs the
 *     padded [B, T, d_model] layout: every position is a query (a PAD query's zero row attends uniformly over its sample's
 *     live keys, as the definition gives), each sample's keys stop at its last non-PAD token, and a sample whose tokens are
 *     all PAD comes out NaN.  m->enc0_emb_w1 must be NULL (a live layer 0 does not start with W1).  aux->enc_self_attn, when
 *     given, receives the maps of the attention that was used.
 *   enc_mask (nullable): one byte mask per sample for the encoder's self-attention in place of the key-padding rule of
 *     lamp/Encoders.py:82 -- the per-sample input graphs of lamp/Encoders.py:85-89.  LAMP_MASK_U8 with stride_b != 0,
 *     element (b, q, k) at ptr[b * stride_b + q * stride_q + k] over the padded T x T square, nonzero = blocked, no tile list.
 *     Needs the flag above or aux->enc_self_attn (otherwise nothing reads it: LAMP_E_UNSUPPORTED).
 *   enc_chain_packs (nullable): host array of n_layers_enc packs of (slf_attn.fc, pos_ffn.w_1, pos_ffn.w_2), as
 *     lamp_model.chain_packs holds them for the decoder: the live layer's row-local tail then runs as one chain launch where
 *     the decoder's would.  Same bits with and without. */
#define LAMP_FWD_PACKED_ENCODER 1  /* lamp_fwd_options.flags, with enc_self_attn: run the live encoder on the PACKED non-PAD token
                                      rows plus one PAD row per sample (csrc/attention_ragged.hip: queries as ragged as keys, no PAD
                                      position computed) where it applies -- no enc_mask, no encoder maps, no one-hot front end,
                                      every encoder layer with more than one head, d_k == d_v <= 128, T <= ~16 k -- else the padded
                                      layout as without the flag.  Same definition, other kernel: results agree within rounding,
                                      not bit for bit, with the padded route; a sample's bits do not depend on T or B either way. */

#define LAMP_FWD_DEC_SIGMOID 2     /* lamp_fwd_options.flags: BOTH attention blocks of every decoder layer (lamp/Layers.py:35,40) run
                                      sigmoid attention -- P = sigmoid(Q K^T / temperature), blocked entries exactly 0, no row
                                      normalisation (lamp/SubLayers.py:17-25,39); a label without one allowed neighbour receives 0,
                                      not NaN.  The reference accepts attn_type and never hands it to its layers (lamp/Layers.py:
                                      23-30): this is the opt-in that does what the flag says.  The encoder, dead or live, stays
                                      softmax (the reference never gives it an attn_type); aux maps of the decoder are the sigmoid
                                      maps.  Micro-batching and the bit-for-bit independence from B, T and the split hold. */

#define LAMP_FWD_MATMUL_BF16X3 4   /* lamp_fwd_options.flags: every nn.Linear-class GEMM launch of the forward runs at LAMP_PREC_BF16X3 */
#define LAMP_FWD_MATMUL_BF16X6 8   /* ... at LAMP_PREC_BF16X6.  Both flags together: LAMP_E_UNSUPPORTED.
                                      Covered (lamp_forward_opts and lamp_onehot_forward_opts): the encoder's feed-forward GEMMs
                                      including the one with the gathered residual, the K/V, Q and Q/K/V projections of every
                                      attention block, the live encoder's projections, and the separate-launch tails (fc, W1, W2)
                                      where the chain launch does not apply.
                                      These STAY fp32: the chain launch (csrc/chain.hip); every attention kernel; conv2 of the
                                      one-hot front end; the read-out; the weights-only precomputations a caller builds once per
                                      weight version (hoisted layer-0 query, embedding fold tables); all of training, lamp_gemm /
                                      lamp_gemm_grouped and the backward.  The workspace functions return what they return
                                      without the flags.  A sample's bits stay independent of B, T and the micro-batch split. */

#define LAMP_FWD_LABEL_BIAS 16     /* lamp_fwd_options.flags (lamp_forward_opts and lamp_onehot_forward_opts): lamp_model.label_mask
                                      is read as a const float* [n_labels, ld] score bias, ld = (n_labels + 3) & ~3, 16-byte
                                      aligned (else LAMP_E_ALIGN), instead of a byte mask: the label self-attention of every
                                      decoder layer runs under LAMP_MASK_BIAS_F32 (NULL: no bias, no mask).  The enc-dec attention
                                      and the encoder never take it.  label_mask_bits, label_tiles, label_mask_flags and
                                      label_mask_allowed must be 0, and LAMP_FWD_DEC_SIGMOID must not be set: LAMP_E_UNSUPPORTED.
                                      The workspace functions return what they return without the flag.  Micro-batching holds;
                                      a sample's bits stay independent of B, T and the split (the kernel's key split is a
                                      function of n_labels alone). */

typedef struct lamp_fwd_options {
    int32_t enc_self_attn;
    int32_t flags;               /* LAMP_FWD_PACKED_ENCODER | LAMP_FWD_DEC_SIGMOID | LAMP_FWD_MATMUL_BF16X3 / _BF16X6 |
                                    LAMP_FWD_LABEL_BIAS, or 0 */
    const lamp_mask* enc_mask;
    const lamp_chain_pack* enc_chain_packs;
} lamp_fwd_options;

/* lamp_forward_workspace_bytes / lamp_forward with options (a live encoder needs query and attention-output rows for
 * max(T, n_labels) positions per sample instead of n_labels).  Sized and carved from the same layout; micro-batching and
 * the bit-for-bit independence of a sample from B and from the split hold as for lamp_forward.  The live self-attention runs
 * under LAMP_MASK_SELF_RAGGED, so a sample's bits do not depend on T either (d_k, d_v <= 128). */
size_t lamp_forward_opts_workspace_bytes(const lamp_model* m, const lamp_fwd_options* opts, int32_t micro_batch, int32_t T,
                                         int32_t want_attn);
int lamp_forward_opts(const lamp_model* m, const lamp_fwd_options* opts, const int64_t* src_seq, const int64_t* src_pos,
                      int32_t B, int32_t T, float* logits, float* enc_output, const lamp_aux* aux, void* workspace,
                      size_t workspace_bytes, lamp_stream_t stream);

/* Optional, weights-only: lamp_pack_weight(format 0) copies of the weight matrices whose projections run as launches of the
 * tile GEMM at sizes where its one-wave-row tile is chosen -- that tile then loads its weight fragments straight from the pack
 * (one contiguous KiB per wave instruction) and no longer passes the weight through LDS.  Same bits with and without, member by
 * member: a NULL member (or array, or struct) leaves that launch on the row-major weight, as does a shape the pack cannot express
 * (output width not a multiple of 16, d_model / d_inner not a multiple of 32), a LAMP_FWD_MATMUL_* flag, or an output / bias /
 * residual that cannot move as 16-byte accesses.  Like lamp_model.chain_packs they depend on weights only: build them once per
 * weight version; each is as large as its matrix (1 MiB for 512 x 512).  The K / V projection of the encoder rows takes its packs
 * from lamp_kv_gemm_pack below (lamp_forward_packs_kv); these three structs keep the layout lamp_forward_packs was published with. */
typedef struct lamp_dec_gemm_pack {
    const float* enc_q;  /* dec_layers[i].enc_attn.w_qs */
    const float* slf_q;  /* dec_layers[i].slf_attn.w_qs, w_ks, w_vs: one three-segment launch, packed when all three are given */
    const float* slf_k;
    const float* slf_v;
} lamp_dec_gemm_pack;
typedef struct lamp_enc_gemm_pack {
    const float* w1;     /* enc_layers[i].pos_ffn.w1 */
    const float* w2;     /* enc_layers[i].pos_ffn.w2 */
} lamp_enc_gemm_pack;
typedef struct lamp_gemm_packs {
    const lamp_enc_gemm_pack* enc;  /* host array of n_layers_enc entries, or NULL */
    const lamp_dec_gemm_pack* dec;  /* host array of n_layers_dec entries, or NULL */
} lamp_gemm_packs;

/* lamp_forward_opts with weight packs for its GEMM launches (opts and packs nullable; workspace: lamp_forward_opts_workspace_bytes).
 * The packs ride beside the model instead of inside it: lamp_model keeps its layout, and a library without this entry point is
 * never handed one. */
int lamp_forward_packs(const lamp_model* m, const lamp_fwd_options* opts, const lamp_gemm_packs* packs, const int64_t* src_seq,
                       const int64_t* src_pos, int32_t B, int32_t T, float* logits, float* enc_output, const lamp_aux* aux,
                       void* workspace, size_t workspace_bytes, lamp_stream_t stream);

/* The packs of the K / V projection of the encoder rows, per decoder layer: dec_layers[i].enc_attn.w_ks / w_vs.  That projection is
 * one launch of 2 n segments for n decoder layers of one head geometry (or one launch per layer): the largest launch of a forward,
 * on the tall packed tile of csrc/gemm.hip.  A launch is packed when every segment of its own has a pack; a NULL member (or
 * array) leaves it on the row-major weights, with the same bits.  They ride in a struct and an entry point of their own, so that
 * lamp_dec_gemm_pack keeps its size -- a host array of it is walked by the library -- and a library without this entry point is
 * never handed them. */
typedef struct lamp_kv_gemm_pack {
    const float* enc_k;  /* dec_layers[i].enc_attn.w_ks */
    const float* enc_v;  /* dec_layers[i].enc_attn.w_vs */
} lamp_kv_gemm_pack;

/* lamp_forward_packs with kv_packs (nullable): host array of n_layers_dec entries. */
int lamp_forward_packs_kv(const lamp_model* m, const lamp_fwd_options* opts, const lamp_gemm_packs* packs, const lamp_kv_gemm_pack* kv_packs,
                          const int64_t* src_seq, const int64_t* src_pos, int32_t B, int32_t T, float* logits, float* enc_output,
                          const lamp_aux* aux, void* workspace, size_t workspace_bytes, lamp_stream_t stream);

/* ---- the one-hot genomics encoder (GraphEncoder(onehot=True), lamp/Encoders.py:46-51,68-73) ----------------------
 * For src_seq / src_pos int64 [B, T] over a vocabulary of n_vocab (9) symbols, with T2 = T / 2:
 *   y1 = conv1(E[src]^T)[:, :, :T]            Conv1d(n_vocab, d, 16, padding 8)
 *   P  = max_pool1d(relu(dropout(y1)), 2, 2)   [B, T2, d]
 *   X  = relu(conv2(P)[:, :, :T2])^T + position_enc(src_pos[:, :T2])   Conv1d(d, d, 16, padding 8) -> the encoder's rows
 * and src_seq[:, :T2] is the key-padding source of the encoder and of the enc-dec attention.  conv1's input is one-hot, so it
 * is a gather from the weights-only tap table t1[v][t][:] = sum_ci E[v][ci] conv1_w[:][ci][t] (the caller builds it once per
 * weight version).  conv2_pack (nullable): conv2_w repacked [co][t][ci] by lamp_conv_pack(flip 0); without it every forward
 * repacks into its workspace.  16-byte aligned pointers, d_model % 4 == 0. */
typedef struct lamp_onehot_frontend {
    const float* t1;          /* [n_vocab, 16, d_model] */
    const float* conv1_b;     /* [d_model] */
    const float* conv2_w;     /* [d_model, d_model, 16] (Conv1d layout; may be NULL when conv2_pack is given) */
    const float* conv2_b;     /* [d_model] */
    const float* conv2_pack;  /* [d_model, 16, d_model] or NULL */
    int32_t n_vocab;          /* <= 16 */
    int32_t taps;             /* 16 */
} lamp_onehot_frontend;

/* lamp_forward with the one-hot front end in place of the embedding gather: logits [B, n_labels], enc_output [B, T2, d_model].
 * m describes the encoder layers and the decoder as for lamp_forward (m->position_enc required, m->enc0_emb_w1 NULL).  The
 * encoder runs the padded layout (T2 depends on the padded length, so padding is part of the result); a sample's outputs do
 * not depend on B or on the micro-batch split, bit for bit, at a fixed T.  conv2 is counted in LAMP_K_GEMM. */
size_t lamp_onehot_forward_workspace_bytes(const lamp_model* m, const lamp_onehot_frontend* fe, int32_t micro_batch, int32_t T,
                                           int32_t want_attn);
int lamp_onehot_forward(const lamp_model* m, const lamp_onehot_frontend* fe, const int64_t* src_seq, const int64_t* src_pos,
                        int32_t B, int32_t T, float* logits, float* enc_output, const lamp_aux* aux, void* workspace,
                        size_t workspace_bytes, lamp_stream_t stream);

/* lamp_onehot_forward with options (lamp_fwd_options above; enc_mask then covers the T2 x T2 square). */
size_t lamp_onehot_forward_opts_workspace_bytes(const lamp_model* m, const lamp_onehot_frontend* fe, const lamp_fwd_options* opts,
                                                int32_t micro_batch, int32_t T, int32_t want_attn);
int lamp_onehot_forward_opts(const lamp_model* m, const lamp_onehot_frontend* fe, const lamp_fwd_options* opts,
                             const int64_t* src_seq, const int64_t* src_pos, int32_t B, int32_t T, float* logits,
                             float* enc_output, const lamp_aux* aux, void* workspace, size_t workspace_bytes,
                             lamp_stream_t stream);

/* Building blocks of the one-hot encoder (training, module-by-module use).  Padded layout "xpad": [B * (T2 + 16) + 16, d]
 * rows, sample b's row q at b * (T2 + 16) + 8 + q, every other row 0.
 *   lamp_conv_pack:        flip 0: packed[co][t][ci] = w[co][ci][t];  flip 1: packed[ci][t][co] = w[co][ci][taps - 1 - t].
 *   lamp_onehot_front_fwd: xpad of P (above); dropout_p > 0: lamp_dropout's counter-based mask on y1, element
 *                          (b * T + p) * d_model + c (channel-last).
 *   lamp_conv_window_fwd:  out[b * rows_out + q][n] = act(sum_{t < 16, ci} x[(b * rows_in + q + t) * c_in + ci] w_pack[n][t][ci]
 *                          + bias[n]) + pos_table[src_pos[b * pos_ld + q]][n]  (bias, pos_table, relu_out nullable; relu_out
 *                          gets act(...) before the position row).  Every output row reads 16 input rows, so rows_in >=
 *                          rows_out + 15 (else LAMP_E_DIMS) and x must hold (B - 1) * rows_in + rows_out + 15 rows.
 *                          conv2 forward: x = xpad, rows_out = T2, rows_in = T2 + 16;
 *                          its input gradient: x = the padded dZ + one row, w_pack = the flip-1 repack.
 *   lamp_conv_relu_bwd_pad: dz (xpad layout) = dy * (relu_out > 0), dy / relu_out [B * rows, d].
 *   lamp_onehot_front_bwd: from dP [B, T2, d] (the gradient of P): dz [B, T, d] = the gradient of y1, and partials
 *                          (lamp_onehot_front_bwd_partials_bytes) whose column sums (lamp_colsum over n_vocab * 16 * d
 *                          columns) are the gradient of t1; dz's column sums are conv1's bias gradient.  Deterministic. */
int lamp_conv_pack(const float* w, int32_t c_out, int32_t c_in, int32_t taps, int32_t flip, float* packed, lamp_stream_t stream);
int lamp_onehot_front_fwd(const int64_t* src_seq, int32_t B, int32_t T, const lamp_onehot_frontend* fe, int32_t d_model,
                          float dropout_p, uint32_t seed, float* xpad, lamp_stream_t stream);
int lamp_conv_window_fwd(const float* xpad, int32_t B, int32_t rows_out, int32_t rows_in, int32_t c_in, const float* w_pack,
                         int32_t c_out, const float* bias, int32_t relu, const float* pos_table, int32_t n_position,
                         const int64_t* src_pos, int64_t pos_ld, float* out, float* relu_out, lamp_stream_t stream);
int lamp_conv_relu_bwd_pad(const float* dy, const float* relu_out, int32_t B, int32_t rows, int32_t d, float* dz,
                           lamp_stream_t stream);
size_t lamp_onehot_front_bwd_partials_bytes(int32_t B, int32_t T, int32_t n_vocab, int32_t d_model);
int lamp_onehot_front_bwd(const int64_t* src_seq, int32_t B, int32_t T, const lamp_onehot_frontend* fe, int32_t d_model,
                          float dropout_p, uint32_t seed, const float* dP, float* dz, float* partials, size_t partials_bytes,
                          lamp_stream_t stream);

/* ---- the evaluation's metrics (utils/evals.py:316-407 compute_metrics) ----------------------------------------------
 * probs / targets: fp32 [n_rows, L] row-major with row strides ld_probs / ld_targets (elements, >= L), device-resident, not
 * modified.  Scores are probabilities: [0, 1] is the contract of these entry points; targets are 0 / 1.
 *
 * lamp_ranking_metrics replaces, per label column, roc_auc_score (compute_auc, utils/evals.py:283-298),
 * precision_recall_curve + auc (compute_aupr, :228-243) and the recall at FDR <= fdr_cutoff (compute_fdr, :208-225) by ONE
 * sort of the column.  With the column sorted by score descending, equal scores collapsed into groups k = 1..G, tp_k / fp_k
 * the cumulative positives / negatives through group k, P = tp_G, N = fp_G, tp_0 = fp_0 = 0, q_k = tp_k / (tp_k + fp_k),
 * q_0 = 1, r_k = tp_k / P:
 *   auc[l]        = sum_k (fp_k - fp_{k-1}) (tp_k + tp_{k-1}) / (2 P N)   64-bit integer numerator, one fp64 division;
 *                   NaN when P == 0 or N == 0
 *   aupr[l]       = sum_k (r_k - r_{k-1}) (q_k + q_{k-1}) / 2             fp64, fixed summation order; NaN when P == 0
 *   fdr_recall[l] = r_k of the lowest-scored group with 1 - q_k <= fdr_cutoff (fp64), 0 when there is none; NaN when P == 0
 *   n_pos / n_neg = P / N (nullable)
 * A column holding a NaN score, a score outside [0, 1] or a target other than 0 / 1 is unranked: NaN in all three, 0 in
 * n_pos / n_neg; the other columns are unaffected.  Deterministic: the same bits from run to run and under any permutation
 * of the rows.  n_rows < 2^31.  The workspace needs no alignment. */
size_t lamp_ranking_metrics_workspace_bytes(int64_t n_rows, int32_t L);
int lamp_ranking_metrics(const float* probs, int64_t ld_probs, const float* targets, int64_t ld_targets, int64_t n_rows,
                         int32_t L, double fdr_cutoff, double* auc, double* aupr, double* fdr_recall, int64_t* n_pos,
                         int64_t* n_neg, void* workspace, size_t workspace_bytes, lamp_stream_t stream);

/* The integer counts behind the thresholded figures (compute_tp_fp_fn and the per-sample loops of utils/evals.py:347-357),
 * with prediction = (score, NaN read as 0) >= threshold and gold = target != 0:
 *   label_tp / label_fp / label_fn [L];  sample_tp, sample_pred (predicted labels), sample_gold (gold labels) and
 *   sample_mismatch (labels where prediction != gold) [n_rows].  All outputs are written in full.  n_rows * L may pass 2^32 bytes; the
 *   per-label counts are int32, so n_rows >= 2^31 is LAMP_E_UNSUPPORTED before any launch (lamp_threshold_counts_vec likewise). */
int lamp_threshold_counts(const float* probs, int64_t ld_probs, const float* targets, int64_t ld_targets, int64_t n_rows,
                          int32_t L, float threshold, int32_t* label_tp, int32_t* label_fp, int32_t* label_fn,
                          int32_t* sample_tp, int32_t* sample_pred, int32_t* sample_gold, int32_t* sample_mismatch,
                          lamp_stream_t stream);

/* ---- decision thresholds fitted per label (csrc/thresholds.hip) -------------------------------------------------------
 * lamp_tune_thresholds chooses, per label column, the threshold that is best under `criterion` on the given rows -- what
 * the reference's Find_Optimal_Cutoff (utils/evals.py:301-313, its use commented out at :335-336) set out to do.  Same inputs
 * and the same sort as lamp_ranking_metrics.  With the column sorted by score descending, equal scores collapsed into groups
 * k = 1..G (-0.0 counts as +0.0), tp_k / fp_k the cumulative positives / negatives through group k, P = tp_G, N = fp_G and
 * cnt_k = tp_k + fp_k, the candidates are c = 0..G:
 *   c = 0   predicts nothing: threshold +inf, tp_0 = fp_0 = cnt_0 = 0;
 *   c = k   threshold = the score of group k, the very bits; by the rule of lamp_threshold_counts (score >= threshold) it
 *           predicts groups 1..k: tp_k true and fp_k false positives.
 * The criteria are decided by exact integer comparison; no floating point takes part in the choice:
 *   LAMP_TUNE_F1       maximise F1 = 2 tp / (2 tp + fp + fn) = 2 tp_c / (cnt_c + P): a beats b iff
 *                      tp_a (cnt_b + P) > tp_b (cnt_a + P)   (unsigned 64-bit; n_rows < 2^31)
 *   LAMP_TUNE_YOUDEN   maximise tp_c N - fp_c P   (signed 64-bit): tpr - fpr scaled by P N
 *   LAMP_TUNE_BALANCE  minimise |tp_c N + fp_c P - P N|: |tpr - (1 - fpr)| scaled by P N, the quantity Find_Optimal_Cutoff
 *                      minimises.  The reference's own answer can differ: sklearn's roc_curve drops collinear points by default
 *                      (drop_intermediate=True), so some candidates never reach its argsort, and that argsort leaves ties open.
 * A tie goes to the smallest c: the highest threshold, the fewest predictions.  Hence with P == 0 all three criteria choose
 * c = 0 (every candidate has tp = 0), and LAMP_TUNE_YOUDEN / LAMP_TUNE_BALANCE with N == 0 tie everywhere and give c = 0.
 * Outputs, [L] each:  threshold (+inf for c = 0);  tp, fp = tp_c, fp_c of the chosen candidate;  n_pos, n_neg = P, N;
 * tuned = 1 (nullable).  A column that lamp_ranking_metrics cannot rank (a NaN score, a score outside [0, 1], a target other
 * than 0 / 1) gets threshold = fallback, 0 in the four counts and tuned = 0; the other columns are unaffected.
 * Deterministic: the same bits from run to run and under any permutation of the rows.  Nothing is allocated, synchronised or
 * read back, the inputs are not written, everything is enqueued on `stream`.  The workspace needs no alignment.  Validation
 * before any launch, in this order: LAMP_E_DIMS (a non-positive size, ld < L), LAMP_E_NULL (any pointer but tuned),
 * LAMP_E_UNSUPPORTED (an unknown criterion, n_rows >= 2^31, a shape the sort does not serve), LAMP_E_WORKSPACE.
 * lamp_tune_thresholds_workspace_bytes is 0 for a shape that is not served.
 *
 * lamp_threshold_counts_vec is lamp_threshold_counts with one threshold per label: thresholds fp32 [L], device-resident.
 * prediction = (score, NaN read as 0) >= thresholds[label].  A +inf threshold predicts nothing (scores are <= 1), and so
 * does a NaN threshold (the comparison is false).  With every entry equal to t it writes what lamp_threshold_counts(t)
 * writes.  LAMP_E_DIMS, LAMP_E_NULL, LAMP_E_UNSUPPORTED in that order before any launch. */
enum lamp_tune_criterion { LAMP_TUNE_F1 = 0, LAMP_TUNE_YOUDEN = 1, LAMP_TUNE_BALANCE = 2 };
size_t lamp_tune_thresholds_workspace_bytes(int64_t n_rows, int32_t L);
int lamp_tune_thresholds(const float* probs, int64_t ld_probs, const float* targets, int64_t ld_targets, int64_t n_rows,
                         int32_t L, int32_t criterion, float fallback, float* threshold, int32_t* tp, int32_t* fp,
                         int32_t* n_pos, int32_t* n_neg, int32_t* tuned, void* workspace, size_t workspace_bytes,
                         lamp_stream_t stream);
int lamp_threshold_counts_vec(const float* probs, int64_t ld_probs, const float* targets, int64_t ld_targets, int64_t n_rows,
                              int32_t L, const float* thresholds, int32_t* label_tp, int32_t* label_fp, int32_t* label_fn,
                              int32_t* sample_tp, int32_t* sample_pred, int32_t* sample_gold, int32_t* sample_mismatch,
                              lamp_stream_t stream);

/* ---- ranking the labels of one sample: top-k predictions, precision / nDCG / recall at k (csrc/rank_at_k.hip) ---------
 * THE ORDER.  In a row of scores, element a at column i ranks before element b at column j when one of these holds:
 *   1. a is a number and b is NaN;
 *   2. both are numbers and a > b as floats;
 *   3. neither of the above decides (equal numbers, or both NaN) and i < j.
 * So +0.0 and -0.0 are tied, +inf is the largest value, -inf ranks above every NaN, and a row of equal scores yields columns
 * 0 .. k-1.  A row's result depends on that row's L scores and on k only: not on n_rows, the row's position, the row stride or
 * what lies in the padding beyond column L.
 *
 * lamp_topk_labels: scores fp32 [n_rows, L], row stride ld >= L (elements), device-resident, not modified; any finite or
 * non-finite values (logits or probabilities).  idx int32 [n_rows, k] (row stride ld_idx >= k) receives the columns of the k
 * first-ranked elements in rank order; val (nullable) fp32 [n_rows, k] (row stride ld_val >= k) the selected elements' own
 * bits (-0.0 stays -0.0, a NaN keeps its payload).  The gaps of a strided output are not written.  1 <= k <= 64, k <= L,
 * L <= 32768, n_rows < 2^31.  Every score is read once; no workspace, no atomics, nothing synchronised; the kernel chosen is a
 * function of L alone.
 *
 * lamp_rank_at_k: idx as lamp_topk_labels wrote it, targets fp32 [n_rows, L] (row stride ld_targets >= L).  A hit at rank r
 * (0-based) of sample i is targets[i, idx[i, r]] != 0 -- the gold rule of lamp_threshold_counts -- and gold_i the number of
 * nonzero targets of row i (an idx outside [0, L) is no hit).  discount / ideal are HOST arrays the caller computed in fp64:
 * discount[r] = 1 / log2(r + 2) for r < k, ideal[m] = discount[0] + ... + discount[m-1] for m <= k (k + 1 entries); they are
 * read before the call returns.  The device outputs, each k entries, entry j-1 for rank j = 1 .. k:
 *   hits_at_rank[j-1] = sum_i hit_{i, j-1}                                                             (int64)
 *   ndcg_sum[j-1]     = sum_i ( sum_{r<j} hit_{i,r} discount[r] ) / ideal[min(j, gold_i)]              (fp64)
 *   recall_sum[j-1]   = sum_i ( sum_{r<j} hit_{i,r} ) / gold_i                                         (fp64)
 *   n_with_gold       = samples with gold_i > 0                                                        (one int64)
 * A sample without a gold label adds 0 to both fp64 sums (and still counts in n_rows, by which the caller divides), as
 * sklearn.metrics.ndcg_score(..., ignore_ties=True) has it.  precision@j = (hits_at_rank[0] + ... + hits_at_rank[j-1]) /
 * (n_rows j).  Per-sample terms are written to the workspace first and added in an order fixed by n_rows: the same bits from
 * run to run; the integer outputs are also invariant under a permutation of the rows.  The workspace needs no alignment.
 *
 * Both validate before any launch, in this order: LAMP_E_DIMS (a non-positive size, ld < L, k > L, ld_idx < k, ld_val < k
 * with val given), LAMP_E_NULL, LAMP_E_UNSUPPORTED (k > 64, L > 32768, n_rows >= 2^31), LAMP_E_WORKSPACE.
 * lamp_rank_at_k_workspace_bytes is 0 for a request that is not served. */
int lamp_topk_labels(const float* scores, int64_t ld, int64_t n_rows, int32_t L, int32_t k, int32_t* idx, int64_t ld_idx,
                     float* val, int64_t ld_val, lamp_stream_t stream);
size_t lamp_rank_at_k_workspace_bytes(int64_t n_rows, int32_t k);
int lamp_rank_at_k(const int32_t* idx, int64_t ld_idx, const float* targets, int64_t ld_targets, int64_t n_rows, int32_t L,
                   int32_t k, const double* discount, const double* ideal, int64_t* hits_at_rank, double* ndcg_sum,
                   double* recall_sum, int64_t* n_with_gold, void* workspace, size_t workspace_bytes, lamp_stream_t stream);

/* ---- label-ranking metrics of whole rows: LRAP, coverage error, ranking loss, one-error, per-sample AUC (csrc/rank_at_k.hip)
 * scores / targets fp32 [n_rows, L] (row strides ld_scores, ld_targets >= L, elements), device-resident, not modified; the
 * scores may be logits or probabilities, any finite or non-finite value.
 * ROW ORDERING.  key(x) is the integer key behind THE ORDER above: +0.0 and -0.0 share a key, all NaNs share one key, which
 * lies below that of -inf; otherwise keys order as the floats do, denormals distinct.  a >= b below means key(a) >= key(b),
 * compared as integers.  The gold set of a row is P = {j : targets[j] != 0} (the rule of lamp_rank_at_k), N the other columns,
 * n_p = |P|, n_n = L - n_p.  For every p in P:
 *   rank_p = #{j : s_j >= s_p}            pos_p = #{j in P : s_j >= s_p}            (both count p itself)
 * THE TIE RULE: a column tied with p counts against it (it is "at or above"), as sklearn's label_ranking_loss and
 * label_ranking_average_precision_score (rank method 'max') have it.
 * Per row, int32 (row_counts, nullable, [n_rows, 6] contiguous, in this order):
 *   n_pos       n_p
 *   coverage    max_p rank_p; 0 for an empty row (n_p = 0), sklearn's coverage_error row
 *   misordered  sum_p (rank_p - pos_p): the pairs (p in P, n in N) with s_n >= s_p
 *   tied        sum_p #{n in N : key(s_n) == key(s_p)}
 *   top1_hit    1 when the first-ranked column in THE ORDER (lowest column on a tie) is gold: rank 1 of lamp_topk_labels
 *   has_nan     1 when the row holds a NaN score; the row is still ranked, NaN lowest
 * Per row, fp64:
 *   lrap  (row_lrap, nullable, [n_rows]) = (1 / n_p) sum_p pos_p / rank_p, every quotient in fp64, added in an order that
 *         the row alone fixes (its L and its gold columns); 1.0 for an empty row (sklearn's convention; a full row gives 1)
 *   rloss = misordered / (n_p n_n), 0 when n_p n_n = 0
 *   auc   = 1 - (misordered - tied / 2) / (n_p n_n), for rows with 0 < n_p < L only: roc_auc_score of that row
 * Dataset outputs (device):
 *   sums   fp64 [3]:  lrap_sum, rloss_sum, auc_sum (auc over the rows with both classes)
 *   counts int64 [5]: coverage_sum, top1_hits, n_with_gold (n_p > 0), n_with_both (0 < n_p < L), n_rows_with_nan
 * so that LRAP = lrap_sum / n_rows, coverage_error = coverage_sum / n_rows, ranking_loss = rloss_sum / n_rows, one_error =
 * 1 - top1_hits / n_rows (1 - P@1 of lamp_rank_at_k) and instance AUC = auc_sum / n_with_both.  Per-row terms are written to
 * the workspace first and added in an order fixed by n_rows alone: the same bits from run to run; the integer outputs are
 * also invariant under a permutation of the rows.  A row's results do not depend on n_rows, its position, the strides or the
 * padding.  The figures describe the matrix given: probabilities that saturate to exactly 0 or 1 tie where their logits did
 * not.  L <= 32768, n_rows < 2^31, 64-bit row offsets; every score and target is read once; no atomics, nothing allocated
 * or synchronised; the kernel chosen is a function of L alone.  The workspace needs no alignment.
 * Validation before any launch, in this order: LAMP_E_DIMS (a non-positive size, ld_scores < L, ld_targets < L),
 * LAMP_E_NULL (any pointer but row_counts and row_lrap), LAMP_E_UNSUPPORTED (L > 32768, n_rows >= 2^31), LAMP_E_WORKSPACE.
 * lamp_label_ranking_workspace_bytes is 0 for a request that is not served. */
size_t lamp_label_ranking_workspace_bytes(int64_t n_rows, int32_t L);
int lamp_label_ranking(const float* scores, int64_t ld_scores, const float* targets, int64_t ld_targets, int64_t n_rows,
                       int32_t L, double* sums, int64_t* counts, int32_t* row_counts, double* row_lrap, void* workspace,
                       size_t workspace_bytes, lamp_stream_t stream);

/* ---- the training step around the model (train.py:37-48, main.py:99) ------------------------------------------------ */

/* train.py:37-44 forward AND backward in one launch: F.sigmoid(pred), F.binary_cross_entropy_with_logits(.., reduction='mean')
 * of the final prediction and of every int_preds intermediate, the weighted sum `loss` and its `loss.backward()` down to the
 * logits.  logits / dlogits / weights: HOST arrays of n_mats (<= 8) device matrices [n_rows, L] (contiguous) and their loss
 * weights (1 for the final prediction = matrix 0, int_pred_weight for the others); targets [n_rows, L].
 *   probs[r * ld_probs + i]            = sigmoid(logits[0][r, i])                          (nullable; ld_probs >= L)
 *   dlogits[k][r, i]                   = weights[k] * (sigmoid(x) - t) / (n_rows * L)      (array and entries nullable)
 *   row_loss[k * ld_row_loss + r]      = sum_i max(x,0) - x*t + log1p(exp(-|x|)),  x = logits[k][r, i], t = targets[r, i]
 * The 'mean' of matrix k is sum_r row_loss[k, r] / (n_rows * L), taken by the caller.  Every sum runs in an order fixed by L
 * alone (no atomics): a row's probabilities and loss sums do not depend on the batch it is in, and neither do its gradients
 * up to the 1 / (n_rows * L) factor.  A NaN logit gives NaN in its own row only.  n_rows * L may pass 2^32 bytes (64-bit row offsets;
 * lamp_multilabel_loss_train likewise); (n_rows + 3) / 4 >= 2^31 is LAMP_E_UNSUPPORTED. */
int lamp_bce_logits_train(const float* const* logits, const float* weights, float* const* dlogits, int32_t n_mats,
                          const float* targets, int64_t n_rows, int32_t L, float* probs, int64_t ld_probs, float* row_loss,
                          int64_t ld_row_loss, lamp_stream_t stream);

/* lamp_bce_logits_train with an objective for imbalanced label sets: per-label positive weights, focal loss (Lin et al. 2017)
 * and asymmetric loss (Ridnik et al. 2021) are members of one family.  For logit x, target t, s = sigmoid(x), ns = sigmoid(-x),
 * label column j, g+ = gamma_pos, g- = gamma_neg, m = clip, w_j = pos_weight[j] (1 without pos_weight):
 *   l+(x)  = - ns^g+ log s                                   (positives)
 *   p      = max(s - m, 0)
 *   l-(x)  = - p^g- log(1 - p)                               (negatives; 1 - p = ns + m where s > m)
 *   loss   = t w_j l+  +  (1 - t) l-
 *   dl+/dx = - ns^g+ (ns - g+ s log s)
 *   dl-/dx =   s ns (p^g- / (1 - p) - g- p^(g- - 1) log(1 - p))   where s > m, else 0
 * with x^0 = 1, 0^0 included.  g+ = g- = 0, m = 0, no pos_weight: the BCE above.  g+ = g- = gamma, m = 0: focal loss, its
 * alpha through w = alpha / (1 - alpha).  The published asymmetric setting is g+ = 0, g- = 4, m = 0.05.  A target inside
 * (0, 1) mixes the two branches as written.
 *   probs[r * ld_probs + i]            = sigmoid(logits[0][r, i])            (the same bits as lamp_bce_logits_train gives)
 *   dlogits[k][r, i]                   = weights[k] * d loss / dx / (n_rows * L)
 *   row_loss[k * ld_row_loss + r]      = sum_i loss(logits[k][r, i], targets[r, i])
 * Same arguments, geometry and order of summation as lamp_bce_logits_train: a row's numbers do not depend on its batch.
 * log s and log ns are taken from x (min(x, 0) - log1p(exp(-|x|)), -max(x, 0) - log1p(exp(-|x|))), so ns log ns is 0, not
 * NaN, where ns underflows at a large finite x; the powers are exp(g log .); with m > 0, log(1 - p) = log1p(-p).
 * opts == NULL, or gamma_pos = gamma_neg = clip = 0 with pos_weight NULL, IS lamp_bce_logits_train: the same kernel, the same
 * bits.  Validated before any launch, in this order: LAMP_E_DIMS and LAMP_E_NULL as lamp_bce_logits_train, then
 * LAMP_E_UNSUPPORTED: an exponent outside {0} u [1, 16] (between 0 and 1 the gradient is unbounded at p = 0), a non-finite
 * parameter, clip outside [0, 1), reserved != 0, n_mats > 8.
 * A NaN logit makes its own gradient element and its row's loss NaN, and nothing else.  A +-inf logit may give inf or NaN in
 * its own element and row only.  The values of pos_weight are the caller's responsibility (a NaN or inf weight reaches every
 * row's loss through its column). */
typedef struct lamp_loss_options {
    float gamma_pos, gamma_neg, clip;
    int32_t reserved;          /* 0 */
    const float* pos_weight;   /* L floats on the device, or NULL */
} lamp_loss_options;
int lamp_multilabel_loss_train(const float* const* logits, const float* weights, float* const* dlogits, int32_t n_mats,
                               const float* targets, int64_t n_rows, int32_t L, float* probs, int64_t ld_probs, float* row_loss,
                               int64_t ld_row_loss, const lamp_loss_options* opts, lamp_stream_t stream);

/* lamp_bce_logits_train with a RANKING objective: a row's positives are to score above its negatives.  Same leading arguments
 * and conventions (<= 8 matrices, probs through ld_probs, row_loss through ld_row_loss, 64-bit row offsets, the caller's
 * stream, no workspace, no allocation, no synchronisation).  For one row with logits x: P = {i : t_i > 0.5}, N = the other
 * columns (the comparison as written: a NaN target is a negative; a target that is neither 0 nor 1 is the caller's business),
 * n_p = |P|, n_n = |N|.  The ranking term R of the row:
 *   LAMP_RANK_LSEP (Li et al., CVPR 2017)   R = log(1 + sum_p sum_n exp(x_n - x_p)), evaluated as softplus(z),
 *       z = LSE_{n in N}(x_n) + LSE_{p in P}(-x_p): O(L) per row, no overflow (logits of +-1e4 give finite numbers);
 *       dR/dx_n = sigmoid(z) exp(x_n - LSE_N),  dR/dx_p = -sigmoid(z) exp(-x_p - LSE_P).  Any L is served.
 *   LAMP_RANK_HINGE      R = 1 / (n_p n_n) sum_p sum_n max(0, a_pn),  a_pn = margin + (x_n - x_p): the fp32 difference FIRST,
 *       then the margin added to it -- that order decides on which side of the kink a pair lands.  A pair is active iff
 *       a_pn > 0 (the subgradient at a_pn = 0 is 0); dR/dx_n = (active pairs of n) / (n_p n_n), dR/dx_p = -(those of p) / (n_p n_n).
 *   LAMP_RANK_LOGISTIC   R = 1 / (n_p n_n) sum_p sum_n softplus(x_n - x_p)  (max(d, 0) + log1p(exp(-|d|)));
 *       dR/dx_n = sum_p sigmoid(x_n - x_p) / (n_p n_n),  dR/dx_p = -sum_n sigmoid(x_n - x_p) / (n_p n_n).
 * HINGE and LOGISTIC walk the pairs that exist: the row's positives and negatives are compacted in column order and every
 * element loops over the opposite class only, n_p n_n evaluations per row and direction (loss + negatives' gradients,
 * positives' gradients); L <= 4096 is served.  An empty class (n_p = 0 or n_n = 0): R = 0 and a zero ranking gradient; the
 * row still counts in n_rows.  With beta = bce_weight the trained loss of matrix k is
 *   loss_k = 1 / n_rows sum_r [ R_r + beta / L sum_i bce(x_ri, t_ri) ]       (bce as lamp_bce_logits_train has it)
 *   dlogits[k][r, i]               = weights[k] * d loss_k / dx
 *   row_loss[k * ld_row_loss + r]  = R_r + beta * bce_row_r / L              (the caller divides by n_rows, NOT by n_rows * L)
 *   probs[r * ld_probs + i]        = sigmoid(logits[0][r, i])                (lamp_bce_logits_train's bits, every kind and beta)
 * Row sums, the LSE sums and the mixing of the two terms run in double and are rounded once.  Every sum runs in an order
 * fixed by L and the row's own target pattern (no atomics): a row's probs and row_loss are the same bits in any batch, its
 * gradients up to the 1 / n_rows factor, and everything from run to run.  A NaN logit makes its row's loss and all of its
 * row's gradients NaN and touches no other row (probs: its own element); a +-inf logit may give inf or NaN in its own row only.
 * Validated before any launch, in this order: LAMP_E_DIMS and LAMP_E_NULL as lamp_bce_logits_train (opts == NULL is
 * LAMP_E_NULL), then LAMP_E_UNSUPPORTED: an unknown kind, a non-finite or negative margin or bce_weight, margin != 0 outside
 * HINGE, reserved != 0, n_mats > 8, L > 4096 for HINGE and LOGISTIC, n_rows >= 2^31. */
enum lamp_rank_kind { LAMP_RANK_LSEP = 1, LAMP_RANK_HINGE = 2, LAMP_RANK_LOGISTIC = 3 };
typedef struct lamp_rank_loss_options {
    int32_t kind;        /* lamp_rank_kind */
    float   margin;      /* HINGE only: finite, >= 0; must be 0 for the other two */
    float   bce_weight;  /* beta >= 0, finite: weight of the row's mean BCE mixed in (0 = the ranking term alone) */
    int32_t reserved;    /* 0 */
} lamp_rank_loss_options;
int lamp_rank_loss_train(const float* const* logits, const float* weights, float* const* dlogits, int32_t n_mats,
                         const float* targets, int64_t n_rows, int32_t L, float* probs, int64_t ld_probs,
                         float* row_loss, int64_t ld_row_loss, const lamp_rank_loss_options* opts, lamp_stream_t stream);

/* lamp_embed_bwd with a fixed summation order, for a training epoch that must be reproducible bit for bit (the embedding
 * gradient feeds optimizer.step(), train.py:47-48): d_emb[src_seq[t], :] += dout[t, :], the rows of a repeated token added in
 * ascending position order by ONE writer per table row -- no atomics.  Same arguments and contract as lamp_embed_bwd; the
 * two differ in the last bits where a token repeats.  Every wave scans the token ids before its own position for an earlier
 * occurrence (n_tokens^2 / 128 id loads per launch on average): meant for a batch's tokens, not for a corpus. */
int lamp_embed_bwd_ordered(const int64_t* src_seq, int64_t n_tokens, const float* dout, int32_t d_model, int32_t n_vocab,
                           int64_t pad_idx, float* d_emb, lamp_stream_t stream);

/* optimizer.step() (train.py:48) for every parameter in one launch per 72 table entries.  entries: HOST array of n device
 * tensors (fp32, 4-byte aligned, any numel >= 0; 16-byte accesses when all of an entry's pointers allow it).
 *   LAMP_OPTIM_ADAM: torch.optim.Adam as main.py:99 builds it (no weight decay, no amsgrad), `step` = this update's 1-based
 *     count:  m = m + (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g g;
 *             w = w - lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *   LAMP_OPTIM_SGD:  w = w - lr * g  (exp_avg / exp_avg_sq unused, may be NULL)
 * The hyper-parameters are doubles: 1 - beta and the bias corrections are taken on the host in double, as torch does,
 * and rounded to fp32 once.  Elementwise: bit-identical from run to run.  An entry may pass 2^32 bytes (a workgroup's offset is its
 * 64-bit chunk index times 4096); 2^31 chunks in one launch's entries is LAMP_E_UNSUPPORTED (lamp_optim_step_ext and lamp_grad_norm likewise). */
enum lamp_optim_kind { LAMP_OPTIM_ADAM = 0, LAMP_OPTIM_SGD = 1 };
typedef struct lamp_optim_entry {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
} lamp_optim_entry;
int lamp_optim_step(const lamp_optim_entry* entries, int32_t n, int32_t kind, int64_t step, double lr, double beta1,
                    double beta2, double eps, lamp_stream_t stream);

/* The global L2 norm of every gradient of a table (entries[i].grad / .numel; the other members are not read), for gradient
 * clipping and for the decision "is this batch's gradient finite" taken on the device.  Deterministic, no atomics:
 *   stage 1  one workgroup per 4096-element chunk of an entry (lamp_optim_step's chunking).  Every element is squared and
 *            added in fp64 -- the square of an fp32 number is exact there, nothing overflows below |g| = 3.4e38 and nothing
 *            underflows -- lanes and waves are folded in a fixed order, and the workgroup writes one double into `workspace`.
 *            72 entries per launch; a longer table takes several launches.
 *   stage 2  ONE workgroup, whatever the table's length: lane t adds partials t, t + 256, ... in ascending order, lanes and
 *            waves fold as in stage 1, and one lane writes the 4-float DEVICE record
 *              grad_state = { norm, scale, finite, 0 }:   norm = float(sqrt(sum));
 *              scale = min(1, max_norm * (1 / (norm + 1e-6))) in fp32, torch.nn.utils.clip_grad_norm_'s own expression
 *                      (its `max_norm / tensor` is reciprocal().mul()); 1 when max_norm < 0 (LAMP_GRAD_NORM_NO_CLIP); a NaN
 *                      norm gives a NaN scale, an infinite one 0, as in torch;
 *              finite = 1.0f when norm is finite, else 0.0f.
 *            skipped (device int32, may be NULL): incremented by one when finite == 0.
 * The record is bit-identical from run to run on the same table; it depends on the order of the entries and on their
 * alignment (16-byte aligned gradients are read four at a time) in the last bits of the fp64 sum, far below one fp32 ulp.
 * Zero-numel entries are skipped; gradients are 4-byte aligned.  lamp_grad_norm_workspace_bytes() is exact: 8 bytes per
 * chunk (0 for a table it refuses).  Validated before any launch: LAMP_E_DIMS (n < 0, a negative numel), LAMP_E_NULL
 * (entries, grad_state, a gradient, the workspace), LAMP_E_UNSUPPORTED (a NaN max_norm, 2^31 chunks), LAMP_E_ALIGN,
 * LAMP_E_WORKSPACE (a workspace smaller than the query's answer). */
#define LAMP_GRAD_NORM_NO_CLIP (-1.0)
size_t lamp_grad_norm_workspace_bytes(const lamp_optim_entry* entries, int32_t n);
int lamp_grad_norm(const lamp_optim_entry* entries, int32_t n, double max_norm, void* workspace, size_t workspace_bytes,
                   float* grad_state, int32_t* skipped, lamp_stream_t stream);

/* lamp_optim_step with the training-loop controls of a Transformer-style model, still one launch per 72 entries.  ext NULL,
 * or an ext that asks for nothing, IS lamp_optim_step (the same kernel, the same bits).  Per element, in this order:
 *   grad_state (DEVICE, the record of lamp_grad_norm; NULL = no clipping): g = g * scale, rounded as torch's in-place mul_
 *     (no contraction).  The gradient buffer is read once and NOT rewritten.
 *   entry_weight_decay (HOST array of n floats >= 0, NULL = 0 everywhere; it travels in the kernel arguments):
 *     flag unset: g = g + wd * w, before the moments (torch's weight_decay);  LAMP_OPTIM_DECOUPLED_DECAY (Adam only):
 *     w = w * (1 - lr * wd) before the update, the factor taken in double on the host (torch.optim.AdamW).  An entry with
 *     decay 0 takes exactly lamp_optim_step's arithmetic (an infinite weight stays what it is), so biases, LayerNorm
 *     parameters and a label bias with -inf entries share the launch.
 *   momentum (LAMP_OPTIM_SGD only, in [0, 1)): buf = momentum * buf + g; w = w - lr * buf, the buffer in the entry's exp_avg
 *     slot.  A zero buffer on the first step is torch's "first step copies the gradient".  No nesterov, no dampening.
 *   LAMP_OPTIM_SKIP_NONFINITE (needs grad_state): when the record's finite is 0 the launch writes NOTHING -- parameters and
 *     moments keep their bits.  Without the flag a non-finite norm does what torch's arithmetic does: the scale is NaN (or 0
 *     against an infinite gradient) and NaN spreads into every parameter and moment of the table.
 * `step` is the caller's count; a skipped launch does not know it was skipped.  Refused before any launch: LAMP_E_DIMS
 * (n < 0, numel < 0, Adam with step < 1), LAMP_E_UNSUPPORTED (unknown kind or flag bits, reserved != 0, momentum outside
 * [0, 1) or with Adam, decoupled decay with SGD, a skip without grad_state, a negative or non-finite decay), LAMP_E_NULL,
 * LAMP_E_ALIGN. */
#define LAMP_OPTIM_DECOUPLED_DECAY 1
#define LAMP_OPTIM_SKIP_NONFINITE 2
typedef struct lamp_optim_ext {
    const float* entry_weight_decay;   /* HOST, n floats, or NULL */
    const float* grad_state;           /* DEVICE, 4 floats, or NULL */
    double momentum;
    int32_t flags;
    int32_t reserved;                  /* 0 */
} lamp_optim_ext;
int lamp_optim_step_ext(const lamp_optim_entry* entries, int32_t n, int32_t kind, int64_t step, double lr, double beta1,
                        double beta2, double eps, const lamp_optim_ext* ext, lamp_stream_t stream);

/* An average of the weights (EMA, SWA) kept beside them, in one launch per 72 table entries, after optimizer.step().
 * entries: lamp_optim_step's HOST table; `param` is the live weight and is READ ONLY, `exp_avg` is the average and is updated
 * in place, `grad` and `exp_avg_sq` are ignored (may be NULL), `numel` counts elements.  weight in [0, 1] is rounded to fp32
 * once on the host.  Per element, without contraction, torch's lerp (what _foreach_lerp_ does for
 * torch.optim.swa_utils.get_ema_multi_avg_fn / get_swa_multi_avg_fn), a = the average, p = the weight:
 *     w < 0.5:  a = a + w (p - a)          otherwise:  a = p - (p - a)(1 - w)
 * with three defined edges:
 *   w == 1   copies the 32-bit patterns of p (the first update of an average; NaN payloads included);
 *   w == 0   launches nothing;
 *   p == a   leaves a as it is: a label bias holds -inf where an edge never moves, and -inf - -inf would make the average
 *            NaN there (torch's lerp does; this does not).
 * A NaN or an infinity anywhere else behaves as fp32 arithmetic does and touches its own element only.
 * lamp_optim_step's geometry: one 256-lane workgroup per 4096-element chunk of an entry, 16-byte accesses when both pointers
 * of the entry allow them (the last numel % 4 elements by single lanes), 4-byte accesses otherwise; zero-numel entries are
 * skipped; an entry may pass 2^32 bytes.  No LDS, no atomics, no workspace, nothing synchronised.  Elementwise: bit-identical
 * from run to run and independent of the table an entry travels in.  An entry whose param and exp_avg are the SAME pointer
 * is a no-op.  Refused before any launch: LAMP_E_DIMS (n < 0, numel < 0), LAMP_E_NULL (entries; param or exp_avg of a
 * non-empty entry), LAMP_E_ALIGN (a pointer that is not 4-byte aligned), LAMP_E_UNSUPPORTED (a weight outside [0, 1] or NaN,
 * an entry of 2^31 chunks, a param and an exp_avg that overlap without being identical). */
int lamp_weight_average(const lamp_optim_entry* entries, int32_t n, double weight, lamp_stream_t stream);

/* Exchanges the 32-bit patterns of `param` and `exp_avg` of every entry (evaluate the average in place, then swap back): NaN
 * payloads are preserved and two calls are the identity.  Table, geometry and refusals are lamp_weight_average's (no weight).
 * The caller bumps the version counters of what it swapped (lamp_amd/optim.py: WeightAverage.swap). */
int lamp_weight_swap(const lamp_optim_entry* entries, int32_t n, lamp_stream_t stream);

/* ---- per-kernel timing (HIP events on the launch stream; used by bench.py's roofline) ------ */
enum lamp_kernel_class {
    LAMP_K_EMBED = 0, LAMP_K_GEMM = 1, LAMP_K_ATTN = 2, LAMP_K_LAYERNORM = 3, LAMP_K_DIAG = 4,
    LAMP_K_COUNT = 5
};
int lamp_prof_enable(int32_t on);  /* bracket every launch with a hipEvent pair while on */
int lamp_prof_reset(void);
/* Synchronises the recorded events and returns, per class: launches, summed milliseconds, and the
 * summed algorithmic FLOPs and bytes of those launches (as the launcher computed them). */
int lamp_prof_read(int32_t kernel_class, int64_t* launches, double* total_ms, double* flops,
                   double* bytes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* LAMP_HIP_H */

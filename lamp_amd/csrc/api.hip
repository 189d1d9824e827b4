// C-ABI entry points of liblamp_hip.so (see include/lamp_hip.h) and the whole-forward launcher.
//
// Host-side only: argument validation, workspace carving and the launch sequence.  No device
// memory is allocated here, no pointer is retained, nothing synchronises (except lamp_prof_read).
#include <algorithm>
#include <mutex>
#include <vector>

#include "lamp_kernels.h"

namespace lamp {

// ------------------------------------------------------------------ profiling
namespace {
struct ProfRec {
    int cls;
    double flops, bytes;
    hipEvent_t e0, e1;
};
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof;          // records in use
std::vector<hipEvent_t> g_event_pool; // recycled events
constexpr size_t PROF_MAX = 1 << 16;

hipEvent_t take_event() {
    if (!g_event_pool.empty()) {
        hipEvent_t e = g_event_pool.back();
        g_event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}
}  // namespace

ProfScope::ProfScope(int kernel_class, double flops, double bytes, hipStream_t stream) : idx(-1), s(stream) {
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof_on || g_prof.size() >= PROF_MAX) return;
    ProfRec r{kernel_class, flops, bytes, take_event(), take_event()};
    if (!r.e0 || !r.e1) return;
    (void)hipEventRecord(r.e0, s);
    idx = int(g_prof.size());
    g_prof.push_back(r);
}

ProfScope::~ProfScope() {
    if (idx < 0) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (idx < int(g_prof.size())) (void)hipEventRecord(g_prof[idx].e1, s);
}

// ------------------------------------------------------------------ helpers
#define LAMP_CK(expr)            \
    do {                         \
        int _e = (expr);         \
        if (_e != 0) return _e;  \
    } while (0)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A workspace is a list of regions of per_sample * mb + fixed floats, each rounded up to 256 bytes.  One layout function
// per workspace declares its regions in order: run over a null base it only sizes them, over the caller's workspace it
// carves them.  `bound` is affine in the micro-batch and never below what carving that many samples takes: its fixed part
// holds one 256-byte alignment allowance per region.
struct Carver {
    char* base;                 // nullptr: sizing only
    size_t mb;                  // samples the regions are carved for
    size_t off = 0;             // bytes taken so far
    size_t per = 0, fixed = 0;  // bytes per sample; fixed bytes
    template <class P>
    void take(P** p, size_t per_sample_floats, size_t fixed_floats = 0) {
        if (p) *p = base ? reinterpret_cast<P*>(base + off) : nullptr;
        off += align_up((per_sample_floats * mb + fixed_floats) * sizeof(float), 256);
        per += per_sample_floats * sizeof(float);
        fixed += fixed_floats * sizeof(float) + 256;
    }
    size_t bound(size_t n) const { return per * n + fixed; }
};

// The residual of a GEMM as a gather from the embedding tables (GemmParams::rg_tok): the encoder's first layer, whose input rows
// are then never written (EmbedFold::row_tok).
struct ResGather {
    const int* tok;
    const int* pos;
    const float* emb;
    const float* pos_table;
};

// lamp_fwd_options.flags -> LAMP_PREC_*, or -1 when both matmul flags are set
static inline int fwd_matmul_prec(const lamp_fwd_options* o) {
    const int f = o ? o->flags & (LAMP_FWD_MATMUL_BF16X3 | LAMP_FWD_MATMUL_BF16X6) : 0;
    return f == 0 ? LAMP_PREC_FP32 : f == LAMP_FWD_MATMUL_BF16X3 ? LAMP_PREC_BF16X3 : f == LAMP_FWD_MATMUL_BF16X6 ? LAMP_PREC_BF16X6 : -1;
}

// prec: LAMP_PREC_* -- which kernel family multiplies (gemm.hip, or gemm_split.hip's bf16x3 / bf16x6 split products)
// Wp (nullable; entries nullable): lamp_pack_weight(W[i], format 0) per segment, for the fp32 tile GEMM's packed-W tile (GemmParams::Wp)
static int linear(const float* A, int64_t M, int K, int64_t lda, const float* const* W, int nseg, int N,
                  int64_t ldw, const float* const* bias, const float* R, int64_t ldr, int relu,
                  float* const* C, int64_t ldc, int prec, hipStream_t s, const int* m_dev = nullptr,
                  const float* A_dense = nullptr, const ResGather* rg = nullptr, const float* const* Wp = nullptr) {
    GemmParams p{};
    p.A = A; p.lda = lda; p.M = M; p.K = K; p.N = N; p.nseg = nseg; p.ldw = ldw; p.ldc = ldc;
    p.R = R; p.ldr = ldr; p.relu = relu; p.m_dev = m_dev; p.A_dense = A_dense;
    if (rg) {
        p.R = nullptr;
        p.rg_tok = rg->tok; p.rg_pos = rg->pos; p.rg_emb = rg->emb; p.rg_pos_table = rg->pos_table;
    }
    for (int i = 0; i < nseg; ++i) {
        p.W[i] = W[i];
        p.Wp[i] = Wp ? Wp[i] : nullptr;
        p.bias[i] = bias ? bias[i] : nullptr;
        p.C[i] = C[i];
    }
    if (prec == LAMP_PREC_BF16X3) return launch_gemm_split(p, 3, s);
    if (prec == LAMP_PREC_BF16X6) return launch_gemm_split(p, 6, s);
    return launch_gemm(p, s);
}

// act: the activation of the attention the mask goes to (a score bias is a softmax matter)
static int check_mask(const lamp_mask* m, int act = LAMP_ATTN_SOFTMAX) {
    if (!m) return 0;
    if (m->kind != LAMP_MASK_NONE && m->kind != LAMP_MASK_U8 && m->kind != LAMP_MASK_KEY_TOKENS_I64 &&
        m->kind != LAMP_MASK_BITS_U32 && m->kind != LAMP_MASK_BIAS_F32)
        return LAMP_E_UNSUPPORTED;
    if (m->kind != LAMP_MASK_NONE && !m->ptr) return LAMP_E_NULL;
    if (m->kind == LAMP_MASK_BIAS_F32) {
        // dense and softmax only: no tile list (not even one the map write-out would ignore), no sparse / ragged route
        if (act == LAMP_ATTN_SIGMOID || m->tile_list || (m->flags & (LAMP_MASK_SPARSE_ROWS | LAMP_MASK_SELF_RAGGED)))
            return LAMP_E_UNSUPPORTED;
        if (!aligned16(m->ptr) || (m->stride_q & 3) || (m->stride_b & 3)) return LAMP_E_ALIGN;
    }
    return 0;
}

// The mask fields of AttnParams from a lamp_mask (nullable); set a.P first: the tile list only serves calls without maps.
static void attn_mask(AttnParams& a, const lamp_mask* mask) {
    a.mask_kind = mask ? mask->kind : LAMP_MASK_NONE;
    a.mask = mask ? mask->ptr : nullptr;
    a.m_sb = mask ? mask->stride_b : 0;
    a.m_sq = mask ? mask->stride_q : 0;
    a.tiles = (mask && !a.P) ? mask->tile_list : nullptr;
    a.tiles_stride = mask ? mask->tile_list_stride : 0;
    a.sparse_rows = mask && (mask->flags & LAMP_MASK_SPARSE_ROWS) != 0;
    a.self_ragged = mask && (mask->flags & LAMP_MASK_SELF_RAGGED) != 0;
    a.allowed_pairs = mask ? mask->allowed_pairs : 0;
}

// The Q / K / V projections of one attention block; a null output is not projected.  Projections that share their input
// go out as segments of ONE launch (same bits as one launch each): K with V when both read the same rows at the same
// width, Q with both when it reads those rows too.  m_dev / A_dense (GemmParams): the key / value rows are packed.
static int project_qkv(const lamp_mha_weights& w, int d, int dk, int dv, const float* xq, int64_t Mq, float* Q,
                       const float* xk, const float* xv, int64_t Mk, float* K, float* V, int prec, hipStream_t s,
                       const int* m_dev, const float* A_dense, const float* const* Wp = nullptr) {
    const int hdk = w.n_head * dk, hdv = w.n_head * dv;
    const bool one_kv = K && V && xk == xv && hdk == hdv;
    const bool one_qkv = one_kv && Q && xq == xk && Mq == Mk && !m_dev;
    const float* W[3] = {w.w_qs, w.w_ks, w.w_vs};
    float* C[3] = {Q, K, V};
    const float* const* P1 = Wp ? Wp + 1 : nullptr;   // Wp: packs of {w_qs, w_ks, w_vs}, entries nullable (a launch needs all of its own)
    const float* const* P2 = Wp ? Wp + 2 : nullptr;
    if (Q) LAMP_CK(linear(xq, Mq, d, d, W, one_qkv ? 3 : 1, hdk, d, nullptr, nullptr, 0, 0, C, hdk, prec, s, nullptr, nullptr, nullptr, Wp));
    if (one_qkv) return 0;
    if (one_kv) return linear(xk, Mk, d, d, W + 1, 2, hdk, d, nullptr, nullptr, 0, 0, C + 1, hdk, prec, s, m_dev, A_dense, nullptr, P1);
    if (K) LAMP_CK(linear(xk, Mk, d, d, W + 1, 1, hdk, d, nullptr, nullptr, 0, 0, C + 1, hdk, prec, s, m_dev, A_dense, nullptr, P1));
    if (V) LAMP_CK(linear(xv, Mk, d, d, W + 2, 1, hdv, d, nullptr, nullptr, 0, 0, C + 2, hdv, prec, s, m_dev, A_dense, nullptr, P2));
    return 0;
}

// PositionwiseFeedForward.forward (lamp/SubLayers.py:133-142).
struct FfnParams {
    const float* x;   // [M, d]; out may alias it
    int64_t M;
    int d, dff;
    const lamp_ffn_weights* w;
    float *out, *hidden;
    const float* w_out = nullptr;   // fused read-out of the last decoder block: the final LayerNorm writes logits, not out
    int n_labels = 0;
    float* logits = nullptr;
    // Packed encoder rows (ragged batches): the live row count in device memory (M is the upper bound the launches are sized
    // for); with `scatter` this is the LAST encoder layer, whose LayerNorm also writes the padded [nb, T, d] encoder output
    // `y_flat` (see layernorm_kernel<.., RG = 2>).
    const int* rows_dev = nullptr;
    const SeqPlan* scatter = nullptr;
    int nb = 0, T = 0;
    float* y_flat = nullptr;
    // relu(x W1^T + b1) is already in `hidden` (the encoder's first layer with W1 folded into the embedding tables,
    // pointwise.hip: gather_row): the first GEMM is not launched, and with `rg` the residual is gathered (x does not exist)
    bool hidden_ready = false;
    const ResGather* rg = nullptr;
    int prec = LAMP_PREC_FP32;   // matmul precision of the two GEMMs (the forward's LAMP_FWD_MATMUL_* flags)
    const float *w1_pack = nullptr, *w2_pack = nullptr;   // lamp_gemm_packs: format-0 packs of w1 / w2 for the packed-W tile
};

static int ffn_core(const FfnParams& f, hipStream_t s) {
    const lamp_ffn_weights& w = *f.w;
    const int d = f.d, dff = f.dff;
    if (!w.w1 || !w.b1 || !w.w2 || !w.b2 || !w.ln_g || !w.ln_b) return LAMP_E_NULL;
    if (f.rg && !f.hidden_ready) return LAMP_E_UNSUPPORTED;
    if (!f.hidden_ready) {
        const float* W[1] = {w.w1};
        const float* b[1] = {w.b1};
        float* C[1] = {f.hidden};
        const float* P[1] = {f.w1_pack};
        LAMP_CK(linear(f.x, f.M, d, d, W, 1, dff, d, b, nullptr, 0, 1, C, dff, f.prec, s, f.rows_dev, nullptr, nullptr, P));
    }
    {
        const float* W[1] = {w.w2};
        const float* b[1] = {w.b2};
        float* C[1] = {f.out};
        const float* P[1] = {f.w2_pack};
        LAMP_CK(linear(f.hidden, f.M, dff, dff, W, 1, d, dff, b, f.x, d, 0, C, d, f.prec, s, f.rows_dev, nullptr, f.rg, P));
    }
    LayerNormParams ln{f.out, f.M, d, w.ln_g, w.ln_b, f.out};
    if (f.scatter) {
        ln.M = int64_t(f.nb) * f.T; ln.scatter = f.scatter; ln.T = f.T; ln.y_flat = f.y_flat;
    } else if (f.rows_dev) {
        ln.m_dev = f.rows_dev;
    } else if (f.w_out) {   // the final decoder LayerNorm also produces the logits and its output row is not stored
        ln.y = nullptr; ln.w_out = f.w_out; ln.n_labels = f.n_labels; ln.logits = f.logits;
    }
    return launch_layernorm(ln, s);
}

// Scratch of one MultiHeadAttention call.
struct MhaScratch {
    float *Q, *K, *V, *A;
    float* S = nullptr;    // (h*B, lq, lk) score scratch, only for d_k or d_v > 128 (attention_general.hip)
    float* lse = nullptr;  // [h][B][lq] row log-sum-exp: lets requested attention maps come from the single-pass kernel
    int* plan_ints = nullptr;  // the SeqPlan of a key-token mask when the caller did not bring one
};
static inline SeqPlan plan_from(int* ints, int64_t B, int T) {
    return SeqPlan{ints, ints + B, ints + 2 * B, ints + 3 * B + 1, reinterpret_cast<unsigned*>(ints + 3 * B + 3), (T + 31) / 32, nullptr};
}
static inline bool wide_heads(int dk, int dv) { return dk > 128 || dv > 128; }
// the SeqPlan of c.mb samples of T keys: 3 mb + 3 ints and mb words of pad bits
static inline void take_plan(Carver& c, int** ints, int T) { c.take(ints, 3 + size_t((T + 31) / 32), 3); }

// The scratch of an attention call with lq queries and lk keys per sample (c.mb samples).  `plan`: with the plan_ints region.
static void mha_layout(Carver& c, MhaScratch& sc, int lq, int lk, int h, int dk, int dv, bool plan) {
    c.take(&sc.Q, size_t(lq) * h * dk);
    c.take(&sc.K, size_t(lk) * h * dk);
    c.take(&sc.V, size_t(lk) * h * dv);
    c.take(&sc.A, size_t(lq) * h * dv);
    if (wide_heads(dk, dv)) c.take(&sc.S, size_t(h) * lq * lk);
    c.take(&sc.lse, size_t(h) * lq);
    if (plan) take_plan(c, &sc.plan_ints, lk);
}

// One MultiHeadAttention.forward (lamp/SubLayers.py:77-121) on B samples: mha_attend, then (with `out`) mha_tail.
struct MhaCall {
    const float* xq;   // [B, lq, d] queries, also the residual; `out` may alias it unless xq_shared
    const float* xkv;  // [B, lk, d] keys and values
    int B, lq, lk, d, dk, dv;
    const lamp_mha_weights* w;
    const lamp_mask* mask;
    float* out;        // nullptr: the attention map only (the reference's dead encoder self-attention)
    float* attn;       // nullable maps (h * P_batch, lq, lk): this call's samples are P_b0 + b
    int P_batch = 0, P_b0 = 0;
    bool xq_shared = false;            // xq is ONE [lq, d] block used by every sample (decoder layer 0: the label embeddings,
                                       // SURVEY.md G11): its projection is computed once, the residual read modulo lq
    const float* q_ready = nullptr;    // the query projection, already computed
    bool kv_ready = false;             // the scratch's K / V already hold this call's projections (see forward)
    const SeqPlan* keys = nullptr;     // per-sample key extents of a key-token mask (ragged batches)
    bool keys_packed = false;          // xkv holds the packed token rows (keys->rows[0] of them, counted on the device)
    const float* xkv_dense = nullptr;  // with keys_packed: the padded rows, read instead when nothing was skipped
    int act = LAMP_ATTN_SOFTMAX;       // LAMP_ATTN_SIGMOID: sigmoid attention (attention_sigmoid.hip), maps in the same pass
    int prec = LAMP_PREC_FP32;         // matmul precision of the projections and of a separate-launch fc (never of the chain launch)
    const float* const* w_packs = nullptr;   // lamp_gemm_packs: format-0 packs of {w_qs, w_ks, w_vs} (entries nullable)
};


// The attention step: projections, the key plan, the attention launch.  Checks the whole call before its first launch.
static int mha_attend(const MhaCall& c, const MhaScratch& sc, hipStream_t s) {
    const lamp_mha_weights& w = *c.w;
    const int h = w.n_head, d = c.d, dk = c.dk, dv = c.dv, B = c.B, lq = c.lq, lk = c.lk;
    if (h < 1 || dk < 1 || dv < 1) return LAMP_E_DIMS;
    if (!w.w_qs || !w.w_ks || !w.w_vs || (c.out && (!w.ln_g || !w.ln_b))) return LAMP_E_NULL;
    if (h == 1 && c.out && dv != d) return LAMP_E_DIMS;  // no fc: O is added to the residual directly
    if (h > 1 && c.out && !w.fc) return LAMP_E_NULL;
    const int hdk = h * dk, hdv = h * dv;
    const bool need_v = c.out != nullptr;
    const bool kv = !c.kv_ready;
    LAMP_CK(project_qkv(w, d, dk, dv, c.xq, c.xq_shared ? lq : int64_t(B) * lq, c.q_ready ? nullptr : sc.Q, c.xkv, c.xkv,
                        int64_t(B) * lk, kv ? sc.K : nullptr, kv && need_v ? sc.V : nullptr, c.prec, s,
                        c.keys_packed ? c.keys->rows : nullptr, c.keys_packed ? c.xkv_dense : nullptr, c.w_packs));

    // A key-token mask without a plan (lamp_mha_fwd on its own): count each sample's keys here, padded layout, so that
    // the module-by-module route takes the same per-sample key split as lamp_forward -- same bits.
    const lamp_mask* mask = c.mask;
    const SeqPlan* keys = c.keys;
    SeqPlan local_plan{};
    if (!keys && mask && mask->kind == LAMP_MASK_KEY_TOKENS_I64 && sc.plan_ints && !wide_heads(dk, dv)) {
        local_plan = plan_from(sc.plan_ints, B, lk);
        LAMP_CK(launch_seq_plan(static_cast<const int64_t*>(mask->ptr), nullptr, B, lk, mask->stride_b, false, local_plan, s));
        keys = &local_plan;
    }

    AttnParams a{};
    a.Q = c.q_ready ? c.q_ready : sc.Q; a.K = sc.K; a.V = need_v ? sc.V : nullptr; a.O = need_v ? sc.A : nullptr; a.P = c.attn;
    a.scratch = sc.S;
    // maps + output: single-pass kernel (same O bits as without maps), scores normalised in place afterwards
    if (c.attn && need_v && sc.lse && c.act == LAMP_ATTN_SOFTMAX) a.lse = sc.lse;
    a.act = c.act;
    a.B = B; a.H = h; a.lq = lq; a.lk = lk; a.dk = dk; a.dv = dv;
    a.P_batch = c.P_batch > 0 ? c.P_batch : B; a.P_b0 = c.P_b0;
    a.lay.q_b = c.xq_shared ? 0 : int64_t(lq) * hdk; a.lay.q_h = dk; a.lay.q_r = hdk;
    a.lay.k_b = int64_t(lk) * hdk; a.lay.k_h = dk; a.lay.k_r = hdk;
    a.lay.v_b = int64_t(lk) * hdv; a.lay.v_h = dv; a.lay.v_r = hdv;
    a.lay.o_b = int64_t(lq) * hdv; a.lay.o_h = dv; a.lay.o_r = hdv;
    a.scale_log2e = float(1.4426950408889634 / sqrt(double(dk)));
    attn_mask(a, mask);
    if (keys && mask && mask->kind == LAMP_MASK_KEY_TOKENS_I64) {
        a.kv_len = keys->klen;
        a.kv_off = keys->off;
        if (!wide_heads(dk, dv)) {   // the plan's bit-packed copy of the same mask: one word per 32-key tile
            a.mask_kind = LAMP_MASK_BITS_U32;
            a.mask = keys->padbits;
            a.m_sb = keys->words;
            a.m_sq = 0;
        }
    }
    return launch_attn(a, s);
}

// The tail step behind mha_attend (c.out set): fc (+ residual) -> LayerNorm into c.out.  With `f`, the position-wise
// feed-forward block that follows the attention in a decoder layer (lamp/Layers.py:35-36, :40-45, reading and writing
// c.out) may run in the same launch (chain.hip, with `pk`: weights-only packed copies of (fc, w1, w2)); then *ffn_ran tells
// the caller whether it did.
static int mha_tail(const MhaCall& c, const MhaScratch& sc, const FfnParams* f, const lamp_chain_pack* pk, bool* ffn_ran,
                    hipStream_t s) {
    const lamp_mha_weights& w = *c.w;
    const int h = w.n_head, d = c.d, B = c.B, lq = c.lq, hdv = h * c.dv;
    const float* xq = c.xq;
    float* out = c.out;
    const int64_t M = int64_t(B) * lq;
    const int64_t r_mod = c.xq_shared ? lq : 0;
    if (f) *ffn_ran = false;
    if (h > 1 && f && chain_applies(M, d, hdv, f->dff, true, pk, c.xq_shared, f->w_out != nullptr)) {
        // fc (+ residual) -> LayerNorm -> W1 -> W2 (+ residual) -> LayerNorm in one launch over 16-row panels (same bits)
        *ffn_ran = true;
        return launch_chain(sc.A, hdv, hdv, xq, r_mod, M, d, w.fc, w.ln_g, w.ln_b, f->w, f->dff, f->w_out ? nullptr : out,
                            f->w_out, f->n_labels, f->logits, s, pk);
    }
    if (h > 1 && f && pk && M > 6144 && (!f->w_out || f->n_labels == lq)) {
        // Just past one chain launch's reach (6145-12288 rows: batch 69-136 at 90 labels) the tail is still faster as TWO chain
        // launches over halves of the batch -- whole samples, so that row % lq of the shared residual / read-out rows stays the
        // group-local row -- when each half fills the CUs with 24-row panels: batch 128 = 2 x 5760 rows, +6 % whole-forward
        // (48.9 k against 46.1 k samples/s).  With smaller halves (batch 96: 2 x 4320 rows) it ties, and from ~190 samples on the
        // five launches have enough tiles per GEMM to win (profiles/r05_batch_sweep.txt): both keep the separate launches.
        const int per = (B + 1) / 2, last = B - per;
        if (int64_t(per) * lq <= 6144 && int64_t(last) * lq > 4608 &&
            chain_applies(int64_t(per) * lq, d, hdv, f->dff, true, pk, c.xq_shared, f->w_out != nullptr) &&
            chain_applies(int64_t(last) * lq, d, hdv, f->dff, true, pk, c.xq_shared, f->w_out != nullptr)) {
            for (int g = 0; g < 2; ++g) {
                const int64_t r0 = int64_t(g) * per * lq, rows = int64_t(g == 0 ? per : last) * lq;
                LAMP_CK(launch_chain(sc.A + r0 * hdv, hdv, hdv, c.xq_shared ? xq : xq + r0 * d, r_mod, rows, d, w.fc, w.ln_g,
                                     w.ln_b, f->w, f->dff, f->w_out ? nullptr : out + r0 * d, f->w_out, f->n_labels,
                                     f->logits ? f->logits + r0 : nullptr, s, pk));
            }
            *ffn_ran = true;
            return 0;
        }
    }
    // the residual: added by the fc GEMM, or by the LayerNorm kernel when there is no fc (O is added directly) or when it
    // is the shared [lq, d] block (row modulo lq)
    LayerNormParams ln{h == 1 ? sc.A : out, M, d, w.ln_g, w.ln_b, out};
    if (h == 1 || c.xq_shared) { ln.residual = xq; ln.r_mod = r_mod; }
    if (h > 1) {
        const float* W[1] = {w.fc};
        float* C[1] = {out};
        LAMP_CK(linear(sc.A, M, hdv, hdv, W, 1, d, hdv, nullptr, ln.residual ? nullptr : xq, ln.residual ? 0 : d, 0, C, d, c.prec, s));
    }
    return launch_layernorm(ln, s);
}

}  // namespace lamp

using namespace lamp;

namespace {
int sdpa_impl(const float* q, const float* k, const float* v, float* out, float* attn, float* lse, int32_t B, int32_t H,
              int32_t lq, int32_t lk, int32_t d_k, int32_t d_v, float inv_temperature, const lamp_mask* mask,
                  const lamp_attn_layout* layout, lamp_stream_t stream, int act = LAMP_ATTN_SOFTMAX) {
    if (!layout) return LAMP_E_NULL;
    LAMP_CK(check_mask(mask, act));
    AttnParams a{};
    a.Q = q; a.K = k; a.V = v; a.O = out; a.P = attn; a.lse = act == LAMP_ATTN_SOFTMAX ? lse : nullptr;
    a.act = act;
    a.B = B; a.H = H; a.lq = lq; a.lk = lk; a.dk = d_k; a.dv = d_v;
    a.P_batch = B; a.P_b0 = 0;
    a.lay = *layout;
    a.scale_log2e = float(double(inv_temperature) * 1.4426950408889634);
    attn_mask(a, mask);
    return launch_attn(a, hipStream_t(stream));
}
}  // namespace

// ================================================================== C ABI
extern "C" {

int lamp_version(void) { return LAMP_HIP_ABI_VERSION; }

const char* lamp_strerror(int status) {
    switch (status) {
        case LAMP_OK: return "ok";
        case LAMP_E_DIMS: return "lamp: non-positive or inconsistent dimensions";
        case LAMP_E_ALIGN: return "lamp: pointer or leading dimension not 16-byte aligned";
        case LAMP_E_WORKSPACE: return "lamp: workspace too small";
        case LAMP_E_UNSUPPORTED: return "lamp: configuration not supported by this build";
        case LAMP_E_NULL: return "lamp: required pointer is NULL";
        default: break;
    }
    if (status > 0) return hipGetErrorString(hipError_t(status));
    return "lamp: unknown status";
}

int lamp_linear_fwd(const float* A, int64_t M, int32_t K, int64_t lda, const float* W, int32_t N, int64_t ldw,
                    const float* bias, const float* residual, int64_t ldr, int32_t relu, float* C, int64_t ldc,
                    lamp_stream_t stream) {
    return lamp_linear_prec_fwd(A, M, K, lda, W, N, ldw, bias, residual, ldr, relu, C, ldc, LAMP_PREC_FP32, stream);
}

int lamp_linear_prec_fwd(const float* A, int64_t M, int32_t K, int64_t lda, const float* W, int32_t N, int64_t ldw,
                         const float* bias, const float* residual, int64_t ldr, int32_t relu, float* C, int64_t ldc,
                         int32_t precision, lamp_stream_t stream) {
    if (precision != LAMP_PREC_FP32 && precision != LAMP_PREC_BF16X3 && precision != LAMP_PREC_BF16X6) return LAMP_E_UNSUPPORTED;
    const float* Ws[1] = {W};
    const float* bs[1] = {bias};
    float* Cs[1] = {C};
    if (lda < K || ldw < K || ldc < N || (residual && ldr < N)) return LAMP_E_DIMS;
    return linear(A, M, K, lda, Ws, 1, N, ldw, bs, residual, ldr, relu, Cs, ldc, precision, hipStream_t(stream));
}

int lamp_linear_packed_fwd(const float* A, int64_t M, int32_t K, int64_t lda, const float* const* W, const float* const* W_pack,
                           int32_t n_seg, int32_t N, int64_t ldw, const float* const* bias, const float* residual, int64_t ldr,
                           int32_t relu, float* const* C, int64_t ldc, const int32_t* m_dev, lamp_stream_t stream) {
    if (!W || !C) return LAMP_E_NULL;
    if (n_seg < 1 || n_seg > GEMM_MAX_SEG || lda < K || ldw < K || ldc < N || (residual && ldr < N)) return LAMP_E_DIMS;
    return linear(A, M, K, lda, W, n_seg, N, ldw, bias, residual, ldr, relu, C, ldc, LAMP_PREC_FP32, hipStream_t(stream), m_dev,
                  nullptr, nullptr, W_pack);
}

int lamp_layernorm_fwd(const float* x, int64_t M, int32_t d, const float* gamma, const float* beta, float eps,
                       float* y, lamp_stream_t stream) {
    LayerNormParams p{x, M, d, gamma, beta, y, eps};
    return launch_layernorm(p, hipStream_t(stream));
}

int lamp_sdpa_fwd(const float* q, const float* k, const float* v, float* out, float* attn, int32_t B, int32_t H,
                  int32_t lq, int32_t lk, int32_t d_k, int32_t d_v, float inv_temperature, const lamp_mask* mask,
                  const lamp_attn_layout* layout, lamp_stream_t stream) {
    return sdpa_impl(q, k, v, out, attn, nullptr, B, H, lq, lk, d_k, d_v, inv_temperature, mask, layout, stream);
}

int lamp_sdpa_act_fwd(const float* q, const float* k, const float* v, float* out, float* attn, int32_t B, int32_t H,
                      int32_t lq, int32_t lk, int32_t d_k, int32_t d_v, float inv_temperature, int32_t act,
                      const lamp_mask* mask, const lamp_attn_layout* layout, lamp_stream_t stream) {
    return sdpa_impl(q, k, v, out, attn, nullptr, B, H, lq, lk, d_k, d_v, inv_temperature, mask, layout, stream, act);
}

int lamp_sdpa_fwd_fast_maps(const float* q, const float* k, const float* v, float* out, float* attn, float* lse,
                            int32_t B, int32_t H, int32_t lq, int32_t lk, int32_t d_k, int32_t d_v,
                            float inv_temperature, const lamp_mask* mask, const lamp_attn_layout* layout,
                            lamp_stream_t stream) {
    if (!attn || !lse || !out || !v) return LAMP_E_NULL;
    return sdpa_impl(q, k, v, out, attn, lse, B, H, lq, lk, d_k, d_v, inv_temperature, mask, layout, stream);
}

size_t lamp_mha_workspace_bytes(int32_t B, int32_t lq, int32_t lk, int32_t d_model, int32_t n_head, int32_t d_k,
                                int32_t d_v) {
    (void)d_model;
    if (B <= 0 || lq <= 0 || lk <= 0 || n_head <= 0 || d_k <= 0 || d_v <= 0) return 0;
    Carver c{nullptr, size_t(B)};
    MhaScratch sc;
    mha_layout(c, sc, lq, lk, n_head, d_k, d_v, true);
    return c.off;
}

int lamp_mha_fwd(const float* xq, const float* xkv, int32_t B, int32_t lq, int32_t lk, int32_t d_model,
                 int32_t d_k, int32_t d_v, const lamp_mha_weights* w, const lamp_mask* mask, float* out,
                 float* attn, void* workspace, size_t workspace_bytes, lamp_stream_t stream) {
    return lamp_mha_act_fwd(xq, xkv, B, lq, lk, d_model, d_k, d_v, w, LAMP_ATTN_SOFTMAX, mask, out, attn, workspace,
                            workspace_bytes, stream);
}

int lamp_mha_act_fwd(const float* xq, const float* xkv, int32_t B, int32_t lq, int32_t lk, int32_t d_model,
                     int32_t d_k, int32_t d_v, const lamp_mha_weights* w, int32_t act, const lamp_mask* mask, float* out,
                     float* attn, void* workspace, size_t workspace_bytes, lamp_stream_t stream) {
    if (act != LAMP_ATTN_SOFTMAX && act != LAMP_ATTN_SIGMOID) return LAMP_E_UNSUPPORTED;
    if (!xq || !xkv || !w || !out || !workspace) return LAMP_E_NULL;
    if (B <= 0 || lq <= 0 || lk <= 0 || d_model <= 0 || d_k <= 0 || d_v <= 0 || w->n_head <= 0) return LAMP_E_DIMS;
    if (d_model & 3) return LAMP_E_UNSUPPORTED;
    LAMP_CK(check_mask(mask, act));
    Carver c{static_cast<char*>(workspace), size_t(B)};
    MhaScratch sc;
    mha_layout(c, sc, lq, lk, w->n_head, d_k, d_v, true);
    if (c.off > workspace_bytes) return LAMP_E_WORKSPACE;
    MhaCall a{xq, xkv, B, lq, lk, d_model, d_k, d_v, w, mask, out, attn};
    a.act = act;
    LAMP_CK(mha_attend(a, sc, hipStream_t(stream)));
    return mha_tail(a, sc, nullptr, nullptr, nullptr, hipStream_t(stream));
}

size_t lamp_ffn_workspace_bytes(int64_t M, int32_t d_model, int32_t d_inner) {
    (void)d_model;
    if (M <= 0 || d_inner <= 0) return 0;
    return align_up(size_t(M) * d_inner * sizeof(float), 256);
}

int lamp_ffn_fwd(const float* x, int64_t M, int32_t d_model, int32_t d_inner, const lamp_ffn_weights* w,
                 float* out, void* workspace, size_t workspace_bytes, lamp_stream_t stream) {
    if (!x || !w || !out || !workspace) return LAMP_E_NULL;
    if (M <= 0 || d_model <= 0 || d_inner <= 0) return LAMP_E_DIMS;
    if ((d_model & 3) || (d_inner & 3)) return LAMP_E_UNSUPPORTED;
    if (workspace_bytes < size_t(M) * d_inner * sizeof(float)) return LAMP_E_WORKSPACE;
    return ffn_core(FfnParams{x, M, d_model, d_inner, w, out, static_cast<float*>(workspace)}, hipStream_t(stream));
}

int lamp_embed_fwd(const int64_t* src_seq, const int64_t* src_pos, int64_t n_tokens, const float* emb,
                   int32_t n_vocab, const float* pos_table, int32_t n_position, int32_t d_model, float* out,
                   lamp_stream_t stream) {
    return launch_embed(src_seq, src_pos, n_tokens, emb, n_vocab, pos_table, n_position, d_model, out,
                        hipStream_t(stream));
}

int lamp_pack_weight(const float* W, int32_t N, int32_t K, int64_t ldw, int32_t format, float* packed, lamp_stream_t stream) {
    return launch_pack_weight(W, N, K, ldw, format, packed, hipStream_t(stream));
}

int lamp_diag_logits_fwd(const float* y, const float* w_out, int32_t B, int32_t L, int32_t d_model,
                         float* logits, lamp_stream_t stream) {
    return launch_diag(y, w_out, B, L, d_model, logits, hipStream_t(stream));
}

static_assert(sizeof(lamp_gemm_desc) == 160, "lamp_gemm_desc layout is part of the ABI");
static_assert(sizeof(lamp_mask) == 56, "lamp_mask layout is part of the ABI (lamp_amd/_native.py: Mask)");
static_assert(sizeof(lamp_model) == 152, "lamp_model layout is part of the ABI (lamp_amd/_native.py: Model)");

size_t lamp_gemm_workspace_bytes(int32_t M, int32_t N, int32_t K, int32_t batch) {
    return gemm_gen_workspace_bytes(M, N, K, batch);
}

int lamp_gemm(const lamp_gemm_desc* d, void* workspace, size_t workspace_bytes, lamp_stream_t stream) {
    if (!d) return LAMP_E_NULL;
    return launch_gemm_gen(*d, workspace, workspace_bytes, hipStream_t(stream));
}

int lamp_gemm_grouped(const lamp_gemm_desc* descs, int32_t n, lamp_stream_t stream) {
    return launch_gemm_group(descs, n, hipStream_t(stream));
}

int lamp_layernorm_residual_fwd(const float* x, const float* residual, int64_t residual_rows, int64_t M, int32_t d,
                                const float* gamma, const float* beta, float eps, float dropout_p, uint32_t seed,
                                float* y, lamp_stream_t stream) {
    if (!y) return LAMP_E_NULL;
    if (!(dropout_p >= 0.f) || !(dropout_p < 1.f)) return LAMP_E_UNSUPPORTED;
    const DropoutSpec ds = make_dropout(dropout_p, seed);
    LayerNormParams p{x, M, d, gamma, beta, y, eps};
    p.residual = residual; p.r_mod = residual_rows; p.drop = dropout_p > 0.f ? &ds : nullptr;
    return launch_layernorm(p, hipStream_t(stream));
}

size_t lamp_layernorm_bwd_workspace_bytes(int64_t M, int32_t d) { return layernorm_bwd_workspace_bytes(M, d); }

int lamp_layernorm_bwd(const float* x, const float* residual, int64_t residual_rows, int64_t M, int32_t d,
                       const float* gamma, float eps, float dropout_p, uint32_t seed, const float* dy, float* dz,
                       float* dx, float* dgamma, float* dbeta, float* dbias, void* workspace, size_t workspace_bytes,
                       lamp_stream_t stream) {
    if (!(dropout_p >= 0.f) || !(dropout_p < 1.f)) return LAMP_E_UNSUPPORTED;
    const DropoutSpec ds = make_dropout(dropout_p, seed);
    return launch_layernorm_bwd(x, residual, residual_rows, M, d, gamma, eps, dropout_p > 0.f ? &ds : nullptr, dy, dz, dx,
                                dgamma, dbeta, dbias, workspace, workspace_bytes, hipStream_t(stream));
}

size_t lamp_colsum_workspace_bytes(int64_t M, int64_t N) { return colsum_workspace_bytes(M, N); }

int lamp_colsum(const float* x, int64_t M, int64_t N, int64_t ldx, float* out, void* workspace, size_t workspace_bytes,
                lamp_stream_t stream) {
    return launch_colsum(x, M, N, ldx, out, workspace, workspace_bytes, hipStream_t(stream));
}

size_t lamp_attn_bias_bwd_workspace_bytes(int64_t n_slices, int32_t lq, int32_t lk) {
    return attn_bias_bwd_workspace_bytes(n_slices, lq, lk);
}

int lamp_attn_bias_bwd(const float* dS, int64_t n_slices, int32_t lq, int32_t lk, float scale, const float* bias,
                       int64_t bias_stride_q, float* dbias, int64_t ld, void* workspace, size_t workspace_bytes,
                       lamp_stream_t stream) {
    return launch_attn_bias_bwd(dS, n_slices, lq, lk, scale, bias, bias_stride_q, dbias, ld, workspace, workspace_bytes,
                                hipStream_t(stream));
}

int lamp_label_bias_fold(const float* param, int64_t ld_p, const uint8_t* blocked_u8, int32_t L, float* out,
                         lamp_stream_t stream) {
    return launch_label_bias_fold(param, ld_p, blocked_u8, L, out, hipStream_t(stream));
}

int lamp_dropout(const float* x, int64_t n, float p, uint32_t seed, float* y, lamp_stream_t stream) {
    return launch_dropout(x, n, p, seed, y, hipStream_t(stream));
}

int lamp_softmax_bwd(const float* P, const float* dP, int64_t rows, int32_t lk, float scale, float* dS,
                     lamp_stream_t stream) {
    return launch_softmax_bwd(P, dP, rows, lk, scale, dS, hipStream_t(stream));
}

int lamp_sigmoid_attn_bwd(const float* P, const float* dP, int64_t rows, int32_t lk, float scale, float dropout_p,
                          uint32_t seed, float* dS, lamp_stream_t stream) {
    if (!(dropout_p >= 0.f) || !(dropout_p < 1.f)) return LAMP_E_UNSUPPORTED;
    const DropoutSpec ds = make_dropout(dropout_p, seed);
    return launch_sigmoid_bwd(P, dP, rows, lk, scale, dS, hipStream_t(stream), dropout_p > 0.f ? &ds : nullptr);
}

int lamp_diag_logits_bwd(const float* y, const float* w_out, const float* dlogits, int32_t B, int32_t L, int32_t d_model,
                         float* dy, float* dw, lamp_stream_t stream) {
    return launch_diag_bwd(y, w_out, dlogits, B, L, d_model, dy, dw, hipStream_t(stream));
}

int lamp_embed_bwd(const int64_t* src_seq, int64_t n_tokens, const float* dout, int32_t d_model, int32_t n_vocab,
                   int64_t pad_idx, float* d_emb, lamp_stream_t stream) {
    return launch_embed_bwd(src_seq, n_tokens, dout, d_model, n_vocab, pad_idx, d_emb, hipStream_t(stream));
}

// ---- training-mode sub-layers, one call each (lamp_amd/training.py) -------------------------------------------------------
namespace {
// C_z[m, n] (+)= sum_k A_z(m, k) B_z(n, k) through gemm_gen; strides in elements, (row, col) per operand
struct Opd {
    const float* p;
    int64_t rs, cs, b0, b1;
};
int gg(const Opd& A, const Opd& B, float* C, int64_t ldc, int64_t cb0, int64_t cb1, int M, int N, int K, int nb0, int nb1,
       bool accumulate, const float* relu_mask, void* ws, size_t ws_bytes, hipStream_t s) {
    lamp_gemm_desc d{};
    d.A = A.p; d.B = B.p; d.C = C;
    d.M = M; d.N = N; d.K = K;
    d.batch0 = nb0; d.batch1 = nb1;
    d.accumulate = accumulate ? 1 : 0;
    d.a_row_stride = A.rs; d.a_col_stride = A.cs; d.a_batch0 = A.b0; d.a_batch1 = A.b1;
    d.b_row_stride = B.rs; d.b_col_stride = B.cs; d.b_batch0 = B.b0; d.b_batch1 = B.b1;
    d.ldc = ldc; d.c_batch0 = cb0; d.c_batch1 = cb1;
    d.relu_mask = relu_mask; d.ld_mask = N;
    d.alpha = 1.f;
    const size_t need = gemm_gen_workspace_bytes(M, N, K, nb0 * nb1);
    return launch_gemm_gen(d, need <= ws_bytes ? ws : nullptr, need <= ws_bytes ? ws_bytes : 0, s);
}
inline Opd rows(const float* p, int64_t ld) { return Opd{p, ld, 1, 0, 0}; }        // [m, k], k contiguous
inline Opd cols(const float* p, int64_t ld) { return Opd{p, 1, ld, 0, 0}; }        // stored [k, m]: the transposed read
inline size_t max3(size_t a, size_t b, size_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// The single-batch products of a backward composite, as (M, N, K) of C[M, N] = A[M, K] B[N, K]^T.  The composite issues its
// products FROM this table and its *_workspace_bytes() takes the maximum OVER it: gemm_gen_workspace_bytes is not monotone in
// the shape (an output of 512 tiles or more takes no K split), so no "largest" shape bounds the others.
struct Prod {
    int M, N, K;
};
enum { FFN_DW2, FFN_DH, FFN_DW1, FFN_DX, FFN_PRODS };
struct FfnBwdProds {
    Prod p[FFN_PRODS];
    FfnBwdProds(int M, int d, int dff) : p{{d, dff, M}, {M, dff, d}, {dff, d, M}, {M, d, dff}} {}
};
enum { MHA_DFC, MHA_DA, MHA_DWQ, MHA_DWK, MHA_DWV, MHA_DXQ, MHA_DXK, MHA_DXV, MHA_PRODS };
struct MhaBwdProds {
    Prod p[MHA_PRODS];
    MhaBwdProds(int Mq, int Mk, int d, int hdk, int hdv)
        : p{{d, hdv, Mq}, {Mq, hdv, d}, {hdk, d, Mq}, {hdk, d, Mk}, {hdv, d, Mk}, {Mq, d, hdk}, {Mk, d, hdk}, {Mk, d, hdv}} {}
};
inline size_t prods_workspace_bytes(const Prod* p, int n) {
    size_t need = 0;
    for (int i = 0; i < n; ++i) need = std::max(need, gemm_gen_workspace_bytes(p[i].M, p[i].N, p[i].K, 1));
    return need;
}
int gp(const Opd& A, const Opd& B, float* C, const Prod& q, bool accumulate, const float* relu_mask, void* ws, size_t ws_bytes,
       hipStream_t s) {
    return gg(A, B, C, q.N, 0, 0, q.M, q.N, q.K, 1, 1, accumulate, relu_mask, ws, ws_bytes, s);
}
}  // namespace

int lamp_ffn_train_fwd(const float* x, int64_t M, int32_t d_model, int32_t d_inner, const lamp_ffn_weights* w,
                       float dropout_p, uint32_t seed, float* h, float* o, float* y, lamp_stream_t stream) {
    if (!x || !w || !h || !o || !y) return LAMP_E_NULL;
    if (!w->w1 || !w->b1 || !w->w2 || !w->b2 || !w->ln_g || !w->ln_b) return LAMP_E_NULL;
    if (M <= 0 || d_model <= 0 || d_inner <= 0) return LAMP_E_DIMS;
    if (!(dropout_p >= 0.f) || !(dropout_p < 1.f)) return LAMP_E_UNSUPPORTED;
    hipStream_t s = hipStream_t(stream);
    {
        const float* W[1] = {w->w1};
        const float* b[1] = {w->b1};
        float* C[1] = {h};
        LAMP_CK(linear(x, M, d_model, d_model, W, 1, d_inner, d_model, b, nullptr, 0, 1, C, d_inner, LAMP_PREC_FP32, s));
    }
    {
        const float* W[1] = {w->w2};
        const float* b[1] = {w->b2};
        float* C[1] = {o};
        LAMP_CK(linear(h, M, d_inner, d_inner, W, 1, d_model, d_inner, b, nullptr, 0, 0, C, d_model, LAMP_PREC_FP32, s));
    }
    const DropoutSpec ds = make_dropout(dropout_p, seed);
    LayerNormParams p{o, M, d_model, w->ln_g, w->ln_b, y};
    p.residual = x; p.drop = dropout_p > 0.f ? &ds : nullptr;
    return launch_layernorm(p, s);
}

size_t lamp_ffn_bwd_workspace_bytes(int64_t M, int32_t d_model, int32_t d_inner) {
    if (M <= 0 || M > 0x7fffffff || d_model <= 0 || d_inner <= 0) return 0;
    const FfnBwdProds g(int(M), d_model, d_inner);
    return max3(layernorm_bwd_workspace_bytes(M, d_model), colsum_workspace_bytes(M, d_inner),
                prods_workspace_bytes(g.p, FFN_PRODS));
}

size_t lamp_ffn_bwd_partials_bytes(int64_t M, int32_t d_model, int32_t d_inner) {
    if (M <= 0 || d_model <= 0 || d_inner <= 0) return 0;
    return align_up(layernorm_bwd_workspace_bytes(M, d_model), 256) + colsum_workspace_bytes(M, d_inner);
}

int lamp_reduce_partials_grouped(const lamp_reduce_job* jobs, int32_t n, lamp_stream_t stream) {
    return launch_reduce_group(jobs, n, hipStream_t(stream));
}

int lamp_ffn_bwd(const float* x, const float* h, const float* o, const float* dy, int64_t M, int32_t d_model,
                 int32_t d_inner, const lamp_ffn_weights* w, float dropout_p, uint32_t seed, float* dx, float* d_o, float* dh,
                 float* dW1, float* dW2, float* db1, float* db2, float* dgamma, float* dbeta, void* workspace,
                 size_t workspace_bytes, void* partials, size_t partials_bytes, lamp_reduce_job* jobs, lamp_stream_t stream) {
    if (partials && (!jobs || partials_bytes < lamp_ffn_bwd_partials_bytes(M, d_model, d_inner))) return LAMP_E_WORKSPACE;
    if (!x || !h || !o || !dy || !w || !dx || !dh || !db1 || !db2 || !dgamma || !dbeta) return LAMP_E_NULL;
    if (!w->w1 || !w->w2 || !w->ln_g) return LAMP_E_NULL;
    if (M <= 0 || M > 0x7fffffff || d_model <= 0 || d_inner <= 0) return LAMP_E_DIMS;
    if (!(dropout_p >= 0.f) || !(dropout_p < 1.f)) return LAMP_E_UNSUPPORTED;
    const bool drop = dropout_p > 0.f;
    if (drop && !d_o) return LAMP_E_NULL;
    if (!drop && !dW2) return LAMP_E_UNSUPPORTED;   // without dropout d_o IS dx, which is accumulated into: dW2 cannot wait
    if (workspace_bytes < lamp_ffn_bwd_workspace_bytes(M, d_model, d_inner) || (!workspace && workspace_bytes))
        return LAMP_E_WORKSPACE;
    hipStream_t s = hipStream_t(stream);
    const DropoutSpec ds = make_dropout(dropout_p, seed);
    const int Mi = int(M);
    const size_t ln_bytes = align_up(layernorm_bwd_workspace_bytes(M, d_model), 256);
    char* keep = static_cast<char*>(partials);
    if (keep)
        LAMP_CK(launch_layernorm_bwd(o, x, 0, M, d_model, w->ln_g, 1e-5f, drop ? &ds : nullptr, dy, dx, drop ? d_o : nullptr,
                                     dgamma, dbeta, db2, keep, ln_bytes, s, &jobs[0]));
    else
        LAMP_CK(launch_layernorm_bwd(o, x, 0, M, d_model, w->ln_g, 1e-5f, drop ? &ds : nullptr, dy, dx, drop ? d_o : nullptr,
                                     dgamma, dbeta, db2, workspace, workspace_bytes, s));
    const float* g_o = drop ? d_o : dx;
    const FfnBwdProds g(Mi, d_model, d_inner);   // the products lamp_ffn_bwd_workspace_bytes sized the workspace for
    if (dW2)   // dW2 = d_o^T h
        LAMP_CK(gp(cols(g_o, d_model), cols(h, d_inner), dW2, g.p[FFN_DW2], false, nullptr, workspace, workspace_bytes, s));
    // dh = relu'(h) * (d_o W2)
    LAMP_CK(gp(rows(g_o, d_model), cols(w->w2, d_inner), dh, g.p[FFN_DH], false, h, workspace, workspace_bytes, s));
    if (keep)
        LAMP_CK(launch_colsum(dh, M, d_inner, d_inner, db1, keep + ln_bytes, partials_bytes - ln_bytes, s, &jobs[1]));
    else
        LAMP_CK(launch_colsum(dh, M, d_inner, d_inner, db1, workspace, workspace_bytes, s));
    if (dW1)   // dW1 = dh^T x
        LAMP_CK(gp(cols(dh, d_inner), cols(x, d_model), dW1, g.p[FFN_DW1], false, nullptr, workspace, workspace_bytes, s));
    // dx = residual branch + dh W1
    return gp(rows(dh, d_inner), cols(w->w1, d_model), dx, g.p[FFN_DX], true, nullptr, workspace, workspace_bytes, s);
}

int lamp_mha_train_fwd(const lamp_mha_train_desc* c, const lamp_mha_weights* w, const float* xq, const float* xk,
                       const float* xv, const lamp_mask* mask, float* q, float* k, float* v, float* a, float* P, float* Pd,
                       float* lse, float* o, float* y, lamp_stream_t stream) {
    return lamp_mha_train_act_fwd(c, w, LAMP_ATTN_SOFTMAX, xq, xk, xv, mask, q, k, v, a, P, Pd, lse, o, y, stream);
}

int lamp_mha_train_act_fwd(const lamp_mha_train_desc* c, const lamp_mha_weights* w, int32_t act, const float* xq,
                           const float* xk, const float* xv, const lamp_mask* mask, float* q, float* k, float* v, float* a,
                           float* P, float* Pd, float* lse, float* o, float* y, lamp_stream_t stream) {
    if (act != LAMP_ATTN_SOFTMAX && act != LAMP_ATTN_SIGMOID) return LAMP_E_UNSUPPORTED;
    if (!c || !w || !xq || !xk || !xv || !q || !k || !v || !a || !P || (!lse && act == LAMP_ATTN_SOFTMAX) || !y) return LAMP_E_NULL;
    if (!w->w_qs || !w->w_ks || !w->w_vs || !w->ln_g || !w->ln_b) return LAMP_E_NULL;
    const int B = c->B, lq = c->lq, lk = c->lk, d = c->d_model, H = c->n_head, dk = c->d_k, dv = c->d_v;
    if (B <= 0 || lq <= 0 || lk <= 0 || d <= 0 || H <= 0 || dk <= 0 || dv <= 0) return LAMP_E_DIMS;
    if (H != w->n_head) return LAMP_E_DIMS;
    if (dk > 128 || dv > 128) return LAMP_E_UNSUPPORTED;   // wide heads keep their scores in the map buffer: per-launch route
    if (!(c->p_attn >= 0.f) || !(c->p_attn < 1.f) || !(c->p_out >= 0.f) || !(c->p_out < 1.f)) return LAMP_E_UNSUPPORTED;
    const bool has_fc = w->fc != nullptr;
    if (has_fc ? !o : (H * dv != d)) return has_fc ? LAMP_E_NULL : LAMP_E_DIMS;
    if (c->p_attn > 0.f && !Pd) return LAMP_E_NULL;
    LAMP_CK(check_mask(mask, act));   // before the projections go out
    hipStream_t s = hipStream_t(stream);
    const int hdk = H * dk, hdv = H * dv;
    const int64_t Mq = int64_t(B) * lq, Mk = int64_t(B) * lk;
    LAMP_CK(project_qkv(*w, d, dk, dv, xq, Mq, q, xk, xv, Mk, k, v, LAMP_PREC_FP32, s, nullptr, nullptr));
    const lamp_attn_layout lay{int64_t(lq) * hdk, dk, hdk, int64_t(lk) * hdk, dk, hdk, int64_t(lk) * hdv, dv, hdv,
                               int64_t(lq) * hdv, dv, hdv};
    LAMP_CK(sdpa_impl(q, k, v, a, P, lse, B, H, lq, lk, dk, dv, c->inv_temperature, mask, &lay, stream, act));
    if (c->p_attn > 0.f) {   // the reference drops probabilities AFTER the softmax (lamp/SubLayers.py:40-41): a = dropout(P) V
        LAMP_CK(launch_dropout(P, int64_t(H) * B * lq * lk, c->p_attn, c->seed_attn, Pd, s));
        LAMP_CK(gg(Opd{Pd, lk, 1, int64_t(B) * lq * lk, int64_t(lq) * lk}, Opd{v, 1, hdv, dv, int64_t(lk) * hdv}, a, hdv, dv,
                   int64_t(lq) * hdv, lq, dv, lk, H, B, false, nullptr, nullptr, 0, s));
    }
    const DropoutSpec ds = make_dropout(c->p_out, c->seed_out);
    const float* pre = a;
    if (has_fc) {
        const float* W[1] = {w->fc};
        float* C[1] = {o};
        LAMP_CK(linear(a, Mq, hdv, hdv, W, 1, d, hdv, nullptr, nullptr, 0, 0, C, d, LAMP_PREC_FP32, s));
        pre = o;
    }
    LayerNormParams ln{pre, Mq, d, w->ln_g, w->ln_b, y};
    ln.residual = xq; ln.drop = c->p_out > 0.f ? &ds : nullptr;
    return launch_layernorm(ln, s);
}

size_t lamp_mha_bwd_workspace_bytes(const lamp_mha_train_desc* c) {
    if (!c || c->B <= 0 || c->lq <= 0 || c->lk <= 0 || c->d_model <= 0 || c->n_head <= 0 || c->d_k <= 0 || c->d_v <= 0) return 0;
    const int64_t Mq = int64_t(c->B) * c->lq, Mk = int64_t(c->B) * c->lk;
    if (Mq > 0x7fffffff || Mk > 0x7fffffff) return 0;
    const MhaBwdProds g(int(Mq), int(Mk), c->d_model, c->n_head * c->d_k, c->n_head * c->d_v);
    const size_t ln = layernorm_bwd_workspace_bytes(Mq, c->d_model), gemm = prods_workspace_bytes(g.p, MHA_PRODS);
    return ln > gemm ? ln : gemm;
}

size_t lamp_mha_bwd_partials_bytes(const lamp_mha_train_desc* c) {
    if (!c || c->B <= 0 || c->lq <= 0 || c->d_model <= 0) return 0;
    return layernorm_bwd_workspace_bytes(int64_t(c->B) * c->lq, c->d_model);
}

int lamp_mha_bwd(const lamp_mha_train_desc* c, const lamp_mha_weights* w, const float* xq, const float* xk, const float* xv,
                 const float* q, const float* k, const float* v, const float* a, const float* P, const float* Pd,
                 const float* o, const float* dy, float* dxq, float* d_o, float* da, float* dP, float* dq, float* dk_,
                 float* dv_, float* dxk, float* dxv, float* dgamma, float* dbeta, float* dwq, float* dwk, float* dwv, float* dfc,
                 void* workspace, size_t workspace_bytes, void* partials, size_t partials_bytes, lamp_reduce_job* job,
                 lamp_stream_t stream) {
    return lamp_mha_act_bwd(c, w, LAMP_ATTN_SOFTMAX, xq, xk, xv, q, k, v, a, P, Pd, o, dy, dxq, d_o, da, dP, dq, dk_, dv_, dxk,
                            dxv, dgamma, dbeta, dwq, dwk, dwv, dfc, workspace, workspace_bytes, partials, partials_bytes, job,
                            stream);
}

int lamp_mha_act_bwd(const lamp_mha_train_desc* c, const lamp_mha_weights* w, int32_t act, const float* xq, const float* xk,
                     const float* xv, const float* q, const float* k, const float* v, const float* a, const float* P,
                     const float* Pd, const float* o, const float* dy, float* dxq, float* d_o, float* da, float* dP, float* dq,
                     float* dk_, float* dv_, float* dxk, float* dxv, float* dgamma, float* dbeta, float* dwq, float* dwk,
                     float* dwv, float* dfc, void* workspace, size_t workspace_bytes, void* partials, size_t partials_bytes,
                     lamp_reduce_job* job, lamp_stream_t stream) {
    if (act != LAMP_ATTN_SOFTMAX && act != LAMP_ATTN_SIGMOID) return LAMP_E_UNSUPPORTED;
    if (partials && (!job || partials_bytes < lamp_mha_bwd_partials_bytes(c))) return LAMP_E_WORKSPACE;
    if (!c || !w || !xq || !xk || !xv || !q || !k || !v || !a || !P || !dy) return LAMP_E_NULL;
    if (!dxq || !dP || !dq || !dk_ || !dv_ || !dxk || !dgamma || !dbeta) return LAMP_E_NULL;
    if (!w->w_qs || !w->w_ks || !w->w_vs || !w->ln_g) return LAMP_E_NULL;
    const int B = c->B, lq = c->lq, lk = c->lk, d = c->d_model, H = c->n_head, dk = c->d_k, dv = c->d_v;
    if (B <= 0 || lq <= 0 || lk <= 0 || d <= 0 || H <= 0 || dk <= 0 || dv <= 0 || H != w->n_head) return LAMP_E_DIMS;
    const int64_t Mq64 = int64_t(B) * lq, Mk64 = int64_t(B) * lk;
    if (Mq64 > 0x7fffffff || Mk64 > 0x7fffffff || int64_t(H) * B > 65535) return LAMP_E_DIMS;
    if (!(c->p_attn >= 0.f) || !(c->p_attn < 1.f) || !(c->p_out >= 0.f) || !(c->p_out < 1.f)) return LAMP_E_UNSUPPORTED;
    const bool has_fc = w->fc != nullptr, drop_o = c->p_out > 0.f, drop_a = c->p_attn > 0.f;
    if (has_fc && (!o || !da)) return LAMP_E_NULL;
    if (drop_o && !d_o) return LAMP_E_NULL;
    if (drop_a && !Pd) return LAMP_E_NULL;
    if (has_fc && !drop_o && !dfc) return LAMP_E_UNSUPPORTED;   // d_o IS dxq then, which is accumulated into: dfc cannot wait
    if (workspace_bytes < lamp_mha_bwd_workspace_bytes(c) || (!workspace && workspace_bytes)) return LAMP_E_WORKSPACE;
    hipStream_t s = hipStream_t(stream);
    const int hdk = H * dk, hdv = H * dv, Mq = int(Mq64), Mk = int(Mk64);
    const DropoutSpec ds = make_dropout(c->p_out, c->seed_out);
    void* ws = workspace;
    const size_t wsb = workspace_bytes;
    const MhaBwdProds g(Mq, Mk, d, hdk, hdv);   // the single-batch products lamp_mha_bwd_workspace_bytes sized the workspace for
    // add & norm (+ output dropout): dxq <- the residual branch, d_o <- the gradient of the fc output
    if (partials)
        LAMP_CK(launch_layernorm_bwd(has_fc ? o : a, xq, 0, Mq64, d, w->ln_g, 1e-5f, drop_o ? &ds : nullptr, dy, dxq,
                                     drop_o ? d_o : nullptr, dgamma, dbeta, nullptr, partials, partials_bytes, s, job));
    else
        LAMP_CK(launch_layernorm_bwd(has_fc ? o : a, xq, 0, Mq64, d, w->ln_g, 1e-5f, drop_o ? &ds : nullptr, dy, dxq,
                                     drop_o ? d_o : nullptr, dgamma, dbeta, nullptr, ws, wsb, s));
    const float* g_o = drop_o ? d_o : dxq;
    const float* g_a = g_o;   // gradient of the concatenated head outputs [Mq, H*dv]
    if (has_fc) {
        if (dfc) LAMP_CK(gp(cols(g_o, d), cols(a, hdv), dfc, g.p[MHA_DFC], false, nullptr, ws, wsb, s));
        LAMP_CK(gp(rows(g_o, d), cols(w->fc, hdv), da, g.p[MHA_DA], false, nullptr, ws, wsb, s));
        g_a = da;
    }   // (single head without output dropout: g_a IS dxq; every product that reads it is issued before (*) accumulates into it)
    // head views: index (h, b) -> batch0 = head, batch1 = sample
    const int64_t PB0 = int64_t(B) * lq * lk, PB1 = int64_t(lq) * lk;
    const float* Pu = drop_a ? Pd : P;
    const DropoutSpec da_spec = make_dropout(c->p_attn, c->seed_attn);
    // dV = Pd^T dA
    LAMP_CK(gg(Opd{Pu, 1, lk, PB0, PB1}, Opd{g_a, 1, hdv, dv, int64_t(lq) * hdv}, dv_, hdv, dv, int64_t(lk) * hdv, lk, dv, lq,
               H, B, false, nullptr, nullptr, 0, s));
    // dPd = dA V^T
    LAMP_CK(gg(Opd{g_a, hdv, 1, dv, int64_t(lq) * hdv}, Opd{v, hdv, 1, dv, int64_t(lk) * hdv}, dP, lk, PB0, PB1, lq, lk, dv, H,
               B, false, nullptr, nullptr, 0, s));
    // dS = softmax backward of dropout-backward(dPd), in place (the mask is applied on load)
    if (act == LAMP_ATTN_SIGMOID)
        LAMP_CK(launch_sigmoid_bwd(P, dP, int64_t(H) * B * lq, lk, c->inv_temperature, dP, s, drop_a ? &da_spec : nullptr));
    else
        LAMP_CK(launch_softmax_bwd(P, dP, int64_t(H) * B * lq, lk, c->inv_temperature, dP, s, drop_a ? &da_spec : nullptr));
    // dQ = dS K, dK = dS^T Q
    LAMP_CK(gg(Opd{dP, lk, 1, PB0, PB1}, Opd{k, 1, hdk, dk, int64_t(lk) * hdk}, dq, hdk, dk, int64_t(lq) * hdk, lq, dk, lk, H, B,
               false, nullptr, nullptr, 0, s));
    LAMP_CK(gg(Opd{dP, 1, lk, PB0, PB1}, Opd{q, 1, hdk, dk, int64_t(lq) * hdk}, dk_, hdk, dk, int64_t(lk) * hdk, lk, dk, lq, H, B,
               false, nullptr, nullptr, 0, s));
    if (dwq) LAMP_CK(gp(cols(dq, hdk), cols(xq, d), dwq, g.p[MHA_DWQ], false, nullptr, ws, wsb, s));
    if (dwk) LAMP_CK(gp(cols(dk_, hdk), cols(xk, d), dwk, g.p[MHA_DWK], false, nullptr, ws, wsb, s));
    if (dwv) LAMP_CK(gp(cols(dv_, hdv), cols(xv, d), dwv, g.p[MHA_DWV], false, nullptr, ws, wsb, s));
    // (*) data gradients of the three projections
    LAMP_CK(gp(rows(dq, hdk), cols(w->w_qs, d), dxq, g.p[MHA_DXQ], true, nullptr, ws, wsb, s));
    // dxk == dxq (self-attention: query and key source are one tensor): its gradient is the sum, accumulated in place
    LAMP_CK(gp(rows(dk_, hdk), cols(w->w_ks, d), dxk, g.p[MHA_DXK], dxk == dxq, nullptr, ws, wsb, s));
    if (dxv) return gp(rows(dv_, hdv), cols(w->w_vs, d), dxv, g.p[MHA_DXV], false, nullptr, ws, wsb, s);
    return gp(rows(dv_, hdv), cols(w->w_vs, d), dxk, g.p[MHA_DXV], true, nullptr, ws, wsb, s);
}

int lamp_prior_graph_build(const int64_t* label_ids, const int64_t* offsets, int64_t n_samples, int32_t L, float* adj,
                           uint8_t* blocked, lamp_stream_t stream) {
    return launch_prior_graph(label_ids, offsets, n_samples, L, adj, blocked, hipStream_t(stream));
}

int lamp_sigmoid_bce_fwd(const float* logits, const float* targets, int64_t n_rows, int32_t L, float* probs,
                         float* row_loss, lamp_stream_t stream) {
    return launch_sigmoid_bce(logits, targets, n_rows, L, probs, row_loss, hipStream_t(stream));
}

// ------------------------------------------------------------------ whole forward
// Shapes of one whole forward: what its workspace layout and its stages read.
struct FwdDims {
    int T, L, R, Rq;         // encoder rows per sample, labels, max(T, L), Q / A rows (R with the encoder's maps, else L)
    int d, dff, h, dk, dv;   // h: the most heads of any attention block
    int n_ahead;             // decoder layers whose enc-attention K / V are projected right after the encoder, or 0
    int fe_rows;             // one-hot front end: padded conv2 input rows per sample, else 0
    bool w2_repack;          // one-hot front end without a caller-packed conv2 weight
    bool live;               // the encoder's self-attention output is used (lamp_fwd_options::enc_self_attn)
};

// The model checks the workspace sizes share with the forward.  T_in: tokens per sample; the one-hot front end `fe`
// halves them.  The K/V-ahead buffers are counted for every decoder layer of a token model: the forward drops them
// (n_ahead = 0) when it does not project ahead.
static int fwd_dims(const lamp_model* m, const lamp_onehot_frontend* fe, int T_in, bool want_attn, FwdDims* g,
                    bool live = false) {
    if (!m) return LAMP_E_NULL;
    const int T = fe ? T_in / 2 : T_in;
    if (m->d_model <= 0 || m->d_inner <= 0 || m->d_k <= 0 || m->d_v <= 0 || m->n_labels <= 0 || T <= 0 ||
        m->n_layers_enc < 0 || m->n_layers_dec < 0)
        return LAMP_E_DIMS;
    if ((m->n_layers_enc && !m->enc_layers) || (m->n_layers_dec && !m->dec_layers)) return LAMP_E_NULL;
    int h = 1;
    for (int i = 0; i < m->n_layers_enc; ++i) h = std::max(h, m->enc_layers[i].slf_attn.n_head);
    for (int i = 0; i < m->n_layers_dec; ++i) {
        const lamp_dec_layer& l = m->dec_layers[i];
        h = std::max(h, l.enc_attn.n_head);
        if (l.slf_attn.present) h = std::max(h, l.slf_attn.n_head);
    }
    const int L = m->n_labels, R = std::max(T + (live ? 1 : 0), L);   // live, packed: + one PAD row per sample
    *g = FwdDims{T, L, R, want_attn || live ? R : L, m->d_model, m->d_inner, h, m->d_k, m->d_v, fe ? 0 : m->n_layers_dec,
                 fe ? T + 16 : 0, fe && !fe->conv2_pack, live};
    return 0;
}

// The carved workspace of the forward.
struct FwdScratch {
    float* H;           // FFN hidden rows (+ one for the shared PAD row of the packed layout)
    MhaScratch mha;     // Q, K, V, A (+ S of wide heads), lse of the largest attention
    float* Y;           // decoder rows
    float* Xp;          // packed encoder rows [n_tok + 1, d]: + the shared PAD row
    int* plan_ints;     // the micro-batch's SeqPlan
    unsigned long long* granules;   // the plan's hand-off words inside the merged plan + gather launch: 2 mb + 2
    int *row_tok, *row_pos;         // [mb T + 1] each: token / position of every packed row, for the gathered residual
    float *K_ahead[GEMM_MAX_SEG / 2], *V_ahead[GEMM_MAX_SEG / 2];   // K/V ahead
    int* live_rows;     // live encoder on the packed rows: n_tok + mb, counted on the device (attention_ragged.hip)
    float* fe_x;        // the one-hot front end's zero-padded channel-last conv2 input
    float* w2;          // conv2's packed weight
};

// THE forward workspace: every region, in carve order.
static void fwd_layout(const FwdDims& g, Carver& c, FwdScratch& w) {
    const size_t T = g.T, d = g.d;
    c.take(&w.H, size_t(g.R) * g.dff, g.dff);
    mha_layout(c, w.mha, g.Rq, g.R, g.h, g.dk, g.dv, false);
    c.take(&w.Y, size_t(g.L) * d);
    c.take(&w.Xp, (T + (g.live ? 1 : 0)) * d, d);
    if (g.live) c.take(&w.live_rows, 0, 4);
    take_plan(c, &w.plan_ints, g.T);
    c.take(&w.granules, 4, 4);
    c.take(&w.row_tok, 2 * T, 2);
    for (int i = 0; i < g.n_ahead; ++i) {   // the byte bound may count more layers than the forward projects ahead
        const bool kept = i < GEMM_MAX_SEG / 2;
        c.take(kept ? &w.K_ahead[i] : nullptr, T * g.h * g.dk);
        c.take(kept ? &w.V_ahead[i] : nullptr, T * g.h * g.dv);
    }
    if (g.fe_rows) c.take(&w.fe_x, size_t(g.fe_rows) * d, 16 * d);
    if (g.w2_repack) c.take(&w.w2, 0, 16 * d * d);
    w.row_pos = w.row_tok ? w.row_tok + (c.mb * T + 1) : nullptr;
}

static Carver fwd_size(const FwdDims& g) {
    Carver c{nullptr, 1};
    FwdScratch unused;
    fwd_layout(g, c, unused);
    return c;
}

// One micro-batch of the forward: what its stages share.
struct Pass {
    const lamp_model* m;
    const lamp_onehot_frontend* fe;
    const FwdDims& g;
    const FwdScratch& w;
    const lamp_aux* aux;
    float* logits;          // of the whole batch
    hipStream_t s;
    int B, nb;              // samples of the batch, of this micro-batch
    int64_t b0;             // this micro-batch's first sample
    const int64_t *seq, *pos;   // [nb, ld_seq] tokens and (nullable) positions
    int64_t ld_seq;
    float* x;               // [nb, T, d] padded encoder output rows
    bool packed;
    SeqPlan sp;
    lamp_mask pad_mask;
    lamp_mask label_mask;
    const float* xk = nullptr;   // what the decoder's K / V projections read: x or the packed rows
    int n_int = 0;               // intermediate predictions written so far
    const lamp_mask* enc_mask = nullptr;             // the encoder self-attention's mask: &pad_mask, or this micro-batch's
                                                     // slice of lamp_fwd_options::enc_mask
    const lamp_chain_pack* enc_packs = nullptr;      // lamp_fwd_options::enc_chain_packs
    int dec_act = LAMP_ATTN_SOFTMAX;                 // LAMP_FWD_DEC_SIGMOID: both attention blocks of every decoder layer
    int prec = LAMP_PREC_FP32;                       // LAMP_FWD_MATMUL_*: every linear() of the pass (FfnParams / MhaCall::prec)
    const lamp_gemm_packs* gp = nullptr;             // lamp_forward_packs: weight packs of the tile GEMM launches
    const lamp_kv_gemm_pack* kvp = nullptr;          // lamp_forward_packs_kv: ... and of the K / V projection of the encoder rows
    void ffn_packs(FfnParams& f, int layer) const {  // encoder layer's pos_ffn
        if (gp && gp->enc) { f.w1_pack = gp->enc[layer].w1; f.w2_pack = gp->enc[layer].w2; }
    }
};

// GraphEncoder.forward (lamp/Encoders.py:64-110) on the packed non-PAD token rows (+ ONE shared PAD row: all PAD positions
// of lamp/Encoders.py:64-79 hold the same row-wise result); the last LayerNorm scatters into the padded encoder output.
// Row-wise kernels and an M-independent k-order make this bit-identical to computing every padded position.
static int encode_packed(Pass& p) {
    const lamp_model* m = p.m;
    const FwdScratch& w = p.w;
    const int d = p.g.d, dff = p.g.dff, T = p.g.T;
    // The plan rides in the first workgroups of the embedding gather's launch and hands its results to the gather through
    // 8-byte granules (pointwise.hip: embed_plan_kernel; round 3 had it as a launch of its own -- a dependent launch costs
    // 5-8 us on this chain however little it does -- after folding it into EVERY workgroup of the gather had measured
    // slower, 21.9 us against 6.6 + 10.5).
    // Encoder layer 0's W1 folded into the embedding tables (lamp_model::enc0_emb_w1): the gather writes that layer's
    // hidden rows into H beside the embedded rows, and its first GEMM is not launched.
    // ... and the embedded rows themselves are not written either: their one reader, the residual of that layer's second
    // GEMM, gathers them from the tables through the row maps the gather kernel leaves instead (8 bytes per row).
    const bool folded = m->enc0_emb_w1 != nullptr;
    const bool gather_res =
        folded && gemm_gathered_residual_ok(d, dff, d, m->enc_layers[0].pos_ffn.b2, w.Xp, m->src_word_emb, m->position_enc);
    const EmbedFold fold{m->enc0_emb_w1, m->enc0_pos_w1, dff, folded ? w.H : nullptr, gather_res ? w.row_tok : nullptr,
                         gather_res ? w.row_pos : nullptr};
    const ResGather rg{w.row_tok, w.row_pos, m->src_word_emb, m->position_enc};
    LAMP_CK(launch_embed_plan(p.seq, p.pos, m->position_enc != nullptr, p.nb, T, m->src_word_emb, m->n_src_vocab,
                              m->position_enc, m->n_position, d, p.sp, w.granules, w.Xp, p.s, &fold));
    for (int i = 0; i < m->n_layers_enc; ++i) {   // lamp/Layers.py:18
        FfnParams f{w.Xp, int64_t(p.nb) * T + 1, d, dff, &m->enc_layers[i].pos_ffn, w.Xp, w.H};
        f.prec = p.prec;
        f.rows_dev = p.sp.rows + 1; f.hidden_ready = folded && i == 0; f.rg = gather_res && i == 0 ? &rg : nullptr;
        if (i + 1 == m->n_layers_enc) { f.scatter = &p.sp; f.nb = p.nb; f.T = T; f.y_flat = p.x; }
        p.ffn_packs(f, i);
        LAMP_CK(ffn_core(f, p.s));
    }
    p.xk = w.Xp;
    return 0;
}

// The LIVE encoder (lamp_fwd_options) on the packed rows: lamp/Layers.py:16 with its output kept, no PAD position computed.
// All PAD positions of one sample hold the same rows at every layer, so each sample has ONE PAD row (row n_tok + b) that is a
// query like its live rows; keys are the live rows.  Q / K / V come from one 3-segment GEMM over the device-counted rows, the
// attention is attention_ragged.hip, the row-local tail the separate launches (the chain launch takes a host row count), and
// a last launch scatters into the padded encoder output.
static int encode_packed_live(Pass& p) {
    const lamp_model* m = p.m;
    const FwdScratch& w = p.w;
    const int d = p.g.d, dff = p.g.dff, T = p.g.T, dk = p.g.dk, dv = p.g.dv;
    const int64_t Mub = int64_t(p.nb) * (T + 1);   // what the launches are sized for; the live count is *w.live_rows
    const EmbedFold fold{nullptr, nullptr, dff, nullptr, nullptr, nullptr};
    LAMP_CK(launch_embed_plan(p.seq, p.pos, m->position_enc != nullptr, p.nb, T, m->src_word_emb, m->n_src_vocab,
                              m->position_enc, m->n_position, d, p.sp, w.granules, w.Xp, p.s, &fold));
    LAMP_CK(launch_pad_rows(m->src_word_emb, m->position_enc, d, p.nb, p.sp, w.Xp, w.live_rows, p.s));
    for (int i = 0; i < m->n_layers_enc; ++i) {
        const lamp_mha_weights& a = m->enc_layers[i].slf_attn;
        const int hdk = a.n_head * dk, hdv = a.n_head * dv;
        const float* W[3] = {a.w_qs, a.w_ks, a.w_vs};
        float* C[3] = {w.mha.Q, w.mha.K, w.mha.V};
        LAMP_CK(linear(w.Xp, Mub, d, d, W, 3, hdk, d, nullptr, nullptr, 0, 0, C, hdk, p.prec, p.s, w.live_rows));
        LAMP_CK(launch_attn_ragged_self(w.mha.Q, w.mha.K, w.mha.V, w.mha.A, p.nb, a.n_head, T, dk, dv, p.sp, p.s));
        const float* Wfc[1] = {a.fc};
        float* Cx[1] = {w.Xp};
        LAMP_CK(linear(w.mha.A, Mub, hdv, hdv, Wfc, 1, d, hdv, nullptr, w.Xp, d, 0, Cx, d, p.prec, p.s, w.live_rows));
        LayerNormParams ln{w.Xp, Mub, d, a.ln_g, a.ln_b, w.Xp};
        ln.m_dev = w.live_rows;
        LAMP_CK(launch_layernorm(ln, p.s));
        FfnParams f{w.Xp, Mub, d, dff, &m->enc_layers[i].pos_ffn, w.Xp, w.H};
        f.rows_dev = w.live_rows; f.prec = p.prec;
        p.ffn_packs(f, i);
        LAMP_CK(ffn_core(f, p.s));
    }
    LAMP_CK(launch_scatter_rows(w.Xp, d, p.nb, T, p.sp, p.x, p.s));
    p.xk = w.Xp;
    return 0;
}

// lamp/Encoders.py:68-73, the one-hot front end in place of the embedding gather: tap gather + ReLU + pair max, then conv2
// as an implicit GEMM whose epilogue adds b2, applies the ReLU and adds the position row, straight into the encoder rows.
static int encode_onehot_front(const Pass& p) {
    const lamp_onehot_frontend* fe = p.fe;
    const int d = p.g.d, T = p.g.T;
    LAMP_CK(launch_front_fwd(p.seq, p.nb, int(p.ld_seq), fe->t1, fe->n_vocab, fe->conv1_b, d, 0.f, 0u, 0, p.w.fe_x, p.s));
    ConvWindowParams cp{p.w.fe_x, p.w.w2, fe->conv2_b, p.x, nullptr, p.m->position_enc, p.pos, int64_t(p.nb) * T, d, p.ld_seq,
                        d, 16 * d, d, T, T + 16, 1, p.m->n_position};
    return launch_conv_window(cp, p.s);
}

// The encoder on the padded [nb, T, d] rows: when the dead encoder self-attention's maps are wanted (layer 0's map reads the
// embedded rows, so they are written), with wide heads, behind the one-hot front end, or with the LIVE self-attention
// (g.live: its output feeds pos_ffn instead of being dropped -- every padded position is a query, a PAD query's zero row
// attends uniformly over its sample's live keys; each sample's keys stop at its last real one).  The enc-dec attention
// still stops at each sample's last real key.
static int encode_padded(Pass& p) {
    const lamp_model* m = p.m;
    const FwdScratch& w = p.w;
    const int d = p.g.d, dff = p.g.dff, T = p.g.T;
    const int64_t Me = int64_t(p.nb) * T;
    LAMP_CK(launch_seq_plan(p.seq, m->position_enc ? p.pos : nullptr, p.nb, T, p.ld_seq, false, p.sp, p.s));
    const bool folded = m->enc0_emb_w1 && m->n_layers_enc > 0;
    if (p.fe) {
        LAMP_CK(encode_onehot_front(p));
    } else {
        const EmbedFold fold{m->enc0_emb_w1, m->enc0_pos_w1, dff, folded ? w.H : nullptr, nullptr, nullptr};
        LAMP_CK(launch_embed(p.seq, p.pos, Me, m->src_word_emb, m->n_src_vocab, m->position_enc, m->n_position, d, p.x, p.s,
                             &fold));
    }
    for (int i = 0; i < m->n_layers_enc; ++i) {
        const lamp_enc_layer& l = m->enc_layers[i];
        float* map = p.aux && p.aux->enc_self_attn ? p.aux->enc_self_attn[i] : nullptr;
        FfnParams f{p.x, Me, d, dff, &l.pos_ffn, p.x, w.H};   // lamp/Layers.py:18
        f.prec = p.prec;
        p.ffn_packs(f, i);
        if (p.g.live) {
            // lamp/Layers.py:16 with its output kept: x <- slf_attn(x, x, x), then pos_ffn(x).  The row-local tail
            // (fc + residual -> LayerNorm -> W1 -> W2 + residual -> LayerNorm) is the decoder's sub-chain.
            MhaCall a{p.x, p.x, p.nb, T, T, d, p.g.dk, p.g.dv, &l.slf_attn, p.enc_mask, p.x, map, p.B, int(p.b0)};
            a.keys = &p.sp; a.prec = p.prec;
            bool ffn_ran = false;
            LAMP_CK(mha_attend(a, w.mha, p.s));
            LAMP_CK(mha_tail(a, w.mha, &f, p.enc_packs ? p.enc_packs + i : nullptr, &ffn_ran, p.s));
            if (!ffn_ran) LAMP_CK(ffn_core(f, p.s));
            continue;
        }
        if (map) {
            // lamp/Layers.py:16 -- only the attention map of this block is ever observable.  Maps are
            // (h*B, T, T) over the WHOLE batch: this micro-batch fills rows h*B + b0 + b.
            MhaCall a{p.x, p.x, p.nb, T, T, d, p.g.dk, p.g.dv, &l.slf_attn, p.enc_mask, nullptr, map, p.B, int(p.b0)};
            a.keys = &p.sp; a.prec = p.prec;
            LAMP_CK(mha_attend(a, w.mha, p.s));
        }
        f.hidden_ready = folded && i == 0;
        LAMP_CK(ffn_core(f, p.s));
    }
    p.xk = p.x;
    return 0;
}

// K and V projections of the first n decoder layers' enc-attention from the same encoder output: ONE launch when the
// 2n weight matrices fit the GEMM's segment list (n <= 2) -- 4 x more tiles per launch than layer by layer.
static int project_kv_layers(const float* x, int64_t Me, int d, int dk, int dv, const lamp_dec_layer* layers, int n,
                             float* const* K, float* const* V, int prec, hipStream_t s, const int* m_dev, const float* A_dense,
                             const lamp_kv_gemm_pack* packs = nullptr) {
    const int h = layers[0].enc_attn.n_head;
    bool uniform = 2 * n <= GEMM_MAX_SEG && h * dk == h * dv;
    for (int i = 1; i < n && uniform; ++i) uniform = layers[i].enc_attn.n_head == h;
    if (uniform) {
        const float* W[GEMM_MAX_SEG];
        float* C[GEMM_MAX_SEG];
        const float* Wp[GEMM_MAX_SEG];   // lamp_kv_gemm_pack: packs of {w_ks, w_vs} per layer (a missing one leaves the launch on the row-major weights)
        for (int i = 0; i < n; ++i) {
            if (!layers[i].enc_attn.w_ks || !layers[i].enc_attn.w_vs) return LAMP_E_NULL;
            W[2 * i] = layers[i].enc_attn.w_ks;
            W[2 * i + 1] = layers[i].enc_attn.w_vs;
            C[2 * i] = K[i];
            C[2 * i + 1] = V[i];
            Wp[2 * i] = packs ? packs[i].enc_k : nullptr;
            Wp[2 * i + 1] = packs ? packs[i].enc_v : nullptr;
        }
        return linear(x, Me, d, d, W, 2 * n, h * dk, d, nullptr, nullptr, 0, 0, C, h * dk, prec, s, m_dev, A_dense, nullptr, Wp);
    }
    for (int i = 0; i < n; ++i) {
        const float* Wp[3] = {nullptr, packs ? packs[i].enc_k : nullptr, packs ? packs[i].enc_v : nullptr};
        LAMP_CK(project_qkv(layers[i].enc_attn, d, dk, dv, nullptr, 0, nullptr, x, x, Me, K[i], V[i], prec, s, m_dev, A_dense, Wp));
    }
    return 0;
}

// An intermediate prediction (lamp/Decoders.py:149-151, lamp/Models.py:130) from the decoder rows, when one is requested.
static int int_pred(Pass& p) {
    const lamp_aux* a = p.aux;
    const int n = p.n_int++;
    if (!a || !a->int_preds || n >= a->n_int_preds || !a->int_preds[n]) return 0;
    return launch_diag(p.w.Y, p.m->w_out, p.nb, p.g.L, p.g.d, a->int_preds[n] + p.b0 * p.g.L, p.s);
}

// One layer of GraphDecoder.forward (lamp/Decoders.py:127-163).  The feed-forward block behind each attention block rides in
// the attention's tail launch when the shape allows (chain.hip: same bits either way); pos_ffn2 follows the self-attention,
// or pos_ffn1 when there is none.
static int decoder_layer(Pass& p, int i) {
    const lamp_model* m = p.m;
    const FwdDims& g = p.g;
    const FwdScratch& w = p.w;
    const lamp_dec_layer& l = m->dec_layers[i];
    const int d = g.d, dff = g.dff, L = g.L;
    const bool last = i + 1 == m->n_layers_dec;
    const int64_t Md = int64_t(p.nb) * L;
    float* Y = w.Y;
    const lamp_chain_pack* pk = m->chain_packs ? m->chain_packs + 2 * i : nullptr;
    bool ffn_ran = false;
    FfnParams f1{Y, Md, d, dff, &l.pos_ffn1, Y, w.H}, f2{Y, Md, d, dff, &l.pos_ffn2, Y, w.H};
    f2.n_labels = L;
    f1.prec = f2.prec = p.prec;
    // the read-out (lamp/Models.py:124-126) rides in the last LayerNorm.  Not with the live encoder: there it is the read-out
    // launch the module-by-module route ends with, so that the two routes agree bit for bit (the fused one sums in another order)
    const bool fused_readout = last && !g.live;
    if (fused_readout) { f2.w_out = m->w_out; f2.logits = p.logits + p.b0 * L; }

    // input->label messages (lamp/Layers.py:35); layer 0's query is the label table itself (its LayerNorm kernel adds the
    // shared residual)
    MhaScratch sc = w.mha;
    if (g.n_ahead) { sc.K = w.K_ahead[i]; sc.V = w.V_ahead[i]; }
    MhaCall enc{i == 0 ? m->tgt_word_emb : Y, p.xk, p.nb, L, g.T, d, g.dk, g.dv, &l.enc_attn, &p.pad_mask, Y,
                p.aux && p.aux->dec_enc_attn ? p.aux->dec_enc_attn[i] : nullptr, p.B, int(p.b0)};
    enc.xq_shared = i == 0; enc.q_ready = i == 0 ? m->dec0_query : nullptr; enc.kv_ready = g.n_ahead > 0;
    enc.keys = &p.sp; enc.keys_packed = p.packed; enc.xkv_dense = p.x;
    enc.act = p.dec_act; enc.prec = p.prec;
    // packs: the projections of both blocks (the K / V projection of the encoder rows usually ran ahead: project_kv_layers)
    const lamp_dec_gemm_pack* dp = p.gp && p.gp->dec ? p.gp->dec + i : nullptr;
    const lamp_kv_gemm_pack* kp = p.kvp ? p.kvp + i : nullptr;
    const float* enc_pk[3] = {dp ? dp->enc_q : nullptr, kp ? kp->enc_k : nullptr, kp ? kp->enc_v : nullptr};
    const float* slf_pk[3] = {dp ? dp->slf_q : nullptr, dp ? dp->slf_k : nullptr, dp ? dp->slf_v : nullptr};
    enc.w_packs = enc_pk;
    LAMP_CK(mha_attend(enc, sc, p.s));
    LAMP_CK(mha_tail(enc, sc, &f1, pk, &ffn_ran, p.s));
    if (!ffn_ran) LAMP_CK(ffn_core(f1, p.s));   // lamp/Layers.py:36

    ffn_ran = false;
    if (l.slf_attn.present) {
        LAMP_CK(int_pred(p));  // dec_output_int, lamp/Decoders.py:149-151
        // label->label messages over the label graph (lamp/Layers.py:40)
        MhaCall slf{Y, Y, p.nb, L, L, d, g.dk, g.dv, &l.slf_attn, &p.label_mask, Y,
                    p.aux && p.aux->dec_self_attn ? p.aux->dec_self_attn[i] : nullptr, p.B, int(p.b0)};
        slf.act = p.dec_act; slf.prec = p.prec; slf.w_packs = slf_pk;
        LAMP_CK(mha_attend(slf, w.mha, p.s));
        LAMP_CK(mha_tail(slf, w.mha, &f2, pk ? pk + 1 : nullptr, &ffn_ran, p.s));
    }
    if (!ffn_ran) LAMP_CK(ffn_core(f2, p.s));   // lamp/Layers.py:45
    if (last && !fused_readout) LAMP_CK(launch_diag(Y, m->w_out, p.nb, L, d, p.logits + p.b0 * L, p.s));
    if (!last) LAMP_CK(int_pred(p));   // all but the last (lamp/Models.py:130)
    return 0;
}

static int onehot_check(const lamp_model* m, const lamp_onehot_frontend* fe, int32_t T) {
    if (!m || !fe) return LAMP_E_NULL;
    if (!fe->t1 || !fe->conv1_b || !fe->conv2_b || (!fe->conv2_w && !fe->conv2_pack)) return LAMP_E_NULL;
    if (fe->n_vocab <= 0 || fe->n_vocab > 16 || fe->taps != 16 || T < 2 || m->d_model <= 0) return LAMP_E_DIMS;
    if (!m->position_enc) return LAMP_E_NULL;   // lamp/Encoders.py:72 adds the position rows unconditionally
    if (m->enc0_emb_w1 || (m->d_model & 3)) return LAMP_E_UNSUPPORTED;
    return 0;
}

// The argument checks of lamp_forward and lamp_onehot_forward (fe), all before any launch.
static int check_forward(const lamp_model* m, const lamp_onehot_frontend* fe, const int64_t* src_seq, const int64_t* src_pos,
                         int32_t B, int32_t T_in, const float* logits, const float* enc_output, const lamp_aux* aux,
                         const void* workspace, FwdDims* g, const lamp_fwd_options* o = nullptr) {
    if (fwd_matmul_prec(o) < 0) return LAMP_E_UNSUPPORTED;   // LAMP_FWD_MATMUL_BF16X3 and _BF16X6 together
    if (fe) LAMP_CK(onehot_check(m, fe, T_in));
    if (!m || !src_seq || (fe && !src_pos) || !logits || !enc_output || !workspace) return LAMP_E_NULL;
    if (B <= 0 || T_in <= 0) return LAMP_E_DIMS;
    if ((!fe && !m->src_word_emb) || !m->tgt_word_emb || !m->w_out) return LAMP_E_NULL;
    if (m->position_enc && !src_pos) return LAMP_E_NULL;
    if (m->enc0_emb_w1 && m->position_enc && !m->enc0_pos_w1) return LAMP_E_NULL;
    if (m->n_layers_dec <= 0) return LAMP_E_DIMS;
    LAMP_CK(fwd_dims(m, fe, T_in, aux && aux->enc_self_attn, g, o && o->enc_self_attn));
    if (g->live) {
        // a live layer 0 starts with the attention, not with W1: the embedding fold has nothing to fold into
        if (m->enc0_emb_w1) return LAMP_E_UNSUPPORTED;
        for (int i = 0; i < m->n_layers_enc; ++i) {
            const lamp_mha_weights& a = m->enc_layers[i].slf_attn;
            if (!a.w_qs || !a.w_ks || !a.w_vs || !a.ln_g || !a.ln_b || (a.n_head > 1 && !a.fc)) return LAMP_E_NULL;
            if (a.n_head < 1 || (a.n_head == 1 && m->d_v != m->d_model)) return LAMP_E_DIMS;
        }
    }
    if (o && o->enc_mask) {
        // one [T, T] byte mask per sample, inside the padded layout
        LAMP_CK(check_mask(o->enc_mask));
        if (o->enc_mask->kind != LAMP_MASK_U8 || o->enc_mask->stride_b == 0 || o->enc_mask->tile_list) return LAMP_E_UNSUPPORTED;
        if (!g->live && !(aux && aux->enc_self_attn)) return LAMP_E_UNSUPPORTED;   // nothing would read it
    }
    if (o && (o->flags & LAMP_FWD_LABEL_BIAS)) {
        // m->label_mask is an fp32 [L, ld] score bias: softmax only, and none of the byte mask's companions
        if ((o->flags & LAMP_FWD_DEC_SIGMOID) || m->label_mask_bits || m->label_tiles || m->label_mask_flags ||
            m->label_mask_allowed)
            return LAMP_E_UNSUPPORTED;
        if (m->label_mask && !aligned16(m->label_mask)) return LAMP_E_ALIGN;
    }
    if ((m->d_model & 3) || (m->d_inner & 3) || (m->d_k & 3) || (m->d_v & 3)) return LAMP_E_UNSUPPORTED;
    if (fe && ((fe->conv2_pack && !aligned16(fe->conv2_pack)) || (!fe->conv2_pack && !aligned16(fe->conv2_w)) ||
               !aligned16(fe->t1) || !aligned16(fe->conv1_b) || !aligned16(workspace)))
        return LAMP_E_ALIGN;
    return 0;
}

// The whole batch in micro-batches that fit `workspace`.  With g.n_ahead, the enc-attention K/V projections of EVERY
// decoder layer (they depend only on the encoder output) are issued as one multi-segment launch right after the encoder.
// Samples are independent and no kernel variant depends on the batch size, so a sample's results are bit-identical for
// every micro-batch split.
static int forward(const lamp_model* m, const lamp_onehot_frontend* fe, const FwdDims& g, const int64_t* src_seq,
                   const int64_t* src_pos, int32_t B, int32_t T_in, float* logits, float* enc_output, const lamp_aux* aux,
                   void* workspace, size_t workspace_bytes, hipStream_t s, const lamp_fwd_options* o = nullptr,
                   const lamp_gemm_packs* gp = nullptr, const lamp_kv_gemm_pack* kvp = nullptr) {
    const Carver size = fwd_size(g);
    if (workspace_bytes < size.bound(1)) return LAMP_E_WORKSPACE;
    const int64_t mb = std::min<int64_t>(B, (workspace_bytes - size.fixed) / size.per);
    Carver c{static_cast<char*>(workspace), size_t(mb)};
    FwdScratch w{};
    fwd_layout(g, c, w);
    if (fe) {   // W2's repack comes first when the caller keeps none
        if (g.w2_repack) LAMP_CK(launch_conv_pack(fe->conv2_w, g.d, g.d, 16, 0, w.w2, s));
        else w.w2 = const_cast<float*>(fe->conv2_pack);
    }

    // Ragged batches.  Every micro-batch first counts its samples' extents on the device (SeqPlan).  Packed: the encoder
    // runs on the packed non-PAD token rows and K / V are projected from them only.  Not packed (the dead encoder
    // self-attention's maps are wanted, wide heads, or the one-hot front end): the padded layout.
    bool packed_live = g.live && o && (o->flags & LAMP_FWD_PACKED_ENCODER) && !o->enc_mask && g.dk == g.dv &&
                       attn_ragged_applies(g.T, g.dk, g.dv);
    for (int i = 0; i < m->n_layers_enc && packed_live; ++i) packed_live = m->enc_layers[i].slf_attn.n_head > 1;
    const bool packed = !(aux && aux->enc_self_attn) && !wide_heads(g.dk, g.dv) && m->n_layers_enc > 0 && !fe &&
                        (!g.live || packed_live);
    // the label graph: bit-packed rows when the caller provides them (one dword per 32-key tile), else bytes
    const int L = g.L;
    lamp_mask label_mask{LAMP_MASK_NONE, 0, nullptr, 0, 0, nullptr, 0};
    if (o && (o->flags & LAMP_FWD_LABEL_BIAS)) {
        if (m->label_mask)   // LAMP_FWD_LABEL_BIAS: the slot holds fp32 rows, (L + 3) & ~3 floats apart (check_forward)
            label_mask = lamp_mask{LAMP_MASK_BIAS_F32, 0, m->label_mask, 0, (L + 3) & ~3, nullptr, 0};
    } else if (m->label_mask_bits)
        label_mask = lamp_mask{LAMP_MASK_BITS_U32, m->label_mask_flags, m->label_mask_bits, 0, (L + 31) / 32, m->label_tiles,
                               (L + 31) / 32 + 1, m->label_mask_allowed};
    else if (m->label_mask)
        label_mask = lamp_mask{LAMP_MASK_U8, 0, m->label_mask, 0, L, m->label_tiles, (L + 31) / 32 + 1};
    for (int64_t b0 = 0; b0 < B; b0 += mb) {
        const int nb = int(std::min<int64_t>(B - b0, mb));
        const int64_t* seq = src_seq + b0 * T_in;
        Pass p{m, fe, g, w, aux, logits, s, B, nb, b0, seq, src_pos ? src_pos + b0 * T_in : nullptr, T_in,
               enc_output + b0 * int64_t(g.T) * g.d, packed, plan_from(w.plan_ints, nb, g.T),
               lamp_mask{LAMP_MASK_KEY_TOKENS_I64, 0, seq, T_in, 0, nullptr, 0}, label_mask};
        p.sp.granules = packed ? w.granules : nullptr;
        lamp_mask enc_mask = p.pad_mask;
        if (o && o->enc_mask) {
            enc_mask = *o->enc_mask;
            enc_mask.ptr = static_cast<const uint8_t*>(enc_mask.ptr) + b0 * enc_mask.stride_b;
        }
        if (g.live) enc_mask.flags |= LAMP_MASK_SELF_RAGGED;   // a sample's kernel and key split: its own length, never T
        p.enc_mask = &enc_mask;
        p.enc_packs = o ? o->enc_chain_packs : nullptr;
        p.dec_act = (o && (o->flags & LAMP_FWD_DEC_SIGMOID)) ? LAMP_ATTN_SIGMOID : LAMP_ATTN_SOFTMAX;
        // LAMP_FWD_MATMUL_*: every linear() of the pass -- encoder FFN, K/V, Q and Q/K/V projections, the separate-launch tails --
        // takes the split kernel (gemm_split.hip); the chain launch, attention, conv2 and the read-out are not linear() calls
        p.prec = fwd_matmul_prec(o);
        p.gp = gp;
        p.kvp = kvp;
        LAMP_CK(!packed ? encode_padded(p) : g.live ? encode_packed_live(p) : encode_packed(p));
        if (g.n_ahead)
            LAMP_CK(project_kv_layers(p.xk, int64_t(nb) * g.T, g.d, g.dk, g.dv, m->dec_layers, g.n_ahead, w.K_ahead,
                                      w.V_ahead, p.prec, s, packed ? p.sp.rows : nullptr, packed ? p.x : nullptr,
                                      kvp));
        for (int i = 0; i < m->n_layers_dec; ++i) LAMP_CK(decoder_layer(p, i));
    }
    return 0;
}

size_t lamp_forward_workspace_bytes(const lamp_model* m, int32_t micro_batch, int32_t T, int32_t want_attn) {
    FwdDims g;
    if (micro_batch <= 0 || fwd_dims(m, nullptr, T, want_attn != 0, &g) != 0) return 0;
    return fwd_size(g).bound(micro_batch);
}

static int forward_tokens(const lamp_model* m, const lamp_fwd_options* o, const int64_t* src_seq, const int64_t* src_pos,
                          int32_t B, int32_t T, float* logits, float* enc_output, const lamp_aux* aux, void* workspace,
                          size_t workspace_bytes, lamp_stream_t stream, const lamp_gemm_packs* gp = nullptr,
                          const lamp_kv_gemm_pack* kvp = nullptr) {
    FwdDims g;
    LAMP_CK(check_forward(m, nullptr, src_seq, src_pos, B, T, logits, enc_output, aux, workspace, &g, o));
    // lamp_forward_workspace_bytes(m, 1, T, want_attn) -- the K/V-ahead buffers counted -- is the least a call accepts, not the
    // smaller layout it falls back to below: what the header documents and what the call checks are one number
    if (workspace_bytes < fwd_size(g).bound(1)) return LAMP_E_WORKSPACE;
    // One launch for every decoder layer's enc-attention K/V projection (they all read the finished encoder output)
    // when the whole batch still fits the workspace with the extra K/V buffers and the weights fit one segment list.
    const bool kv_ahead =
        2 * m->n_layers_dec <= GEMM_MAX_SEG && m->n_layers_dec > 1 && workspace_bytes >= fwd_size(g).bound(size_t(B));
    if (!kv_ahead) g.n_ahead = 0;
    return forward(m, nullptr, g, src_seq, src_pos, B, T, logits, enc_output, aux, workspace, workspace_bytes,
                   hipStream_t(stream), o, gp, kvp);
}

int lamp_forward(const lamp_model* m, const int64_t* src_seq, const int64_t* src_pos, int32_t B, int32_t T,
                 float* logits, float* enc_output, const lamp_aux* aux, void* workspace, size_t workspace_bytes,
                 lamp_stream_t stream) {
    return forward_tokens(m, nullptr, src_seq, src_pos, B, T, logits, enc_output, aux, workspace, workspace_bytes, stream);
}

size_t lamp_forward_opts_workspace_bytes(const lamp_model* m, const lamp_fwd_options* opts, int32_t micro_batch, int32_t T,
                                         int32_t want_attn) {
    FwdDims g;
    if (micro_batch <= 0 || fwd_dims(m, nullptr, T, want_attn != 0, &g, opts && opts->enc_self_attn) != 0) return 0;
    return fwd_size(g).bound(micro_batch);
}

int lamp_forward_opts(const lamp_model* m, const lamp_fwd_options* opts, const int64_t* src_seq, const int64_t* src_pos,
                      int32_t B, int32_t T, float* logits, float* enc_output, const lamp_aux* aux, void* workspace,
                      size_t workspace_bytes, lamp_stream_t stream) {
    return forward_tokens(m, opts, src_seq, src_pos, B, T, logits, enc_output, aux, workspace, workspace_bytes, stream);
}

int lamp_forward_packs(const lamp_model* m, const lamp_fwd_options* opts, const lamp_gemm_packs* packs, const int64_t* src_seq,
                       const int64_t* src_pos, int32_t B, int32_t T, float* logits, float* enc_output, const lamp_aux* aux,
                       void* workspace, size_t workspace_bytes, lamp_stream_t stream) {
    return forward_tokens(m, opts, src_seq, src_pos, B, T, logits, enc_output, aux, workspace, workspace_bytes, stream, packs);
}

int lamp_forward_packs_kv(const lamp_model* m, const lamp_fwd_options* opts, const lamp_gemm_packs* packs, const lamp_kv_gemm_pack* kv_packs,
                          const int64_t* src_seq, const int64_t* src_pos, int32_t B, int32_t T, float* logits, float* enc_output,
                          const lamp_aux* aux, void* workspace, size_t workspace_bytes, lamp_stream_t stream) {
    return forward_tokens(m, opts, src_seq, src_pos, B, T, logits, enc_output, aux, workspace, workspace_bytes, stream, packs, kv_packs);
}

// ------------------------------------------------------------------ one-hot genomics encoder (conv.hip)
size_t lamp_onehot_forward_workspace_bytes(const lamp_model* m, const lamp_onehot_frontend* fe, int32_t micro_batch, int32_t T,
                                           int32_t want_attn) {
    FwdDims g;
    if (micro_batch <= 0 || onehot_check(m, fe, T) != 0 || fwd_dims(m, fe, T, want_attn != 0, &g) != 0) return 0;
    return fwd_size(g).bound(micro_batch);
}

// The encoder sees T / 2 rows of each sample (T tokens, row stride T in src_seq / src_pos) in the padded layout.
int lamp_onehot_forward(const lamp_model* m, const lamp_onehot_frontend* fe, const int64_t* src_seq, const int64_t* src_pos,
                        int32_t B, int32_t T, float* logits, float* enc_output, const lamp_aux* aux, void* workspace,
                        size_t workspace_bytes, lamp_stream_t stream) {
    return lamp_onehot_forward_opts(m, fe, nullptr, src_seq, src_pos, B, T, logits, enc_output, aux, workspace, workspace_bytes,
                                    stream);
}

size_t lamp_onehot_forward_opts_workspace_bytes(const lamp_model* m, const lamp_onehot_frontend* fe, const lamp_fwd_options* opts,
                                                int32_t micro_batch, int32_t T, int32_t want_attn) {
    FwdDims g;
    if (micro_batch <= 0 || onehot_check(m, fe, T) != 0 ||
        fwd_dims(m, fe, T, want_attn != 0, &g, opts && opts->enc_self_attn) != 0)
        return 0;
    return fwd_size(g).bound(micro_batch);
}

int lamp_onehot_forward_opts(const lamp_model* m, const lamp_onehot_frontend* fe, const lamp_fwd_options* opts,
                             const int64_t* src_seq, const int64_t* src_pos, int32_t B, int32_t T, float* logits,
                             float* enc_output, const lamp_aux* aux, void* workspace, size_t workspace_bytes,
                             lamp_stream_t stream) {
    FwdDims g;
    LAMP_CK(check_forward(m, fe, src_seq, src_pos, B, T, logits, enc_output, aux, workspace, &g, opts));
    return forward(m, fe, g, src_seq, src_pos, B, T, logits, enc_output, aux, workspace, workspace_bytes, hipStream_t(stream),
                   opts);
}

int lamp_conv_pack(const float* w, int32_t c_out, int32_t c_in, int32_t taps, int32_t flip, float* packed,
                   lamp_stream_t stream) {
    return launch_conv_pack(w, c_out, c_in, taps, flip, packed, hipStream_t(stream));
}

int lamp_onehot_front_fwd(const int64_t* src_seq, int32_t B, int32_t T, const lamp_onehot_frontend* fe, int32_t d_model,
                          float dropout_p, uint32_t seed, float* xpad, lamp_stream_t stream) {
    if (!fe) return LAMP_E_NULL;
    return launch_front_fwd(src_seq, B, T, fe->t1, fe->n_vocab, fe->conv1_b, d_model, dropout_p, seed, 0, xpad,
                            hipStream_t(stream));
}

int lamp_conv_window_fwd(const float* xpad, int32_t B, int32_t rows_out, int32_t rows_in, int32_t c_in, const float* w_pack,
                         int32_t c_out, const float* bias, int32_t relu, const float* pos_table, int32_t n_position,
                         const int64_t* src_pos, int64_t pos_ld, float* out, float* relu_out, lamp_stream_t stream) {
    if (B <= 0) return LAMP_E_DIMS;
    ConvWindowParams p{xpad, w_pack, bias, out, relu_out, pos_table, src_pos, int64_t(B) * rows_out, c_out, pos_ld,
                       c_out, 16 * c_in, c_in, rows_out, rows_in, relu != 0, n_position};
    return launch_conv_window(p, hipStream_t(stream));
}

int lamp_conv_relu_bwd_pad(const float* dy, const float* relu_out, int32_t B, int32_t rows, int32_t d, float* dz,
                           lamp_stream_t stream) {
    return launch_relu_bwd_pad(dy, relu_out, B, rows, d, dz, hipStream_t(stream));
}

size_t lamp_onehot_front_bwd_partials_bytes(int32_t B, int32_t T, int32_t n_vocab, int32_t d_model) {
    if (B <= 0 || T <= 0 || n_vocab <= 0 || d_model <= 0) return 0;
    return size_t(front_dt1_chunks(B, T)) * n_vocab * 16 * d_model * sizeof(float);
}

int lamp_onehot_front_bwd(const int64_t* src_seq, int32_t B, int32_t T, const lamp_onehot_frontend* fe, int32_t d_model,
                          float dropout_p, uint32_t seed, const float* dP, float* dz, float* partials, size_t partials_bytes,
                          lamp_stream_t stream) {
    if (!fe) return LAMP_E_NULL;
    if (partials_bytes < lamp_onehot_front_bwd_partials_bytes(B, T, fe->n_vocab, d_model)) return LAMP_E_WORKSPACE;
    return launch_front_bwd(src_seq, B, T, fe->t1, fe->n_vocab, fe->conv1_b, d_model, dropout_p, seed, dP, dz, partials,
                            hipStream_t(stream));
}

// ------------------------------------------------------------------ profiling ABI
int lamp_prof_enable(int32_t on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
    return 0;
}

int lamp_prof_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof) {
        (void)hipEventSynchronize(r.e1);
        g_event_pool.push_back(r.e0);
        g_event_pool.push_back(r.e1);
    }
    g_prof.clear();
    return 0;
}

int lamp_prof_read(int32_t kernel_class, int64_t* launches, double* total_ms, double* flops, double* bytes) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    int64_t n = 0;
    double ms = 0, fl = 0, by = 0;
    for (auto& r : g_prof) {
        if (r.cls != kernel_class) continue;
        hipError_t e = hipEventSynchronize(r.e1);
        if (e != hipSuccess) return int(e);
        float t = 0.f;
        e = hipEventElapsedTime(&t, r.e0, r.e1);
        if (e != hipSuccess) return int(e);
        ms += t;
        fl += r.flops;
        by += r.bytes;
        ++n;
    }
    if (launches) *launches = n;
    if (total_ms) *total_ms = ms;
    if (flops) *flops = fl;
    if (bytes) *bytes = by;
    return 0;
}

}  // extern "C"

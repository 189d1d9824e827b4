// The two ends of a training step that are not the model (reference: train.py:37-48, main.py:99).
//
//   bce_train   sigmoid + binary-cross-entropy-with-logits, forward AND backward, of the final prediction and the int_preds
//               intermediates against one target matrix in ONE launch: the probabilities of the final matrix (through a row
//               stride, so they land in an epoch-wide matrix), d loss / d logits of every matrix, and every (matrix, row)'s
//               loss sum.  One wave per (matrix, row); a lane walks the row in steps of 64 and the 64 partial sums are folded
//               by wave64_sum, so the order of every sum is a function of L alone: a row's numbers do not depend on the batch
//               it travels in.  No atomics, no scratch.
//   multilabel_loss_train  the same launch for the objectives of imbalanced label sets: per-label positive weights, focal
//               and asymmetric loss, specialised at compile time on "has an exponent" and "has a margin".
//   optim_step  Adam (torch.optim.Adam's single-tensor arithmetic, no weight decay, no amsgrad) or plain SGD over EVERY
//               parameter of the model in one launch.  The table of (param, grad, exp_avg, exp_avg_sq, numel) travels in the
//               kernel arguments (OPTIM_TABLE entries per launch); a workgroup owns one OPTIM_CHUNK-element chunk of one
//               tensor, found by a binary search over the table's running chunk counts.  16-byte accesses when all four
//               pointers allow it, the chunk's last numel % 4 elements by single lanes; 4-byte accesses otherwise.
//   embed_bwd_ordered  the embedding scatter-add without atomics (see the kernel), so that an epoch is reproducible.
// All are enqueued on the caller's stream; neither allocates, synchronises or reads anything back.
#include "lamp_kernels.h"

namespace lamp {
namespace {

constexpr int BCE_MAX_MATS = 8;
constexpr int OPTIM_TABLE = 72;          // entries per launch: 72 * 40 + 73 * 4 + 32 bytes of arguments (the limit is 4096)
constexpr int OPTIM_CHUNK = 4096;        // elements per workgroup: 256 lanes x 4 rounds x 4 floats

struct BceTrainParams {
    const float* logits[BCE_MAX_MATS];
    float* dlogits[BCE_MAX_MATS];
    float coef[BCE_MAX_MATS];            // weight_k / (n_rows * L): the gradient of the weighted mean
    const float* targets;
    float* probs;
    float* row_loss;
    int64_t n_rows, ld_probs, ld_loss;
    int L, n_mats;
};

__global__ __launch_bounds__(256) void bce_train_kernel(const BceTrainParams p) {
    const int lane = int(threadIdx.x) & 63;
    const int64_t row = int64_t(blockIdx.x) * 4 + (int(threadIdx.x) >> 6);
    const int k = int(blockIdx.y);
    if (row >= p.n_rows) return;
    const float* __restrict__ x_row = p.logits[k] + row * p.L;
    const float* __restrict__ t_row = p.targets + row * p.L;
    float* __restrict__ d_row = p.dlogits[k] ? p.dlogits[k] + row * p.L : nullptr;
    float* __restrict__ p_row = (k == 0 && p.probs) ? p.probs + row * p.ld_probs : nullptr;
    const float coef = p.coef[k];
    float loss = 0.f;
    for (int i = lane; i < p.L; i += 64) {
        const float x = x_row[i], t = t_row[i];
        // e = exp(-|x|) <= 1: sigmoid(|x|) = 1 / (1 + e), sigmoid(-|x|) = e / (1 + e), neither cancels
        const float e = expf(-fabsf(x));
        const float r = 1.0f / (1.0f + e);
        const float big = r, small = e * r;
        const float s = x >= 0.f ? big : small;      // sigmoid(x); a NaN logit gives NaN in e, hence in s, ns and the loss
        const float ns = x >= 0.f ? small : big;     // sigmoid(-x) = 1 - sigmoid(x)
        if (p_row) p_row[i] = s;
        // sigmoid(x) - t = (1 - t) sigmoid(x) - t sigmoid(-x): exact for t = 0 / 1, no cancellation next to t = 1
        if (d_row) d_row[i] = coef * ((1.0f - t) * s - t * ns);
        loss += fmaxf(x, 0.f) - x * t + log1pf(e);
    }
    loss = wave64_sum(loss);
    if (lane == 0 && p.row_loss) p.row_loss[int64_t(k) * p.ld_loss + row] = loss;
}

// bce_train_kernel's geometry with the loss family of lamp_multilabel_loss_train (include/lamp_hip.h):
//   l+ = -ns^g+ log s,   l- = -p^g- log(1 - p),  p = max(s - m, 0),   loss = t w l+ + (1 - t) l-.
// FOCUS: an exponent is set; MARGIN: m > 0.  Neither: per-label positive weights alone, which cost no transcendental beyond
// BCE's own exp and log1p.  log s and log ns come from x, never from s or ns: finite wherever x is, so that ns log ns is 0
// where ns has underflowed.  The powers are exp(g log .); with a margin, p has no logarithm at hand and p^g- is
// p exp((g- - 1) log p), which also is the p^(g- - 1) of the gradient.
struct LossTrainParams {
    BceTrainParams b;
    const float* pos_weight;             // L floats or nullptr
    float gamma_pos, gamma_neg, clip;
};

// wave64_sum's pairing on doubles: the same four DPP steps on both halves of the value, then the four row totals.
template <int CTRL>
__device__ __forceinline__ double dpp_move_f64(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = unsigned(__builtin_amdgcn_update_dpp(0, int(unsigned(u)), CTRL, 0xF, 0xF, true));
    const unsigned hi = unsigned(__builtin_amdgcn_update_dpp(0, int(unsigned(u >> 32)), CTRL, 0xF, 0xF, true));
    return __builtin_bit_cast(double, (unsigned long long)(hi) << 32 | lo);
}
__device__ __forceinline__ double readlane_f64(double v, int src) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = unsigned(__builtin_amdgcn_readlane(int(unsigned(u)), src));
    const unsigned hi = unsigned(__builtin_amdgcn_readlane(int(unsigned(u >> 32)), src));
    return __builtin_bit_cast(double, (unsigned long long)(hi) << 32 | lo);
}
__device__ __forceinline__ double wave64_sum_f64(double v) {
    v += dpp_move_f64<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_move_f64<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_move_f64<0x141>(v);  // row_half_mirror
    v += dpp_move_f64<0x140>(v);  // row_mirror
    return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}

template <bool FOCUS, bool MARGIN>
__global__ __launch_bounds__(256) void multilabel_loss_train_kernel(const LossTrainParams q) {
    const BceTrainParams& p = q.b;
    const int lane = int(threadIdx.x) & 63;
    const int64_t row = int64_t(blockIdx.x) * 4 + (int(threadIdx.x) >> 6);
    const int k = int(blockIdx.y);
    if (row >= p.n_rows) return;
    const float* __restrict__ x_row = p.logits[k] + row * p.L;
    const float* __restrict__ t_row = p.targets + row * p.L;
    const float* __restrict__ w_col = q.pos_weight;
    float* __restrict__ d_row = p.dlogits[k] ? p.dlogits[k] + row * p.L : nullptr;
    float* __restrict__ p_row = (k == 0 && p.probs) ? p.probs + row * p.ld_probs : nullptr;
    const float coef = p.coef[k];
    const float gp = q.gamma_pos, gn = q.gamma_neg, m = q.clip;
    double loss = 0.0;
    for (int i = lane; i < p.L; i += 64) {
        const float x = x_row[i], t = t_row[i];
        const float w = w_col ? w_col[i] : 1.0f;
        const float e = expf(-fabsf(x));             // (as bce_train_kernel: the probabilities are its bits)
        const float r = 1.0f / (1.0f + e);
        const float small = e * r;
        if (p_row) p_row[i] = x >= 0.f ? r : small;
        // the gradient's own larger half: 1 - small carries half an ulp of its own, r the rounding of 1 + e as well.  It
        // shows next to 1, where the gradient is largest and the tolerance an ulp of it
        const float big = 1.0f - small;
        const float s = x >= 0.f ? big : small;
        const float ns = x >= 0.f ? small : big;
        const float l1p = log1pf(e);
        const float ls = fminf(x, 0.f) - l1p;        // log s; a NaN logit is NaN in e, hence in both logs and in l+ below
        const float lns = -fmaxf(x, 0.f) - l1p;      // log ns
        float lpos, dpos, lneg, dneg;                // l+, dl+/dx, l-, dl-/dx
        if (FOCUS) {
            const float f = gp > 0.f ? expf(gp * lns) : 1.0f;         // ns^g+
            lpos = -f * ls;
            dpos = -f * (ns - gp * s * ls);
        } else {
            lpos = -ls;
            dpos = -ns;
        }
        if (MARGIN) {
            const bool on = s > m;                   // off: p = 0, the element is discarded (l- = 0 for every g-)
            const float pm = s - m;
            const float omp = ns + m;                // 1 - p
            const float l1 = log1pf(-pm);            // log(1 - p)
            float pg = 1.0f, dpg = 0.f;              // p^g-, g- p^(g- - 1)
            if (FOCUS && gn > 0.f) {
                const float pgm1 = expf((gn - 1.0f) * logf(pm));
                pg = pgm1 * pm;
                dpg = gn * pgm1;
            }
            lneg = on ? -pg * l1 : 0.f;
            dneg = on ? s * ns * (pg / omp - dpg * l1) : 0.f;
        } else if (FOCUS) {
            const float g = gn > 0.f ? expf(gn * ls) : 1.0f;          // s^g-
            lneg = -g * lns;
            dneg = g * (s - gn * ns * lns);          // s ns (s^g- / ns - g- s^(g- - 1) log ns) without the division by ns
        } else {
            lneg = -lns;
            dneg = s;
        }
        // the two branches are mixed, scaled and summed in double and rounded once: t w, the products and (where one branch
        // is off) the sum are then exact, and a row's sum carries the roundings of its elements, not those of its additions
        const double tw = double(t) * double(w), nt = 1.0 - double(t);
        if (d_row) d_row[i] = float(double(coef) * (tw * double(dpos) + nt * double(dneg)));
        loss += tw * double(lpos) + nt * double(lneg);
    }
    loss = wave64_sum_f64(loss);
    if (lane == 0 && p.row_loss) p.row_loss[int64_t(k) * p.ld_loss + row] = float(loss);
}

struct OptimEntry {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
};

struct OptimParams {
    OptimEntry e[OPTIM_TABLE];
    int32_t chunk_start[OPTIM_TABLE + 1];   // running chunk counts: entry i owns workgroups [chunk_start[i], chunk_start[i + 1])
    int32_t n;
    float lr;            // SGD: the learning rate.  Adam: lr / (1 - beta1^step)
    float beta2;
    float omb1, omb2;    // 1 - beta1, 1 - beta2: taken in double on the host, as torch takes them (1.0f - 0.9f is 2 ulp off 0.1f)
    float inv_bc2_sqrt;  // 1 / sqrt(1 - beta2^step)
    float eps;
};

template <bool ADAM>
__device__ __forceinline__ void optim_update(float& w, float g, float& m, float& v, const OptimParams& p) {
#pragma clang fp contract(off)
    if (ADAM) {
        m = m + (g - m) * p.omb1;                           // exp_avg.lerp_(grad, 1 - beta1)
        v = v * p.beta2 + p.omb2 * g * g;                   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        const float denom = sqrtf(v) * p.inv_bc2_sqrt + p.eps;
        w = w - p.lr * (m / denom);                          // param.addcdiv_(exp_avg, denom, value=-step_size)
    } else {
        w = w - p.lr * g;
    }
}

template <bool ADAM>
__global__ __launch_bounds__(256) void optim_step_kernel(const OptimParams p) {
    const int b = int(blockIdx.x);
    int lo = 0, hi = p.n;            // the entry with chunk_start[lo] <= b < chunk_start[lo + 1] (uniform: scalar loads)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p.chunk_start[mid] <= b) lo = mid; else hi = mid;
    }
    const OptimEntry& t = p.e[lo];
    const int64_t off = int64_t(b - p.chunk_start[lo]) * OPTIM_CHUNK;
    const int64_t left = t.numel - off;
    const int n = left < OPTIM_CHUNK ? int(left) : OPTIM_CHUNK;
    float* __restrict__ w = t.param + off;
    const float* __restrict__ g = t.grad + off;
    float* __restrict__ m = ADAM ? t.exp_avg + off : nullptr;
    float* __restrict__ v = ADAM ? t.exp_avg_sq + off : nullptr;
    const int tid = int(threadIdx.x);
    // off is a multiple of 4096 floats: the chunk is 16-byte aligned iff the tensor is
    const uintptr_t bits = reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(g) |
                           (ADAM ? reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) : uintptr_t(0));
    if ((bits & 15u) == 0) {
        const int nq = n >> 2;
        for (int q = tid; q < nq; q += 256) {
            float4 w4 = reinterpret_cast<float4*>(w)[q];
            const float4 g4 = reinterpret_cast<const float4*>(g)[q];
            float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = m4;
            if (ADAM) {
                m4 = reinterpret_cast<float4*>(m)[q];
                v4 = reinterpret_cast<float4*>(v)[q];
            }
            optim_update<ADAM>(w4.x, g4.x, m4.x, v4.x, p);
            optim_update<ADAM>(w4.y, g4.y, m4.y, v4.y, p);
            optim_update<ADAM>(w4.z, g4.z, m4.z, v4.z, p);
            optim_update<ADAM>(w4.w, g4.w, m4.w, v4.w, p);
            reinterpret_cast<float4*>(w)[q] = w4;
            if (ADAM) {
                reinterpret_cast<float4*>(m)[q] = m4;
                reinterpret_cast<float4*>(v)[q] = v4;
            }
        }
        const int i = (nq << 2) + tid;      // the tail: at most three single lanes
        if (i < n) {
            float wi = w[i], mi = ADAM ? m[i] : 0.f, vi = ADAM ? v[i] : 0.f;
            optim_update<ADAM>(wi, g[i], mi, vi, p);
            w[i] = wi;
            if (ADAM) {
                m[i] = mi;
                v[i] = vi;
            }
        }
    } else {
        for (int i = tid; i < n; i += 256) {
            float wi = w[i], mi = ADAM ? m[i] : 0.f, vi = ADAM ? v[i] : 0.f;
            optim_update<ADAM>(wi, g[i], mi, vi, p);
            w[i] = wi;
            if (ADAM) {
                m[i] = mi;
                v[i] = vi;
            }
        }
    }
}

// lamp_embed_bwd with a fixed order.  One wave per token position.  The wave of a token id's FIRST position owns that id's
// row: it walks the positions from its own on, 64 at a time, and adds the rows of every later occurrence in ascending position
// order -- one writer per row, no atomics.  Waves of later occurrences find an earlier one and leave.  64 * EMB_ACC channels
// per pass; wider tables take further passes.
constexpr int EMB_ACC = 8;
__global__ __launch_bounds__(256) void embed_bwd_ordered_kernel(const int64_t* __restrict__ seq, int64_t n_tok,
                                                                const float* __restrict__ dout, int d, int n_vocab,
                                                                int64_t pad_idx, float* __restrict__ d_emb) {
    const int lane = int(threadIdx.x) & 63;
    const int64_t t = int64_t(blockIdx.x) * 4 + (int(threadIdx.x) >> 6);
    if (t >= n_tok) return;
    const int64_t tok = seq[t];
    if (tok == pad_idx || tok < 0 || tok >= n_vocab) return;
    for (int64_t s0 = 0; s0 < t; s0 += 64) {          // an earlier occurrence owns the row
        const int64_t s = s0 + lane;
        if (__ballot(s < t && seq[s] == tok)) return;
    }
    float* dst = d_emb + tok * d;
    for (int c0 = 0; c0 < d; c0 += 64 * EMB_ACC) {
        float acc[EMB_ACC];
#pragma unroll
        for (int j = 0; j < EMB_ACC; ++j) acc[j] = 0.f;
        for (int64_t s0 = t; s0 < n_tok; s0 += 64) {
            const int64_t s = s0 + lane;
            unsigned long long hit = __ballot(s < n_tok && seq[s] == tok);
            while (hit) {
                const int b = __ffsll((long long)hit) - 1;
                hit &= hit - 1;
                const float* src = dout + (s0 + b) * d + c0;
#pragma unroll
                for (int j = 0; j < EMB_ACC; ++j)
                    if (c0 + lane + 64 * j < d) acc[j] += src[lane + 64 * j];
            }
        }
#pragma unroll
        for (int j = 0; j < EMB_ACC; ++j)
            if (c0 + lane + 64 * j < d) dst[c0 + lane + 64 * j] += acc[j];
    }
}

}  // namespace
}  // namespace lamp

using namespace lamp;

int lamp_bce_logits_train(const float* const* logits, const float* weights, float* const* dlogits, int32_t n_mats,
                          const float* targets, int64_t n_rows, int32_t L, float* probs, int64_t ld_probs, float* row_loss,
                          int64_t ld_row_loss, lamp_stream_t stream) {
    if (n_rows <= 0 || L <= 0 || n_mats <= 0) return LAMP_E_DIMS;
    if (n_mats > BCE_MAX_MATS) return LAMP_E_UNSUPPORTED;
    if (!logits || !weights || !targets) return LAMP_E_NULL;
    if ((probs && ld_probs < L) || (row_loss && n_mats > 1 && ld_row_loss < n_rows)) return LAMP_E_DIMS;
    const int64_t blocks = (n_rows + 3) / 4;
    if (blocks >= (int64_t(1) << 31)) return LAMP_E_UNSUPPORTED;
    BceTrainParams p{};
    const double n_mean = double(n_rows) * double(L);
    for (int k = 0; k < n_mats; ++k) {
        if (!logits[k]) return LAMP_E_NULL;
        p.logits[k] = logits[k];
        p.dlogits[k] = dlogits ? dlogits[k] : nullptr;
        p.coef[k] = float(double(weights[k]) / n_mean);
    }
    p.targets = targets;
    p.probs = probs;
    p.row_loss = row_loss;
    p.n_rows = n_rows;
    p.ld_probs = ld_probs;
    p.ld_loss = ld_row_loss;
    p.L = L;
    p.n_mats = n_mats;
    hipLaunchKernelGGL(bce_train_kernel, dim3(unsigned(blocks), unsigned(n_mats)), dim3(256), 0, hipStream_t(stream), p);
    return int(hipGetLastError());
}

static bool loss_exponent_served(float g) { return g == 0.f || (g >= 1.f && g <= 16.f); }   // (false for NaN and inf)

int lamp_multilabel_loss_train(const float* const* logits, const float* weights, float* const* dlogits, int32_t n_mats,
                               const float* targets, int64_t n_rows, int32_t L, float* probs, int64_t ld_probs, float* row_loss,
                               int64_t ld_row_loss, const lamp_loss_options* opts, lamp_stream_t stream) {
    if (n_rows <= 0 || L <= 0 || n_mats <= 0) return LAMP_E_DIMS;
    if ((probs && ld_probs < L) || (row_loss && n_mats > 1 && ld_row_loss < n_rows)) return LAMP_E_DIMS;
    if (!logits || !weights || !targets) return LAMP_E_NULL;
    for (int k = 0; k < n_mats; ++k)
        if (!logits[k]) return LAMP_E_NULL;
    if (n_mats > BCE_MAX_MATS) return LAMP_E_UNSUPPORTED;
    const int64_t blocks = (n_rows + 3) / 4;
    if (blocks >= (int64_t(1) << 31)) return LAMP_E_UNSUPPORTED;
    if (opts) {
        if (!loss_exponent_served(opts->gamma_pos) || !loss_exponent_served(opts->gamma_neg) ||
            !(opts->clip >= 0.f && opts->clip < 1.f) || opts->reserved != 0)
            return LAMP_E_UNSUPPORTED;
    }
    const bool focus = opts && (opts->gamma_pos != 0.f || opts->gamma_neg != 0.f);
    const bool margin = opts && opts->clip != 0.f;
    if (!focus && !margin && !(opts && opts->pos_weight))      // plain BCE: the kernel it has always been, the same bits
        return lamp_bce_logits_train(logits, weights, dlogits, n_mats, targets, n_rows, L, probs, ld_probs, row_loss, ld_row_loss,
                                     stream);
    LossTrainParams q{};
    BceTrainParams& p = q.b;
    const double n_mean = double(n_rows) * double(L);
    for (int k = 0; k < n_mats; ++k) {
        p.logits[k] = logits[k];
        p.dlogits[k] = dlogits ? dlogits[k] : nullptr;
        p.coef[k] = float(double(weights[k]) / n_mean);
    }
    p.targets = targets;
    p.probs = probs;
    p.row_loss = row_loss;
    p.n_rows = n_rows;
    p.ld_probs = ld_probs;
    p.ld_loss = ld_row_loss;
    p.L = L;
    p.n_mats = n_mats;
    q.pos_weight = opts->pos_weight;
    q.gamma_pos = opts->gamma_pos;
    q.gamma_neg = opts->gamma_neg;
    q.clip = opts->clip;
    const dim3 grid = dim3(unsigned(blocks), unsigned(n_mats)), block = dim3(256);
    if (focus && margin) hipLaunchKernelGGL((multilabel_loss_train_kernel<true, true>), grid, block, 0, hipStream_t(stream), q);
    else if (focus) hipLaunchKernelGGL((multilabel_loss_train_kernel<true, false>), grid, block, 0, hipStream_t(stream), q);
    else if (margin) hipLaunchKernelGGL((multilabel_loss_train_kernel<false, true>), grid, block, 0, hipStream_t(stream), q);
    else hipLaunchKernelGGL((multilabel_loss_train_kernel<false, false>), grid, block, 0, hipStream_t(stream), q);
    return int(hipGetLastError());
}

int lamp_embed_bwd_ordered(const int64_t* src_seq, int64_t n_tokens, const float* dout, int32_t d_model, int32_t n_vocab,
                           int64_t pad_idx, float* d_emb, lamp_stream_t stream) {
    if (n_tokens <= 0 || d_model <= 0 || n_vocab <= 0) return LAMP_E_DIMS;
    if (!src_seq || !dout || !d_emb) return LAMP_E_NULL;
    const int64_t g = (n_tokens + 3) / 4;
    if (g > 0x7fffffffLL) return LAMP_E_DIMS;
    hipLaunchKernelGGL(embed_bwd_ordered_kernel, dim3(unsigned(g)), dim3(256), 0, hipStream_t(stream), src_seq, n_tokens, dout,
                       d_model, n_vocab, pad_idx, d_emb);
    return int(hipGetLastError());
}

int lamp_optim_step(const lamp_optim_entry* entries, int32_t n, int32_t kind, int64_t step, double lr, double beta1,
                    double beta2, double eps, lamp_stream_t stream) {
    static_assert(sizeof(OptimEntry) == sizeof(lamp_optim_entry), "the table is copied entry by entry");
    static_assert(sizeof(OptimParams) <= 4096, "kernel arguments");
    if (n < 0) return LAMP_E_DIMS;
    if (n == 0) return LAMP_OK;
    if (!entries) return LAMP_E_NULL;
    if (kind != LAMP_OPTIM_ADAM && kind != LAMP_OPTIM_SGD) return LAMP_E_UNSUPPORTED;
    if (kind == LAMP_OPTIM_ADAM && step < 1) return LAMP_E_DIMS;
    for (int i = 0; i < n; ++i) {
        const lamp_optim_entry& e = entries[i];
        if (e.numel < 0) return LAMP_E_DIMS;
        if (e.numel == 0) continue;      // (an empty tensor has no storage to point to)
        if (!e.param || !e.grad || (kind == LAMP_OPTIM_ADAM && (!e.exp_avg || !e.exp_avg_sq))) return LAMP_E_NULL;
        if ((reinterpret_cast<uintptr_t>(e.param) | reinterpret_cast<uintptr_t>(e.grad) |
             reinterpret_cast<uintptr_t>(e.exp_avg) | reinterpret_cast<uintptr_t>(e.exp_avg_sq)) & 3u)
            return LAMP_E_ALIGN;
    }
    OptimParams p{};
    p.beta2 = float(beta2);
    p.omb1 = float(1.0 - beta1);
    p.omb2 = float(1.0 - beta2);
    p.eps = float(eps);
    if (kind == LAMP_OPTIM_ADAM) {   // the scalars torch computes on the host in double (torch/optim/adam.py, _single_tensor_adam)
        const double bc1 = 1.0 - pow(beta1, double(step));
        const double bc2 = 1.0 - pow(beta2, double(step));
        p.lr = float(lr / bc1);
        p.inv_bc2_sqrt = float(1.0 / sqrt(bc2));
    } else {
        p.lr = float(lr);
        p.inv_bc2_sqrt = 1.f;
    }
    hipStream_t s = hipStream_t(stream);
    int i = 0;
    while (i < n) {
        int cnt = 0;
        int64_t chunks = 0;
        for (; i < n && cnt < OPTIM_TABLE; ++i) {
            const lamp_optim_entry& e = entries[i];
            if (e.numel == 0) continue;
            const int64_t c = (e.numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK;
            if (chunks + c >= (int64_t(1) << 31)) {
                if (cnt == 0) return LAMP_E_UNSUPPORTED;
                break;
            }
            p.e[cnt] = OptimEntry{e.param, e.grad, e.exp_avg, e.exp_avg_sq, e.numel};
            p.chunk_start[cnt] = int32_t(chunks);
            chunks += c;
            ++cnt;
        }
        if (cnt == 0) break;
        p.chunk_start[cnt] = int32_t(chunks);
        p.n = cnt;
        if (kind == LAMP_OPTIM_ADAM)
            hipLaunchKernelGGL(optim_step_kernel<true>, dim3(unsigned(chunks)), dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL(optim_step_kernel<false>, dim3(unsigned(chunks)), dim3(256), 0, s, p);
        if (hipError_t e = hipGetLastError()) return int(e);
    }
    return LAMP_OK;
}

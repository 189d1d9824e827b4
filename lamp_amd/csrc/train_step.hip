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
//   rank_loss_train  the same launch for ranking objectives: LSEP in O(L) per row (one wave per (matrix, row)), and the pairwise
//               hinge and logistic losses over the pairs that exist (one workgroup per (matrix, row), the row's positives and
//               negatives compacted in LDS, every element against the opposite class only), each plus a share of the mean BCE.
//   optim_step  Adam (torch.optim.Adam's single-tensor arithmetic, no weight decay, no amsgrad) or plain SGD over EVERY
//               parameter of the model in one launch.  The table of (param, grad, exp_avg, exp_avg_sq, numel) travels in the
//               kernel arguments (OPTIM_TABLE entries per launch); a workgroup owns one OPTIM_CHUNK-element chunk of one
//               tensor.
//   grad_norm   the global L2 norm of a table's gradients in fp64, one partial per chunk and one closing workgroup: the device
//               record {norm, scale, finite, 0} that optim_step_ext reads.  No atomics.
//   optim_step_ext  optim_step behind gradient clipping (the record's scale, applied in registers), per-entry weight decay
//               (L2 or decoupled), SGD momentum, and "write nothing when the norm is not finite".
//   weight_average / weight_swap  an average of the weights (EMA, SWA) kept beside them: torch's lerp of (param, exp_avg) over the
//               optimizer's table in optim_step's geometry, and the exchange of the two; walk_chunk2 is their two-pointer walk.
//   embed_bwd_ordered  the embedding scatter-add without atomics (see the kernel), so that an epoch is reproducible.
// All are enqueued on the caller's stream; neither allocates, synchronises or reads anything back.
//
// What the entries share, each written once:
//   device  table_entry()      a workgroup's table entry, by binary search over the running chunk counts (the three table kernels)
//           walk_chunk()       the walk over one chunk -- 16-byte path, tail lanes, 4-byte path -- with the update passed in
//                              (optim_step and optim_step_ext; grad_norm only reads g and keeps its own loop)
//           block_sum_f64()    a workgroup's fp64 sum (grad_norm's two stages, the pair kernels)
//           bce_element()      the BCE term of the rank kernels.  bce_train_kernel keeps its own copy on purpose (see there).
//   host    check_loss_args() / fill_loss_params()   the argument rules of multilabel and rank, the parameter fill of all three
//           for_each_launch()  cuts a table into launches of OPTIM_TABLE entries with their chunk counts (all three table entries)
//           check_optim_entries() / set_optim_scalars()   the per-entry rules and the step's scalars (optim_step, optim_step_ext)
// The order in which an entry answers a call that breaks two rules is its own (lamp_bce_logits_train's differs from the
// other two loss entries'); tests/test_train_step_refusals_cpu.py holds every such answer.
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
        // (bce_element's arithmetic, a second copy on purpose: through bce_element this kernel takes other registers and schedule)
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

// A 256-lane workgroup's sum of one double per lane: the lanes of a wave by wave64_sum_f64, the four waves as
// (w0 + w1) + (w2 + w3) through red[4].  A caller that sums twice through one red puts a barrier between the two calls.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    v = wave64_sum_f64(v);
    const int tid = int(threadIdx.x);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- lamp_rank_loss_train (include/lamp_hip.h): a row's positives against its negatives ------------------------------
constexpr int RANK_PAIR_MAX_L = 4096;    // HINGE / LOGISTIC: the row lives in LDS (16 KB of logits + 8 KB of column numbers)

struct RankTrainParams {
    const float* logits[BCE_MAX_MATS];
    float* dlogits[BCE_MAX_MATS];
    double coef[BCE_MAX_MATS];           // weight_k / n_rows
    const float* targets;
    float* probs;
    float* row_loss;
    int64_t n_rows, ld_probs, ld_loss;
    double beta_over_L;                  // bce_weight / L (0: the ranking term alone, the BCE term is not evaluated)
    float margin;
    int L;
};

__device__ __forceinline__ float wave64_max(float v) {       // wave64_sum's steps with fmaxf (which drops a NaN)
    v = fmaxf(v, dpp_move<0xB1>(v));
    v = fmaxf(v, dpp_move<0x4E>(v));
    v = fmaxf(v, dpp_move<0x141>(v));
    v = fmaxf(v, dpp_move<0x140>(v));
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// bce_train_kernel's element: the probability (its bits), d bce / dx and the loss term
__device__ __forceinline__ void bce_element(float x, float t, float& s, float& dx, float& loss) {
    const float e = expf(-fabsf(x));
    const float r = 1.0f / (1.0f + e);
    const float big = r, small = e * r;
    s = x >= 0.f ? big : small;
    const float ns = x >= 0.f ? small : big;
    dx = (1.0f - t) * s - t * ns;
    loss = fmaxf(x, 0.f) - x * t + log1pf(e);
}

// LSEP in bce_train_kernel's geometry, one wave per (matrix, row), three passes over the row (the second and third hit the
// cache): class maxima and counts (+ the BCE side), the two exponential sums in double, the gradients.
//   R = softplus(z), z = (max_N + log sum_n exp(x_n - max_N)) + (max_P + log sum_p exp(-x_p - max_P)), in double;
//   dR/dx_n = sigmoid(z) exp(x_n - max_N) / sum_N,  dR/dx_p = -sigmoid(z) exp(-x_p - max_P) / sum_P.
__global__ __launch_bounds__(256) void rank_lsep_train_kernel(const RankTrainParams p) {
    const int lane = int(threadIdx.x) & 63;
    const int64_t row = int64_t(blockIdx.x) * 4 + (int(threadIdx.x) >> 6);
    const int k = int(blockIdx.y);
    if (row >= p.n_rows) return;
    const int L = p.L;
    const float* __restrict__ x_row = p.logits[k] + row * L;
    const float* __restrict__ t_row = p.targets + row * L;
    float* __restrict__ d_row = p.dlogits[k] ? p.dlogits[k] + row * L : nullptr;
    float* __restrict__ p_row = (k == 0 && p.probs) ? p.probs + row * p.ld_probs : nullptr;
    const bool mix = p.beta_over_L != 0.0;
    const float NEG_INF = -__builtin_inff();
    float max_n = NEG_INF, max_p = NEG_INF;
    int n_p = 0;
    bool nan = false;
    double bce = 0.0;
    for (int c = 0; c < L; c += 64) {                // (whole waves to the ballot)
        const int i = c + lane;
        const bool valid = i < L;
        const float x = valid ? x_row[i] : 0.f, t = valid ? t_row[i] : 0.f;
        const bool pos = valid && t > 0.5f;
        n_p += __builtin_popcountll(__builtin_amdgcn_ballot_w64(pos));
        if (valid) {
            nan |= x != x;
            if (pos) max_p = fmaxf(max_p, -x);
            else max_n = fmaxf(max_n, x);
            if (p_row || mix) {
                float s, dx, l;
                bce_element(x, t, s, dx, l);
                if (p_row) p_row[i] = s;
                bce += double(l);
            }
        }
    }
    const bool has_nan = __builtin_amdgcn_ballot_w64(nan) != 0;
    const bool ranked = n_p > 0 && n_p < L;          // an empty class: R = 0, no ranking gradient
    double R = 0.0, g_n = 0.0, g_p = 0.0;            // g_n = sigmoid(z) / sum_N, g_p = -sigmoid(z) / sum_P
    if (ranked) {
        max_n = wave64_max(max_n);
        max_p = wave64_max(max_p);
        double sum_n = 0.0, sum_p = 0.0;
        for (int i = lane; i < L; i += 64) {
            const float x = x_row[i];
            if (t_row[i] > 0.5f) sum_p += double(expf(-x - max_p));
            else sum_n += double(expf(x - max_n));
        }
        sum_n = wave64_sum_f64(sum_n);
        sum_p = wave64_sum_f64(sum_p);
        const double z = (double(max_n) + log(sum_n)) + (double(max_p) + log(sum_p));
        const double ez = exp(-fabs(z));
        const double sig = z >= 0.0 ? 1.0 / (1.0 + ez) : ez / (1.0 + ez);
        R = fmax(z, 0.0) + log1p(ez);
        g_n = sig / sum_n;
        g_p = -sig / sum_p;
    }
    const double NAN64 = __builtin_nan("");
    if (d_row) {
        const double coef = p.coef[k];
        for (int i = lane; i < L; i += 64) {
            const float x = x_row[i], t = t_row[i];
            double g = 0.0;
            if (ranked) g = t > 0.5f ? g_p * double(expf(-x - max_p)) : g_n * double(expf(x - max_n));
            if (mix) {
                float s, dx, l;
                bce_element(x, t, s, dx, l);
                g += p.beta_over_L * double(dx);
            }
            d_row[i] = float(has_nan ? NAN64 : coef * g);
        }
    }
    if (mix) R += p.beta_over_L * wave64_sum_f64(bce);
    if (lane == 0 && p.row_loss) p.row_loss[int64_t(k) * p.ld_loss + row] = float(has_nan ? NAN64 : R);
}

// The pair kinds: one workgroup per (matrix, row).  The row's logits are compacted into LDS in column order, positives in
// xs[0, n_p), negatives in xs[n_p, L), col[] the column of each slot; wave w compacts columns [w Q, (w + 1) Q) by ballots, its
// offsets from one count pass.  An element then loops over the OPPOSITE class only: n_p n_n evaluations per direction.

// One element against slots [lo, hi) of the opposite class -> LOGISTIC: sum of sigmoid(x_n - x_p); HINGE: the number of
// active pairs.  The negatives' direction also takes the loss.
template <int KIND, bool NEG_OWN>
__device__ __forceinline__ double pair_range(const float* xs, float x_own, int lo, int hi, float margin, double& loss) {
    double g = 0.0;
    int active = 0;
    for (int o = lo; o < hi; ++o) {
        const float d = NEG_OWN ? x_own - xs[o] : xs[o] - x_own;      // x_n - x_p
        if (KIND == LAMP_RANK_HINGE) {
            const float a = margin + d;                               // the difference first, then the margin
            const bool on = a > 0.f;
            active += on ? 1 : 0;
            if (NEG_OWN) loss += on ? double(a) : 0.0;
        } else {
            const float e = expf(-fabsf(d));
            const float r = 1.0f / (1.0f + e);
            g += double(d >= 0.f ? r : e * r);
            if (NEG_OWN) loss += double(fmaxf(d, 0.f)) + double(log1pf(e));
        }
    }
    return KIND == LAMP_RANK_HINGE ? double(active) : g;
}

struct RankRow {                 // what finishing a slot needs
    const float* t_row;
    float* d_row;
    double coef, inv_pairs, beta_over_L;
    bool has_nan;
};

template <bool NEG_OWN>
__device__ __forceinline__ void rank_finish_slot(const RankRow& r, const float* xs, const unsigned short* col, int slot, double g) {
    if (!r.d_row) return;
    const int c = int(col[slot]);
    double v = NEG_OWN ? g * r.inv_pairs : -(g * r.inv_pairs);
    if (r.beta_over_L != 0.0) {
        float s, dx, l;
        bce_element(xs[slot], r.t_row[c], s, dx, l);
        v += r.beta_over_L * double(dx);
    }
    r.d_row[c] = float(r.has_nan ? __builtin_nan("") : r.coef * v);
}

// Every element of one class against the other.  With fewer than 256 own elements the opposite class is cut into S slices
// (S a power of two, own_cnt S <= 256), one (slice, element) per thread, the S partial sums of an element added in slice
// order: the order of every sum is a function of (n_p, n_n).
template <int KIND, bool NEG_OWN>
__device__ __forceinline__ void rank_direction(const RankRow& r, const float* xs, const unsigned short* col, double* part,
                                               int own_base, int own_cnt, int opp_base, int opp_cnt, float margin, int tid,
                                               double& loss) {
    if (own_cnt <= 0) return;                        // (uniform over the workgroup, like every branch around a barrier here)
    if (own_cnt >= 256 || opp_cnt <= 1) {
        for (int e = tid; e < own_cnt; e += 256) {
            const double g = pair_range<KIND, NEG_OWN>(xs, xs[own_base + e], opp_base, opp_base + opp_cnt, margin, loss);
            rank_finish_slot<NEG_OWN>(r, xs, col, own_base + e, g);
        }
        return;
    }
    const int S = 1 << (31 - __builtin_clz(256 / own_cnt));
    const int len = (opp_cnt + S - 1) / S;
    if (tid < own_cnt * S) {
        const int s = tid / own_cnt, e = tid - s * own_cnt;
        const int lo = min(s * len, opp_cnt), hi = min(lo + len, opp_cnt);
        part[tid] = pair_range<KIND, NEG_OWN>(xs, xs[own_base + e], opp_base + lo, opp_base + hi, margin, loss);
    }
    __syncthreads();
    if (tid < own_cnt) {
        double g = 0.0;
        for (int s = 0; s < S; ++s) g += part[s * own_cnt + tid];
        rank_finish_slot<NEG_OWN>(r, xs, col, own_base + tid, g);
    }
    __syncthreads();                                 // (part is the next direction's)
}

template <int KIND>
__global__ __launch_bounds__(256) void rank_pair_train_kernel(const RankTrainParams p) {
    __shared__ float xs[RANK_PAIR_MAX_L];
    __shared__ unsigned short col[RANK_PAIR_MAX_L];
    __shared__ double part[256];
    __shared__ double red[4];
    __shared__ int wave_pos[4];
    const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int64_t row = int64_t(blockIdx.x);
    const int k = int(blockIdx.y);
    const int L = p.L;
    const float* __restrict__ x_row = p.logits[k] + row * L;
    const float* __restrict__ t_row = p.targets + row * L;
    float* __restrict__ p_row = (k == 0 && p.probs) ? p.probs + row * p.ld_probs : nullptr;
    const bool mix = p.beta_over_L != 0.0;
    const int Q = ((L + 255) >> 8) << 6;             // columns per wave, a multiple of 64
    const int lo = min(wave * Q, L), hi = min(lo + Q, L);
    int mine = 0;
    for (int c = lo; c < hi; c += 64) {
        const int i = c + lane;
        mine += __builtin_popcountll(__builtin_amdgcn_ballot_w64(i < hi && t_row[min(i, hi - 1)] > 0.5f));
    }
    if (lane == 0) wave_pos[wave] = mine;
    __syncthreads();
    int n_p = 0, base_p = 0;
    for (int w = 0; w < 4; ++w) {
        base_p += w < wave ? wave_pos[w] : 0;
        n_p += wave_pos[w];
    }
    const int n_n = L - n_p;
    int base_n = n_p + (lo - base_p);
    bool nan = false;
    double bce = 0.0;
    for (int c = lo; c < hi; c += 64) {
        const int i = c + lane;
        const bool valid = i < hi;
        const float x = valid ? x_row[i] : 0.f, t = valid ? t_row[i] : 0.f;
        const bool pos = valid && t > 0.5f;
        const unsigned long long m_pos = __builtin_amdgcn_ballot_w64(pos), m_neg = __builtin_amdgcn_ballot_w64(valid && !pos);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (valid) {
            const int slot = pos ? base_p + __builtin_popcountll(m_pos & below) : base_n + __builtin_popcountll(m_neg & below);
            xs[slot] = x;
            col[slot] = (unsigned short)(i);
            nan |= x != x;
            if (p_row || mix) {
                float s, dx, l;
                bce_element(x, t, s, dx, l);
                if (p_row) p_row[i] = s;
                bce += double(l);
            }
        }
        base_p += __builtin_popcountll(m_pos);
        base_n += __builtin_popcountll(m_neg);
    }
    RankRow r;
    r.has_nan = __syncthreads_or(nan ? 1 : 0) != 0;  // (also: xs and col are complete)
    r.t_row = t_row;
    r.d_row = p.dlogits[k] ? p.dlogits[k] + row * L : nullptr;
    r.coef = p.coef[k];
    r.beta_over_L = p.beta_over_L;
    const double pairs = double(n_p) * double(n_n);
    r.inv_pairs = pairs > 0.0 ? 1.0 / pairs : 0.0;   // an empty class: the loops below are empty and R = 0
    double loss = 0.0;
    rank_direction<KIND, true>(r, xs, col, part, n_p, n_n, 0, n_p, p.margin, tid, loss);
    if (r.d_row) {
        double unused = 0.0;
        rank_direction<KIND, false>(r, xs, col, part, 0, n_p, n_p, n_n, p.margin, tid, unused);
    }
    __syncthreads();                                 // (nothing has used red yet: the barrier this kernel has always had here)
    double R = block_sum_f64(loss, red) * r.inv_pairs;
    if (mix) {
        __syncthreads();                             // (red is still being read from the sum before)
        R += p.beta_over_L * block_sum_f64(bce, red);
    }
    if (tid == 0 && p.row_loss) p.row_loss[int64_t(k) * p.ld_loss + row] = float(r.has_nan ? __builtin_nan("") : R);
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

// The table entry that owns workgroup b: chunk_start[lo] <= b < chunk_start[lo + 1] (uniform: scalar loads).
__device__ __forceinline__ int table_entry(const int32_t* chunk_start, int n, int b) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_start[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// One workgroup's walk over the OPTIM_CHUNK elements of entry t from element `off` on: update(w, g, m, v) on every element,
// the moments the kernel has (HAS_M, HAS_V) loaded before it and stored after it.  16-byte accesses when every pointer allows
// them, the chunk's last numel % 4 elements by single lanes; 4-byte accesses otherwise.
template <bool HAS_M, bool HAS_V, class Update>
__device__ __forceinline__ void walk_chunk(const OptimEntry& t, int64_t off, Update update) {
    const int64_t left = t.numel - off;
    const int n = left < OPTIM_CHUNK ? int(left) : OPTIM_CHUNK;
    float* __restrict__ w = t.param + off;
    const float* __restrict__ g = t.grad + off;
    float* __restrict__ m = HAS_M ? t.exp_avg + off : nullptr;
    float* __restrict__ v = HAS_V ? t.exp_avg_sq + off : nullptr;
    const int tid = int(threadIdx.x);
    // off is a multiple of 4096 floats: the chunk is 16-byte aligned iff the tensor is
    const uintptr_t bits = reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(g) |
                           (HAS_M ? reinterpret_cast<uintptr_t>(m) : uintptr_t(0)) |
                           (HAS_V ? reinterpret_cast<uintptr_t>(v) : uintptr_t(0));
    if ((bits & 15u) == 0) {
        const int nq = n >> 2;
        for (int q = tid; q < nq; q += 256) {
            float4 w4 = reinterpret_cast<float4*>(w)[q];
            const float4 g4 = reinterpret_cast<const float4*>(g)[q];
            float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = m4;
            if (HAS_M) m4 = reinterpret_cast<float4*>(m)[q];
            if (HAS_V) v4 = reinterpret_cast<float4*>(v)[q];
            update(w4.x, g4.x, m4.x, v4.x);
            update(w4.y, g4.y, m4.y, v4.y);
            update(w4.z, g4.z, m4.z, v4.z);
            update(w4.w, g4.w, m4.w, v4.w);
            reinterpret_cast<float4*>(w)[q] = w4;
            if (HAS_M) reinterpret_cast<float4*>(m)[q] = m4;
            if (HAS_V) reinterpret_cast<float4*>(v)[q] = v4;
        }
        const int i = (nq << 2) + tid;      // the tail: at most three single lanes
        if (i < n) {
            float wi = w[i], mi = HAS_M ? m[i] : 0.f, vi = HAS_V ? v[i] : 0.f;
            update(wi, g[i], mi, vi);
            w[i] = wi;
            if (HAS_M) m[i] = mi;
            if (HAS_V) v[i] = vi;
        }
    } else {
        for (int i = tid; i < n; i += 256) {
            float wi = w[i], mi = HAS_M ? m[i] : 0.f, vi = HAS_V ? v[i] : 0.f;
            update(wi, g[i], mi, vi);
            w[i] = wi;
            if (HAS_M) m[i] = mi;
            if (HAS_V) v[i] = vi;
        }
    }
}

template <bool ADAM>
__global__ __launch_bounds__(256) void optim_step_kernel(const OptimParams p) {
    const int b = int(blockIdx.x);
    const int lo = table_entry(p.chunk_start, p.n, b);
    walk_chunk<ADAM, ADAM>(p.e[lo], int64_t(b - p.chunk_start[lo]) * OPTIM_CHUNK,
                           [&](float& w, float g, float& m, float& v) { optim_update<ADAM>(w, g, m, v, p); });
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

// ---- lamp_grad_norm: the global L2 norm of every gradient of a table, in two stages, without atomics ----
// Stage 1 has optim_step_kernel's geometry: one workgroup per OPTIM_CHUNK of one entry.  A lane squares its elements in
// double (the square of an fp32 number is exact there: no overflow below 3.4e38, no underflow) and adds them in the order
// it walks them; the 64 lanes of a wave fold by wave64_sum_f64, the four waves as (w0 + w1) + (w2 + w3); one double per
// workgroup goes to partial[blockIdx.x].
struct NormParams {
    const float* grad[OPTIM_TABLE];
    int64_t numel[OPTIM_TABLE];
    int32_t chunk_start[OPTIM_TABLE + 1];
    int32_t n;
    double* partial;     // this launch's first partial
};

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const NormParams p) {
    __shared__ double red[4];
    const int b = int(blockIdx.x);
    const int lo = table_entry(p.chunk_start, p.n, b);
    const int64_t off = int64_t(b - p.chunk_start[lo]) * OPTIM_CHUNK;
    const int64_t left = p.numel[lo] - off;
    const int n = left < OPTIM_CHUNK ? int(left) : OPTIM_CHUNK;
    const float* __restrict__ g = p.grad[lo] + off;
    const int tid = int(threadIdx.x);
    double acc = 0.0;
    if ((reinterpret_cast<uintptr_t>(g) & 15u) == 0) {
        const int nq = n >> 2;
        for (int q = tid; q < nq; q += 256) {
            const float4 g4 = reinterpret_cast<const float4*>(g)[q];
            acc += double(g4.x) * double(g4.x);
            acc += double(g4.y) * double(g4.y);
            acc += double(g4.z) * double(g4.z);
            acc += double(g4.w) * double(g4.w);
        }
        const int i = (nq << 2) + tid;
        if (i < n) acc += double(g[i]) * double(g[i]);
    } else {
        for (int i = tid; i < n; i += 256) acc += double(g[i]) * double(g[i]);
    }
    const double total = block_sum_f64(acc, red);
    if (tid == 0) p.partial[b] = total;
}

// Stage 2, one workgroup: lane t adds partials t, t + 256, ... in ascending order, lanes and waves fold as in stage 1, and
// lane 0 writes the record {norm, scale, finite, 0}.  scale is clip_grad_norm_'s own fp32 expression,
// clamp(max_norm * reciprocal(norm + 1e-6), max=1) -- `max_norm / tensor` is reciprocal().mul() in torch -- and keeps a NaN.
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double* __restrict__ partial, int64_t n_partials,
                                                              float max_norm, int clip, float* __restrict__ grad_state,
                                                              int32_t* __restrict__ skipped) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int tid = int(threadIdx.x);
    double acc = 0.0;
    for (int64_t i = tid; i < n_partials; i += 256) acc += partial[i];
    const double total = block_sum_f64(acc, red);
    if (tid == 0) {
        const float norm = float(sqrt(total));
        float scale = 1.0f;
        if (clip) {
            const float coef = (1.0f / (norm + 1e-6f)) * max_norm;
            scale = coef > 1.0f ? 1.0f : coef;
        }
        const bool finite = fabsf(norm) <= 3.402823466e38f;      // (false for inf and NaN)
        grad_state[0] = norm;
        grad_state[1] = scale;
        grad_state[2] = finite ? 1.0f : 0.0f;
        grad_state[3] = 0.0f;
        if (skipped && !finite) skipped[0] = skipped[0] + 1;
    }
}

// ---- lamp_optim_step_ext: optim_step_kernel's geometry and arithmetic behind the clip factor, weight decay and momentum ----
enum { OPT_ADAM = 0, OPT_SGD = 1, OPT_SGD_MOMENTUM = 2 };
enum { DECAY_NONE = 0, DECAY_L2 = 1, DECAY_DECOUPLED = 2 };

struct OptimExtParams {
    OptimParams o;
    float decay[OPTIM_TABLE];     // per entry: weight_decay (L2 form) or float(1 - lr * weight_decay) (decoupled form)
    const float* grad_state;      // {norm, scale, finite, 0} of lamp_grad_norm, or nullptr
    float momentum;
    int32_t decay_mode;           // DECAY_L2 / DECAY_DECOUPLED: what `decay` holds (an entry with weight_decay 0 takes neither)
    int32_t skip_nonfinite;
};

struct OptimExtStep {             // what is uniform over a workgroup
    float scale, decay, momentum;
    bool clip;
    int decay_mode;
};

template <int KIND>
__device__ __forceinline__ void optim_update_ext(float& w, float g, float& m, float& v, const OptimParams& p, const OptimExtStep& s) {
#pragma clang fp contract(off)
    if (s.clip) g = g * s.scale;                             // clip_grad_norm_'s grad.mul_(clip_coef), kept in a register
    if (s.decay_mode == DECAY_L2) g = g + s.decay * w;       // grad.add(param, alpha=weight_decay)
    else if (s.decay_mode == DECAY_DECOUPLED) w = w * s.decay;   // param.mul_(1 - lr * weight_decay)
    if (KIND == OPT_SGD_MOMENTUM) {
        m = s.momentum * m + g;                              // buf.mul_(momentum).add_(grad)
        w = w - p.lr * m;                                    // param.add_(buf, alpha=-lr)
    } else {
        optim_update<KIND == OPT_ADAM>(w, g, m, v, p);
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void optim_step_ext_kernel(const OptimExtParams x) {
    constexpr bool HAS_M = KIND != OPT_SGD, HAS_V = KIND == OPT_ADAM;
    const OptimParams& p = x.o;
    OptimExtStep s;
    s.clip = x.grad_state != nullptr;
    s.scale = 1.0f;
    if (s.clip) {
        if (x.skip_nonfinite && x.grad_state[2] == 0.0f) return;     // a non-finite norm: this launch writes nothing
        s.scale = x.grad_state[1];
    }
    s.momentum = x.momentum;
    const int b = int(blockIdx.x);
    const int lo = table_entry(p.chunk_start, p.n, b);
    const OptimEntry& t = p.e[lo];
    s.decay = x.decay[lo];
    // an entry without decay takes exactly optim_step_kernel's arithmetic: 0 * w would turn an infinite weight into NaN
    s.decay_mode = (x.decay_mode == DECAY_L2 && s.decay != 0.0f) || (x.decay_mode == DECAY_DECOUPLED && s.decay != 1.0f)
                       ? x.decay_mode : DECAY_NONE;
    walk_chunk<HAS_M, HAS_V>(t, int64_t(b - p.chunk_start[lo]) * OPTIM_CHUNK,
                             [&](float& w, float g, float& m, float& v) { optim_update_ext<KIND>(w, g, m, v, p, s); });
}

// ---- lamp_weight_average / lamp_weight_swap: optim_step_kernel's geometry over the two pointers (param, exp_avg) ----------
// The table is OptimParams itself (grad and exp_avg_sq are carried and never read); the only scalar, the weight, travels in
// `lr`.  1 - w is taken in fp32 as torch takes it; it is only used for w >= 0.5, where it is exact.
// torch's lerp (ATen/native/Lerp.h) with a = the average, p = the weight:  w < 0.5: a + w (p - a);  else p - (p - a)(1 - w).
// Two deviations (include/lamp_hip.h): w == 1 copies the bits, and an element with p == a keeps a (-inf - -inf would be NaN).
template <bool COPY>
__device__ __forceinline__ void average_update(float p, float& a, float w) {
#pragma clang fp contract(off)
    if (COPY) {
        a = p;
    } else if (p != a) {                                    // (a NaN on either side compares unequal and spreads)
        const float d = p - a;
        a = w < 0.5f ? a + w * d : p - d * (1.0f - w);
    }
}

// walk_chunk's walk for two pointers: update(p, a) with both loaded before it and both stored after it when STORE_P (the swap),
// p read only otherwise (the average).  COPY / swap move 32-bit patterns: a float4 load and store keep a NaN's payload.
template <bool STORE_P, class Update>
__device__ __forceinline__ void walk_chunk2(const OptimEntry& t, int64_t off, Update update) {
    const int64_t left = t.numel - off;
    const int n = left < OPTIM_CHUNK ? int(left) : OPTIM_CHUNK;
    float* __restrict__ p = t.param + off;
    float* __restrict__ a = t.exp_avg + off;
    const int tid = int(threadIdx.x);
    // off is a multiple of 4096 floats: the chunk is 16-byte aligned iff the tensor is
    if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(a)) & 15u) == 0) {
        const int nq = n >> 2;
        for (int q = tid; q < nq; q += 256) {
            float4 p4 = reinterpret_cast<const float4*>(p)[q];
            float4 a4 = reinterpret_cast<float4*>(a)[q];
            update(p4.x, a4.x);
            update(p4.y, a4.y);
            update(p4.z, a4.z);
            update(p4.w, a4.w);
            if (STORE_P) reinterpret_cast<float4*>(p)[q] = p4;
            reinterpret_cast<float4*>(a)[q] = a4;
        }
        const int i = (nq << 2) + tid;      // the tail: at most three single lanes
        if (i < n) {
            float pi = p[i], ai = a[i];
            update(pi, ai);
            if (STORE_P) p[i] = pi;
            a[i] = ai;
        }
    } else {
        for (int i = tid; i < n; i += 256) {
            float pi = p[i], ai = a[i];
            update(pi, ai);
            if (STORE_P) p[i] = pi;
            a[i] = ai;
        }
    }
}

template <bool COPY>
__global__ __launch_bounds__(256) void weight_average_kernel(const OptimParams p) {
    const int b = int(blockIdx.x);
    const int lo = table_entry(p.chunk_start, p.n, b);
    const float w = p.lr;
    walk_chunk2<false>(p.e[lo], int64_t(b - p.chunk_start[lo]) * OPTIM_CHUNK,
                       [&](float& x, float& a) { average_update<COPY>(x, a, w); });
}

__global__ __launch_bounds__(256) void weight_swap_kernel(const OptimParams p) {
    const int b = int(blockIdx.x);
    const int lo = table_entry(p.chunk_start, p.n, b);
    walk_chunk2<true>(p.e[lo], int64_t(b - p.chunk_start[lo]) * OPTIM_CHUNK, [](float& x, float& a) {
        const float t = x;
        x = a;
        a = t;
    });
}

}  // namespace
}  // namespace lamp

using namespace lamp;

// ---- the loss entries' shared host side -------------------------------------------------------------------------------
// The argument rules lamp_multilabel_loss_train and lamp_rank_loss_train answer in one order: sizes and leading dimensions
// (DIMS), then the three arrays and the first n_checked matrices (NULL).  lamp_bce_logits_train keeps an order of its own
// (tests/test_train_step_refusals_cpu.py pins both).
static int check_loss_args(const float* const* logits, const float* weights, int32_t n_mats, int32_t n_checked, const float* targets,
                           int64_t n_rows, int32_t L, const float* probs, int64_t ld_probs, const float* row_loss,
                           int64_t ld_row_loss) {
    if (n_rows <= 0 || L <= 0 || n_mats <= 0) return LAMP_E_DIMS;
    if ((probs && ld_probs < L) || (row_loss && n_mats > 1 && ld_row_loss < n_rows)) return LAMP_E_DIMS;
    if (!logits || !weights || !targets) return LAMP_E_NULL;
    for (int k = 0; k < n_checked; ++k)
        if (!logits[k]) return LAMP_E_NULL;
    return LAMP_OK;
}

// What BceTrainParams and RankTrainParams have in common: the matrices, their coefficients weight_k / denom (taken in double,
// rounded to the struct's own type), the target and output pointers, the strides and L.
template <class Params>
static void fill_loss_params(Params& p, const float* const* logits, const float* weights, float* const* dlogits, int32_t n_mats,
                             double denom, const float* targets, int64_t n_rows, int32_t L, float* probs, int64_t ld_probs,
                             float* row_loss, int64_t ld_row_loss) {
    for (int k = 0; k < n_mats; ++k) {
        p.logits[k] = logits[k];
        p.dlogits[k] = dlogits ? dlogits[k] : nullptr;
        p.coef[k] = decltype(+p.coef[0])(double(weights[k]) / denom);
    }
    p.targets = targets;
    p.probs = probs;
    p.row_loss = row_loss;
    p.n_rows = n_rows;
    p.ld_probs = ld_probs;
    p.ld_loss = ld_row_loss;
    p.L = L;
}

int lamp_bce_logits_train(const float* const* logits, const float* weights, float* const* dlogits, int32_t n_mats,
                          const float* targets, int64_t n_rows, int32_t L, float* probs, int64_t ld_probs, float* row_loss,
                          int64_t ld_row_loss, lamp_stream_t stream) {
    // this entry's own order of answers (the oldest of the three; unifying them would change recorded statuses)
    if (n_rows <= 0 || L <= 0 || n_mats <= 0) return LAMP_E_DIMS;
    if (n_mats > BCE_MAX_MATS) return LAMP_E_UNSUPPORTED;
    if (!logits || !weights || !targets) return LAMP_E_NULL;
    if ((probs && ld_probs < L) || (row_loss && n_mats > 1 && ld_row_loss < n_rows)) return LAMP_E_DIMS;
    const int64_t blocks = (n_rows + 3) / 4;
    if (blocks >= (int64_t(1) << 31)) return LAMP_E_UNSUPPORTED;
    for (int k = 0; k < n_mats; ++k)
        if (!logits[k]) return LAMP_E_NULL;
    BceTrainParams p{};
    fill_loss_params(p, logits, weights, dlogits, n_mats, double(n_rows) * double(L), targets, n_rows, L, probs, ld_probs, row_loss,
                     ld_row_loss);
    p.n_mats = n_mats;
    hipLaunchKernelGGL(bce_train_kernel, dim3(unsigned(blocks), unsigned(n_mats)), dim3(256), 0, hipStream_t(stream), p);
    return int(hipGetLastError());
}

static bool loss_exponent_served(float g) { return g == 0.f || (g >= 1.f && g <= 16.f); }   // (false for NaN and inf)

int lamp_multilabel_loss_train(const float* const* logits, const float* weights, float* const* dlogits, int32_t n_mats,
                               const float* targets, int64_t n_rows, int32_t L, float* probs, int64_t ld_probs, float* row_loss,
                               int64_t ld_row_loss, const lamp_loss_options* opts, lamp_stream_t stream) {
    if (int st = check_loss_args(logits, weights, n_mats, n_mats, targets, n_rows, L, probs, ld_probs, row_loss, ld_row_loss)) return st;
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
    fill_loss_params(q.b, logits, weights, dlogits, n_mats, double(n_rows) * double(L), targets, n_rows, L, probs, ld_probs, row_loss,
                     ld_row_loss);
    q.b.n_mats = n_mats;
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

static bool rank_weight_served(float v) { return v >= 0.f && v <= 3.402823466e38f; }   // finite and >= 0 (false for NaN)

int lamp_rank_loss_train(const float* const* logits, const float* weights, float* const* dlogits, int32_t n_mats,
                         const float* targets, int64_t n_rows, int32_t L, float* probs, int64_t ld_probs, float* row_loss,
                         int64_t ld_row_loss, const lamp_rank_loss_options* opts, lamp_stream_t stream) {
    // (the matrices beyond BCE_MAX_MATS are not looked at: n_mats is refused further down)
    if (int st = check_loss_args(logits, weights, n_mats, n_mats < BCE_MAX_MATS ? n_mats : BCE_MAX_MATS, targets, n_rows, L, probs,
                                 ld_probs, row_loss, ld_row_loss))
        return st;
    if (!opts) return LAMP_E_NULL;
    const int kind = opts->kind;
    if (kind != LAMP_RANK_LSEP && kind != LAMP_RANK_HINGE && kind != LAMP_RANK_LOGISTIC) return LAMP_E_UNSUPPORTED;
    if (!rank_weight_served(opts->margin) || !rank_weight_served(opts->bce_weight)) return LAMP_E_UNSUPPORTED;
    if ((kind != LAMP_RANK_HINGE && opts->margin != 0.f) || opts->reserved != 0) return LAMP_E_UNSUPPORTED;
    if (n_mats > BCE_MAX_MATS) return LAMP_E_UNSUPPORTED;
    if (kind != LAMP_RANK_LSEP && L > RANK_PAIR_MAX_L) return LAMP_E_UNSUPPORTED;
    if (n_rows >= (int64_t(1) << 31)) return LAMP_E_UNSUPPORTED;
    RankTrainParams p{};
    fill_loss_params(p, logits, weights, dlogits, n_mats, double(n_rows), targets, n_rows, L, probs, ld_probs, row_loss, ld_row_loss);
    p.beta_over_L = double(opts->bce_weight) / double(L);
    p.margin = opts->margin;
    const hipStream_t s = hipStream_t(stream);
    if (kind == LAMP_RANK_LSEP)
        hipLaunchKernelGGL(rank_lsep_train_kernel, dim3(unsigned((n_rows + 3) / 4), unsigned(n_mats)), dim3(256), 0, s, p);
    else if (kind == LAMP_RANK_HINGE)
        hipLaunchKernelGGL((rank_pair_train_kernel<LAMP_RANK_HINGE>), dim3(unsigned(n_rows), unsigned(n_mats)), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((rank_pair_train_kernel<LAMP_RANK_LOGISTIC>), dim3(unsigned(n_rows), unsigned(n_mats)), dim3(256), 0, s, p);
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

// ---- the optimizer entries' shared host side --------------------------------------------------------------------------
// The table batcher: cuts a table into launches of at most OPTIM_TABLE non-empty entries.  put(slot, i) stores entries[i] in
// the launch's slot, chunk_start[] takes the running chunk counts and n_slots the count, launch(chunks) enqueues.  A launch ends
// in front of the entry that would take it to 2^31 chunks; an entry that has that many alone is LAMP_E_UNSUPPORTED (after the
// launches in front of it).
template <class Put, class Launch>
static int for_each_launch(const lamp_optim_entry* entries, int32_t n, int32_t* chunk_start, int32_t& n_slots, Put put, Launch launch) {
    int i = 0;
    while (i < n) {
        int cnt = 0;
        int64_t chunks = 0;
        for (; i < n && cnt < OPTIM_TABLE; ++i) {
            if (entries[i].numel == 0) continue;     // (an empty tensor has no storage to point to)
            const int64_t c = (entries[i].numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK;
            if (chunks + c >= (int64_t(1) << 31)) {
                if (cnt == 0) return LAMP_E_UNSUPPORTED;
                break;
            }
            put(cnt, i);
            chunk_start[cnt] = int32_t(chunks);
            chunks += c;
            ++cnt;
        }
        if (cnt == 0) break;
        chunk_start[cnt] = int32_t(chunks);
        n_slots = cnt;
        launch(chunks);
        if (hipError_t e = hipGetLastError()) return int(e);
    }
    return LAMP_OK;
}

// Every non-empty entry of an optimizer step: numel (DIMS), the pointers its kind reads (NULL), 4-byte alignment (ALIGN).
static int check_optim_entries(const lamp_optim_entry* entries, int32_t n, bool needs_m, bool needs_v) {
    for (int i = 0; i < n; ++i) {
        const lamp_optim_entry& e = entries[i];
        if (e.numel < 0) return LAMP_E_DIMS;
        if (e.numel == 0) continue;
        if (!e.param || !e.grad || (needs_m && !e.exp_avg) || (needs_v && !e.exp_avg_sq)) return LAMP_E_NULL;
        if ((reinterpret_cast<uintptr_t>(e.param) | reinterpret_cast<uintptr_t>(e.grad) |
             reinterpret_cast<uintptr_t>(e.exp_avg) | reinterpret_cast<uintptr_t>(e.exp_avg_sq)) & 3u)
            return LAMP_E_ALIGN;
    }
    return LAMP_OK;
}

// The scalars of a step, computed in double as torch computes them on the host (torch/optim/adam.py, _single_tensor_adam) and
// rounded once.
static void set_optim_scalars(OptimParams& p, int32_t kind, int64_t step, double lr, double beta1, double beta2, double eps) {
    p.beta2 = float(beta2);
    p.omb1 = float(1.0 - beta1);
    p.omb2 = float(1.0 - beta2);
    p.eps = float(eps);
    if (kind == LAMP_OPTIM_ADAM) {
        const double bc1 = 1.0 - pow(beta1, double(step));
        const double bc2 = 1.0 - pow(beta2, double(step));
        p.lr = float(lr / bc1);
        p.inv_bc2_sqrt = float(1.0 / sqrt(bc2));
    } else {
        p.lr = float(lr);
        p.inv_bc2_sqrt = 1.f;
    }
}

static OptimEntry optim_entry(const lamp_optim_entry& e) { return OptimEntry{e.param, e.grad, e.exp_avg, e.exp_avg_sq, e.numel}; }

int lamp_optim_step(const lamp_optim_entry* entries, int32_t n, int32_t kind, int64_t step, double lr, double beta1,
                    double beta2, double eps, lamp_stream_t stream) {
    static_assert(sizeof(OptimEntry) == sizeof(lamp_optim_entry), "the table is copied entry by entry");
    static_assert(sizeof(OptimParams) <= 4096, "kernel arguments");
    if (n < 0) return LAMP_E_DIMS;
    if (n == 0) return LAMP_OK;
    if (!entries) return LAMP_E_NULL;
    if (kind != LAMP_OPTIM_ADAM && kind != LAMP_OPTIM_SGD) return LAMP_E_UNSUPPORTED;
    const bool adam = kind == LAMP_OPTIM_ADAM;
    if (adam && step < 1) return LAMP_E_DIMS;
    if (int st = check_optim_entries(entries, n, adam, adam)) return st;
    OptimParams p{};
    set_optim_scalars(p, kind, step, lr, beta1, beta2, eps);
    const hipStream_t s = hipStream_t(stream);
    return for_each_launch(
        entries, n, p.chunk_start, p.n, [&](int slot, int i) { p.e[slot] = optim_entry(entries[i]); },
        [&](int64_t chunks) {
            if (adam) hipLaunchKernelGGL(optim_step_kernel<true>, dim3(unsigned(chunks)), dim3(256), 0, s, p);
            else hipLaunchKernelGGL(optim_step_kernel<false>, dim3(unsigned(chunks)), dim3(256), 0, s, p);
        });
}

// The chunk count of a table, or -1 when an entry's numel is negative / the count leaves int32 (the partials are indexed by it).
static int64_t grad_norm_chunks(const lamp_optim_entry* entries, int32_t n) {
    int64_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        if (entries[i].numel < 0) return -1;
        chunks += (entries[i].numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK;
        if (chunks >= (int64_t(1) << 31)) return -1;
    }
    return chunks;
}

size_t lamp_grad_norm_workspace_bytes(const lamp_optim_entry* entries, int32_t n) {
    if (n <= 0 || !entries) return 0;
    const int64_t chunks = grad_norm_chunks(entries, n);
    return chunks < 0 ? 0 : size_t(chunks) * sizeof(double);
}

int lamp_grad_norm(const lamp_optim_entry* entries, int32_t n, double max_norm, void* workspace, size_t workspace_bytes,
                   float* grad_state, int32_t* skipped, lamp_stream_t stream) {
    static_assert(sizeof(NormParams) <= 4096, "kernel arguments");
    if (n < 0) return LAMP_E_DIMS;
    if (n > 0 && !entries) return LAMP_E_NULL;
    if (!grad_state) return LAMP_E_NULL;
    if (max_norm != max_norm) return LAMP_E_UNSUPPORTED;
    for (int i = 0; i < n; ++i)
        if (entries[i].numel < 0) return LAMP_E_DIMS;
    const int64_t total = grad_norm_chunks(entries, n);
    if (total < 0) return LAMP_E_UNSUPPORTED;      // 2^31 chunks or more: the batcher below never has to cut for them
    for (int i = 0; i < n; ++i) {
        if (entries[i].numel == 0) continue;
        if (!entries[i].grad) return LAMP_E_NULL;
        if (reinterpret_cast<uintptr_t>(entries[i].grad) & 3u) return LAMP_E_ALIGN;
    }
    if ((reinterpret_cast<uintptr_t>(grad_state) & 3u) || (reinterpret_cast<uintptr_t>(skipped) & 3u) ||
        (reinterpret_cast<uintptr_t>(workspace) & 7u))
        return LAMP_E_ALIGN;
    if (total > 0 && !workspace) return LAMP_E_NULL;
    if (workspace_bytes < size_t(total) * sizeof(double)) return LAMP_E_WORKSPACE;
    const hipStream_t s = hipStream_t(stream);
    NormParams p{};
    int64_t done = 0;
    const int st = for_each_launch(
        entries, n, p.chunk_start, p.n,
        [&](int slot, int i) {
            p.grad[slot] = entries[i].grad;
            p.numel[slot] = entries[i].numel;
        },
        [&](int64_t chunks) {
            p.partial = static_cast<double*>(workspace) + done;
            hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(unsigned(chunks)), dim3(256), 0, s, p);
            done += chunks;
        });
    if (st) return st;
    const bool clip = max_norm >= 0.0;
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, s, static_cast<const double*>(workspace), done,
                       clip ? float(max_norm) : 0.0f, clip ? 1 : 0, grad_state, skipped);
    return int(hipGetLastError());
}

int lamp_optim_step_ext(const lamp_optim_entry* entries, int32_t n, int32_t kind, int64_t step, double lr, double beta1,
                        double beta2, double eps, const lamp_optim_ext* ext, lamp_stream_t stream) {
    static_assert(sizeof(OptimExtParams) <= 4096, "kernel arguments");
    if (!ext) return lamp_optim_step(entries, n, kind, step, lr, beta1, beta2, eps, stream);
    if (n < 0) return LAMP_E_DIMS;
    if (kind != LAMP_OPTIM_ADAM && kind != LAMP_OPTIM_SGD) return LAMP_E_UNSUPPORTED;
    if ((ext->flags & ~(LAMP_OPTIM_DECOUPLED_DECAY | LAMP_OPTIM_SKIP_NONFINITE)) || ext->reserved != 0) return LAMP_E_UNSUPPORTED;
    if (!(ext->momentum >= 0.0 && ext->momentum < 1.0)) return LAMP_E_UNSUPPORTED;       // (NaN fails both)
    if (ext->momentum != 0.0 && kind != LAMP_OPTIM_SGD) return LAMP_E_UNSUPPORTED;
    const bool decoupled = (ext->flags & LAMP_OPTIM_DECOUPLED_DECAY) != 0;
    const bool skip = (ext->flags & LAMP_OPTIM_SKIP_NONFINITE) != 0;
    if (decoupled && kind != LAMP_OPTIM_ADAM) return LAMP_E_UNSUPPORTED;
    if (skip && !ext->grad_state) return LAMP_E_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(ext->grad_state) & 3u) return LAMP_E_ALIGN;
    if (n == 0) return LAMP_OK;
    if (!entries) return LAMP_E_NULL;
    bool any_decay = false;
    if (ext->entry_weight_decay)
        for (int i = 0; i < n; ++i) {
            const float wd = ext->entry_weight_decay[i];
            if (!(wd >= 0.f && wd <= 3.402823466e38f)) return LAMP_E_UNSUPPORTED;      // negative, infinite or NaN
            any_decay |= wd != 0.f;
        }
    const bool mom = ext->momentum != 0.0;
    if (!any_decay && !mom && !ext->grad_state)      // nothing asked for: the kernel it has always been, the same bits
        return lamp_optim_step(entries, n, kind, step, lr, beta1, beta2, eps, stream);
    const bool adam = kind == LAMP_OPTIM_ADAM;
    if (adam && step < 1) return LAMP_E_DIMS;
    if (int st = check_optim_entries(entries, n, adam || mom, adam)) return st;
    OptimExtParams x{};
    OptimParams& p = x.o;
    set_optim_scalars(p, kind, step, lr, beta1, beta2, eps);
    x.grad_state = ext->grad_state;
    x.momentum = float(ext->momentum);
    x.decay_mode = !any_decay ? DECAY_NONE : decoupled ? DECAY_DECOUPLED : DECAY_L2;
    x.skip_nonfinite = skip ? 1 : 0;
    const hipStream_t s = hipStream_t(stream);
    return for_each_launch(
        entries, n, p.chunk_start, p.n,
        [&](int slot, int i) {
            p.e[slot] = optim_entry(entries[i]);
            const float wd = any_decay ? ext->entry_weight_decay[i] : 0.f;
            // AdamW's factor is taken in double on the host and rounded once, as torch passes it to param.mul_
            x.decay[slot] = x.decay_mode == DECAY_DECOUPLED ? float(1.0 - lr * double(wd)) : wd;
        },
        [&](int64_t chunks) {
            const dim3 grid = dim3(unsigned(chunks)), block = dim3(256);
            if (adam) hipLaunchKernelGGL(optim_step_ext_kernel<OPT_ADAM>, grid, block, 0, s, x);
            else if (mom) hipLaunchKernelGGL(optim_step_ext_kernel<OPT_SGD_MOMENTUM>, grid, block, 0, s, x);
            else hipLaunchKernelGGL(optim_step_ext_kernel<OPT_SGD>, grid, block, 0, s, x);
        });
}

// ---- lamp_weight_average / lamp_weight_swap ---------------------------------------------------------------------------
// The rules of both (check_optim_entries' order over the two pointers they read): numel (DIMS), param / exp_avg (NULL),
// 4-byte alignment (ALIGN), a param and an exp_avg that overlap without being identical (UNSUPPORTED).  `skip` says whether
// an entry with identical pointers -- a no-op -- exists: the table is then copied without them.
static int check_average_entries(const lamp_optim_entry* entries, int32_t n, bool& skip) {
    skip = false;
    for (int i = 0; i < n; ++i) {
        const lamp_optim_entry& e = entries[i];
        if (e.numel < 0) return LAMP_E_DIMS;
        if (e.numel == 0) continue;
        if (!e.param || !e.exp_avg) return LAMP_E_NULL;
        const uintptr_t p = reinterpret_cast<uintptr_t>(e.param), a = reinterpret_cast<uintptr_t>(e.exp_avg);
        if ((p | a) & 3u) return LAMP_E_ALIGN;
        if (p == a) {
            skip = true;
            continue;
        }
        const uintptr_t gap = p < a ? a - p : p - a;
        if (gap / sizeof(float) < uintptr_t(e.numel)) return LAMP_E_UNSUPPORTED;
    }
    return LAMP_OK;
}

// 2^31 chunks in one entry, asked before any launch (for_each_launch would answer after the launches in front of it)
static bool average_chunks_served(const lamp_optim_entry* entries, int32_t n) {
    for (int i = 0; i < n; ++i)
        if ((entries[i].numel + OPTIM_CHUNK - 1) / OPTIM_CHUNK >= (int64_t(1) << 31)) return false;
    return true;
}

template <class Launch>
static int average_launches(const lamp_optim_entry* entries, int32_t n, bool skip, OptimParams& p, Launch launch) {
    if (!skip)
        return for_each_launch(entries, n, p.chunk_start, p.n, [&](int slot, int i) { p.e[slot] = optim_entry(entries[i]); }, launch);
    lamp_optim_entry* kept = new lamp_optim_entry[n];
    int m = 0;
    for (int i = 0; i < n; ++i)
        if (entries[i].numel == 0 || entries[i].param != entries[i].exp_avg) kept[m++] = entries[i];
    const int st = for_each_launch(kept, m, p.chunk_start, p.n, [&](int slot, int i) { p.e[slot] = optim_entry(kept[i]); }, launch);
    delete[] kept;
    return st;
}

int lamp_weight_average(const lamp_optim_entry* entries, int32_t n, double weight, lamp_stream_t stream) {
    if (n < 0) return LAMP_E_DIMS;
    if (!(weight >= 0.0 && weight <= 1.0)) return LAMP_E_UNSUPPORTED;      // (NaN fails both)
    if (n == 0) return LAMP_OK;
    if (!entries) return LAMP_E_NULL;
    bool skip = false;
    if (int st = check_average_entries(entries, n, skip)) return st;
    if (!average_chunks_served(entries, n)) return LAMP_E_UNSUPPORTED;
    const float w = float(weight);
    if (w == 0.f) return LAMP_OK;                    // the average keeps its bits: nothing to launch
    OptimParams p{};
    p.lr = w;
    const hipStream_t s = hipStream_t(stream);
    return average_launches(entries, n, skip, p, [&](int64_t chunks) {
        if (w == 1.f) hipLaunchKernelGGL(weight_average_kernel<true>, dim3(unsigned(chunks)), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(weight_average_kernel<false>, dim3(unsigned(chunks)), dim3(256), 0, s, p);
    });
}

int lamp_weight_swap(const lamp_optim_entry* entries, int32_t n, lamp_stream_t stream) {
    if (n < 0) return LAMP_E_DIMS;
    if (n == 0) return LAMP_OK;
    if (!entries) return LAMP_E_NULL;
    bool skip = false;
    if (int st = check_average_entries(entries, n, skip)) return st;
    if (!average_chunks_served(entries, n)) return LAMP_E_UNSUPPORTED;
    OptimParams p{};
    const hipStream_t s = hipStream_t(stream);
    return average_launches(entries, n, skip, p, [&](int64_t chunks) {
        hipLaunchKernelGGL(weight_swap_kernel, dim3(unsigned(chunks)), dim3(256), 0, s, p);
    });
}

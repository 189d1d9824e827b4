// Per-label decision thresholds fitted on the device (the reference's Find_Optimal_Cutoff, utils/evals.py:301-313, whose use
// at :335-336 is commented out because its pandas / sklearn loop is too slow per epoch), and the thresholded counts at a
// threshold per label.
//
//   key build + sort   shared with lamp_ranking_metrics (metrics.hip: rank_sort_columns): label-major u32 keys
//                      (bits(score) << 1) | target, every column ascending, and the per-label "cannot be ranked" flags.
//   tune walk          one workgroup per label.  A first pass over the sorted column counts its positives P (every criterion
//                      weighs a candidate against P, and N = n - P).  The second pass streams the column from its high end
//                      (score descending) in tiles of 1024 keys: tp by a wave scan with a carry between tiles, a group end where
//                      the next key's score differs.  Every group end is a candidate (tp, cnt); every thread keeps its best
//                      one, compared in integers; one fixed-order reduction picks the label's.  The candidate "predict nothing"
//                      is (0, 0), where every thread starts.  A candidate's position cnt orders the candidates by threshold
//                      descending, so "the smallest c on a tie" is "the smallest cnt".
//   counts             threshold_counts_kernel of metrics.hip with the slab's thresholds staged in LDS.
// The sorted column is a function of the column's multiset and the choice is made in integers: results are bit-identical from
// run to run and under any permutation of the rows.  Nothing here allocates, synchronises or writes its inputs; all of it is
// enqueued on the caller's stream.
#include "lamp_kernels.h"

namespace lamp {
namespace {

constexpr int WALK_ITEMS = 4;            // consecutive keys per thread and tile
constexpr int WALK_TILE = 256 * WALK_ITEMS;
constexpr uint32_t KEY_PAD = 0xFFFFFFFFu;   // above every key (keys are <= 0x7F000001); its group id equals no real one
constexpr int VEC_SLAB = 2048;           // labels whose counters and thresholds one workgroup of the counts keeps in LDS (32 KiB)

__device__ __forceinline__ int lane_id() { return int(threadIdx.x) & 63; }

__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane_id() >= o) v += u;
    }
    return v;
}

// Candidate a = (tp_a, cnt_a) against b: > 0 a is better, 0 they tie, < 0 b is better.  Integers only (n < 2^31: tp, cnt, P, N
// < 2^31, so cnt + P < 2^32, tp (cnt + P) < 2^63, tp N, fp P and P N < 2^62).
template <int CRIT>
__device__ __forceinline__ int cand_cmp(uint32_t tp_a, uint32_t cnt_a, uint32_t tp_b, uint32_t cnt_b, uint32_t P, uint32_t N) {
    if (CRIT == LAMP_TUNE_F1) {   // 2 tp / (cnt + P)
        const unsigned long long l = static_cast<unsigned long long>(tp_a) * (static_cast<unsigned long long>(cnt_b) + P);
        const unsigned long long r = static_cast<unsigned long long>(tp_b) * (static_cast<unsigned long long>(cnt_a) + P);
        return l > r ? 1 : (l < r ? -1 : 0);
    }
    const long long p = P, q = N;
    long long va = static_cast<long long>(tp_a) * q, vb = static_cast<long long>(tp_b) * q;
    const long long fa = static_cast<long long>(cnt_a - tp_a) * p, fb = static_cast<long long>(cnt_b - tp_b) * p;
    if (CRIT == LAMP_TUNE_YOUDEN) {   // tp N - fp P
        va -= fa;
        vb -= fb;
    } else {   // -|tp N + fp P - P N|
        va += fa - p * q;
        vb += fb - p * q;
        va = va < 0 ? va : -va;
        vb = vb < 0 ? vb : -vb;
    }
    return va > vb ? 1 : (va < vb ? -1 : 0);
}

// Position i of the walk is array index n - 1 - i (score descending); the candidate that ends at position i has cnt = i + 1.
template <int CRIT>
__global__ __launch_bounds__(256) void tune_walk_kernel(const uint32_t* __restrict__ keys, int64_t n64,
                                                        const uint32_t* __restrict__ invalid, float fallback,
                                                        float* __restrict__ threshold, int* __restrict__ out_tp,
                                                        int* __restrict__ out_fp, int* __restrict__ n_pos,
                                                        int* __restrict__ n_neg, int* __restrict__ tuned) {
    __shared__ uint32_t s_sum[4];
    __shared__ uint32_t r_tp[256];
    __shared__ uint32_t r_cnt[256];
    const int tid = int(threadIdx.x), lane = lane_id(), w = tid >> 6;
    const uint32_t n = uint32_t(n64);
    const uint32_t* col = keys + int64_t(blockIdx.x) * n64;
    // the column's positives
    uint32_t ones = 0;
    for (uint32_t i = uint32_t(tid); i < n; i += 256) ones += col[i] & 1u;
    const uint32_t ones_incl = wave_incl_sum(ones);
    if (lane == 63) s_sum[w] = ones_incl;
    __syncthreads();
    const uint32_t P = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]), N = n - P;
    __syncthreads();   // s_sum is rewritten by the first tile
    uint32_t carry_tp = 0;
    uint32_t best_tp = 0, best_cnt = 0;   // c = 0: predict nothing
    for (uint32_t tile = 0; tile < n; tile += WALK_TILE) {
        const uint32_t i0 = tile + uint32_t(tid) * WALK_ITEMS;
        uint32_t k[WALK_ITEMS + 1];
#pragma unroll
        for (int j = 0; j <= WALK_ITEMS; ++j) {
            const uint32_t i = i0 + j;
            k[j] = (i0 < n && i < n) ? col[n - 1 - i] : KEY_PAD;
        }
        uint32_t local = 0;
#pragma unroll
        for (int j = 0; j < WALK_ITEMS; ++j) local += (k[j] != KEY_PAD) ? (k[j] & 1u) : 0u;
        const uint32_t incl = wave_incl_sum(local);
        if (lane == 63) s_sum[w] = incl;
        __syncthreads();
        uint32_t run = carry_tp + incl - local;
        uint32_t tile_total = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < w) run += s_sum[q];
            tile_total += s_sum[q];
        }
#pragma unroll
        for (int j = 0; j < WALK_ITEMS; ++j) {
            if (k[j] != KEY_PAD) {
                run += k[j] & 1u;
                if ((k[j] >> 1) != (k[j + 1] >> 1)) {   // a group end; positions grow, so only a strictly better one replaces
                    const uint32_t cnt = i0 + j + 1;
                    if (cand_cmp<CRIT>(run, cnt, best_tp, best_cnt, P, N) > 0) {
                        best_tp = run;
                        best_cnt = cnt;
                    }
                }
            }
        }
        carry_tp += tile_total;
        __syncthreads();   // s_sum is rewritten by the next tile
    }
    r_tp[tid] = best_tp;
    r_cnt[tid] = best_cnt;
    __syncthreads();
    if (tid == 0) {
        uint32_t b_tp = r_tp[0], b_cnt = r_cnt[0];
        for (int q = 1; q < 256; ++q) {   // thread order: fixed; a tie goes to the earlier position
            const uint32_t c_tp = r_tp[q], c_cnt = r_cnt[q];
            const int c = cand_cmp<CRIT>(c_tp, c_cnt, b_tp, b_cnt, P, N);
            if (c > 0 || (c == 0 && c_cnt < b_cnt)) {
                b_tp = c_tp;
                b_cnt = c_cnt;
            }
        }
        const bool bad = invalid[blockIdx.x] != 0;
        float thr = __builtin_inff();
        if (b_cnt) thr = __uint_as_float(col[n - b_cnt] >> 1);   // the group's score, the very bits
        threshold[blockIdx.x] = bad ? fallback : thr;
        out_tp[blockIdx.x] = bad ? 0 : int(b_tp);
        out_fp[blockIdx.x] = bad ? 0 : int(b_cnt - b_tp);
        n_pos[blockIdx.x] = bad ? 0 : int(P);
        n_neg[blockIdx.x] = bad ? 0 : int(N);
        if (tuned) tuned[blockIdx.x] = bad ? 0 : 1;
    }
}

// ------------------------------------------------------------------ thresholded counts, one threshold per label
// One wave per row, 64 rows per wave, as the scalar kernel: the per-sample counts are ballots, the per-label counts collect in
// LDS and reach memory with one integer add per touched label and workgroup.
__global__ __launch_bounds__(256) void threshold_counts_vec_kernel(const float* __restrict__ probs, int64_t ldp,
                                                                   const float* __restrict__ targets, int64_t ldt, int64_t n,
                                                                   int L, const float* __restrict__ thresholds,
                                                                   int* __restrict__ lab_tp, int* __restrict__ lab_fp,
                                                                   int* __restrict__ lab_fn, int* __restrict__ ex_tp,
                                                                   int* __restrict__ ex_pred, int* __restrict__ ex_gold,
                                                                   int* __restrict__ ex_mis) {
    __shared__ int s_cnt[3][VEC_SLAB];
    __shared__ float s_thr[VEC_SLAB];
    const int tid = int(threadIdx.x), lane = lane_id(), w = tid >> 6;
    const int l_lo = int(blockIdx.y) * VEC_SLAB;
    const int l_hi = l_lo + VEC_SLAB < L ? l_lo + VEC_SLAB : L;
    for (int i = tid; i < 3 * VEC_SLAB; i += 256) (&s_cnt[0][0])[i] = 0;
    for (int i = tid; i < l_hi - l_lo; i += 256) s_thr[i] = thresholds[l_lo + i];
    __syncthreads();
    const int64_t row0 = int64_t(blockIdx.x) * 256 + w * 64;
    for (int rr = 0; rr < 64; ++rr) {
        const int64_t r = row0 + rr;
        if (r >= n) break;   // wave-uniform
        int c_tp = 0, c_pred = 0, c_gold = 0, c_mis = 0;
        for (int lb = l_lo; lb < l_hi; lb += 64) {
            const int l = lb + lane;
            bool pred = false, gold = false;
            if (l < l_hi) {
                const float p = probs[r * ldp + l];
                pred = (p != p ? 0.0f : p) >= s_thr[l - l_lo];   // a NaN threshold compares false: predicts nothing
                gold = targets[r * ldt + l] != 0.0f;
                if (pred | gold) atomicAdd(&s_cnt[pred ? (gold ? 0 : 1) : 2][l - l_lo], 1);
            }
            c_tp += __popcll(__ballot(pred && gold));
            c_pred += __popcll(__ballot(pred));
            c_gold += __popcll(__ballot(gold));
            c_mis += __popcll(__ballot(pred != gold));
        }
        if (lane == 0) {
            atomicAdd(&ex_tp[r], c_tp);
            atomicAdd(&ex_pred[r], c_pred);
            atomicAdd(&ex_gold[r], c_gold);
            atomicAdd(&ex_mis[r], c_mis);
        }
    }
    __syncthreads();
    for (int i = tid; i < l_hi - l_lo; i += 256) {
        if (s_cnt[0][i]) atomicAdd(&lab_tp[l_lo + i], s_cnt[0][i]);
        if (s_cnt[1][i]) atomicAdd(&lab_fp[l_lo + i], s_cnt[1][i]);
        if (s_cnt[2][i]) atomicAdd(&lab_fn[l_lo + i], s_cnt[2][i]);
    }
}

}  // namespace
}  // namespace lamp

using namespace lamp;

size_t lamp_tune_thresholds_workspace_bytes(int64_t n_rows, int32_t L) {
    if (int64_t(L) > int64_t(65535) * 64) return 0;   // the key build's grid
    return rank_sort_workspace_bytes(n_rows, L);
}

int lamp_tune_thresholds(const float* probs, int64_t ld_probs, const float* targets, int64_t ld_targets, int64_t n_rows, int32_t L,
                         int32_t criterion, float fallback, float* threshold, int32_t* tp, int32_t* fp, int32_t* n_pos,
                         int32_t* n_neg, int32_t* tuned, void* workspace, size_t workspace_bytes, lamp_stream_t stream) {
    if (n_rows <= 0 || L <= 0 || ld_probs < L || ld_targets < L) return LAMP_E_DIMS;
    if (!probs || !targets || !threshold || !tp || !fp || !n_pos || !n_neg || !workspace) return LAMP_E_NULL;
    if (criterion != LAMP_TUNE_F1 && criterion != LAMP_TUNE_YOUDEN && criterion != LAMP_TUNE_BALANCE) return LAMP_E_UNSUPPORTED;
    if (lamp_tune_thresholds_workspace_bytes(n_rows, L) == 0) return LAMP_E_UNSUPPORTED;
    RankSorted r;
    if (int e = rank_sort_columns(probs, ld_probs, targets, ld_targets, n_rows, L, workspace, workspace_bytes, stream, &r)) return e;
    hipStream_t s = hipStream_t(stream);
    auto* kern = criterion == LAMP_TUNE_F1       ? tune_walk_kernel<LAMP_TUNE_F1>
                 : criterion == LAMP_TUNE_YOUDEN ? tune_walk_kernel<LAMP_TUNE_YOUDEN>
                                                 : tune_walk_kernel<LAMP_TUNE_BALANCE>;
    hipLaunchKernelGGL(kern, dim3(unsigned(L)), dim3(256), 0, s, r.keys, n_rows, r.invalid, fallback, threshold, tp, fp, n_pos,
                       n_neg, tuned);
    return int(hipGetLastError());
}

int lamp_threshold_counts_vec(const float* probs, int64_t ld_probs, const float* targets, int64_t ld_targets, int64_t n_rows,
                              int32_t L, const float* thresholds, int32_t* label_tp, int32_t* label_fp, int32_t* label_fn,
                              int32_t* sample_tp, int32_t* sample_pred, int32_t* sample_gold, int32_t* sample_mismatch,
                              lamp_stream_t stream) {
    if (n_rows <= 0 || L <= 0 || ld_probs < L || ld_targets < L) return LAMP_E_DIMS;
    if (!probs || !targets || !thresholds || !label_tp || !label_fp || !label_fn || !sample_tp || !sample_pred || !sample_gold ||
        !sample_mismatch)
        return LAMP_E_NULL;
    const int64_t row_blocks = (n_rows + 255) / 256;
    const int slabs = (L + VEC_SLAB - 1) / VEC_SLAB;
    // the per-label counts are int32: a label of 2^31 rows could not hold its own count
    if (n_rows >= (int64_t(1) << 31) || slabs > 65535) return LAMP_E_UNSUPPORTED;
    hipStream_t s = hipStream_t(stream);
    for (int32_t* p : {label_tp, label_fp, label_fn})
        if (hipError_t e = hipMemsetAsync(p, 0, size_t(L) * sizeof(int32_t), s)) return int(e);
    for (int32_t* p : {sample_tp, sample_pred, sample_gold, sample_mismatch})
        if (hipError_t e = hipMemsetAsync(p, 0, size_t(n_rows) * sizeof(int32_t), s)) return int(e);
    hipLaunchKernelGGL(threshold_counts_vec_kernel, dim3(unsigned(row_blocks), unsigned(slabs)), dim3(256), 0, s, probs, ld_probs,
                       targets, ld_targets, n_rows, L, thresholds, label_tp, label_fp, label_fn, sample_tp, sample_pred,
                       sample_gold, sample_mismatch);
    return int(hipGetLastError());
}

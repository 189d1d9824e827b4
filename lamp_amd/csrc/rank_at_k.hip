// Ranking the labels of one sample (include/lamp_hip.h): the k best columns of every row of an [n, L]
// score matrix in a defined order, and precision / nDCG / recall at every rank 1..k from those columns and the targets.
//
//   order       element a at column i ranks before b at column j when a is a number and b is NaN, or both are numbers and
//               a > b, or neither decides and i < j.  order_key() maps the fp32 bits to a u32 that is larger for the element
//               that ranks first (+0 and -0 share a key, every NaN shares the lowest one); a tie is broken by the column.
//   top-k       a row lives in the registers of the threads that rank it: E scores per thread, 64 W threads per row, each
//               score loaded once (thread t holds columns t, t + 64 W, ...: coalesced).  Rank r is the maximum of
//               (key, ~column) over the row that is still in play: every thread keeps its own best, a butterfly gives the
//               wave's, W > 1 waves meet in LDS (one barrier per rank, two buffers); the owner of the winner retires it and
//               looks for its next best.  k such rounds leave the k columns in rank order; they are stored together at the end.
//               L <= 1024: a wave per row, four rows per workgroup.  L <= 4096: a workgroup of 4 waves per row.  Beyond: 16 waves.
//               E is the power of two that holds ceil(L / (64 W)).  The route is a function of L alone.
//   rank at k   a wave per sample writes its hit mask (bit r: the target at the rank-r column is nonzero) and its gold count;
//               one workgroup per 1024 samples turns them into per-rank partial sums, sample by sample; one workgroup adds
//               the partials chunk by chunk.  The order of every sum is fixed by n.
// No workspace for the top-k, no global atomics, nothing allocated or synchronised, inputs never written; all launches go to
// the caller's stream.
#include "lamp_kernels.h"

namespace lamp {
namespace {

constexpr int TOPK_MAX_K = 64;
constexpr int TOPK_MAX_L = 32768;
constexpr int RANK_CHUNK = 1024;   // samples whose terms one workgroup of the partial sums adds, in sample order

__device__ __forceinline__ uint32_t order_key(uint32_t bits) {
    const uint32_t mag = bits & 0x7FFFFFFFu;
    if (mag > 0x7F800000u) return 1u;             // NaN: below -inf (0x007FFFFF), above a retired or padding slot (0)
    if (mag == 0u) return 0x80000000u;            // +0.0 and -0.0 are tied
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

template <int E, int W>
__global__ __launch_bounds__(W == 1 ? 256 : 64 * W) void topk_labels_kernel(const float* __restrict__ scores, int64_t ld, int64_t n,
                                                                            int L, int k, int32_t* __restrict__ idx,
                                                                            int64_t ld_idx, float* __restrict__ val,
                                                                            int64_t ld_val) {
    constexpr int T = 64 * W;                 // threads that share a row
    constexpr int ROWS = W == 1 ? 4 : 1;      // rows of a workgroup
    __shared__ unsigned long long s_best[2][W];
    __shared__ int32_t s_idx[ROWS][TOPK_MAX_K];
    __shared__ uint32_t s_val[ROWS][TOPK_MAX_K];
    const int tid = int(threadIdx.x), lane = tid & 63, w = tid >> 6;
    const int slot = W == 1 ? w : 0;
    const int t = W == 1 ? lane : tid;        // this thread's place among the T of its row
    const int64_t row = int64_t(blockIdx.x) * ROWS + slot;
    const bool live = row < n;
    const float* src = scores + (live ? row : 0) * ld;
    uint32_t raw[E], key[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int col = e * T + t;
        const bool in = live && col < L;
        raw[e] = in ? __float_as_uint(src[col]) : 0u;
        key[e] = in ? order_key(raw[e]) : 0u;
    }
    uint32_t bk = 0, braw = 0;
    int be = 0;
#pragma unroll
    for (int e = 0; e < E; ++e)               // ascending columns and a strict compare: the lowest column of a tie
        if (key[e] > bk) {
            bk = key[e];
            be = e;
            braw = raw[e];
        }
    for (int r = 0; r < k; ++r) {
        unsigned long long p = (static_cast<unsigned long long>(bk) << 32) | uint32_t(~uint32_t(be * T + t));
        p = wave_max_u64(p);
        if (W > 1) {
            if (lane == 0) s_best[r & 1][w] = p;
            __syncthreads();   // the other buffer is written next round: nobody is still reading it (they passed this barrier)
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const unsigned long long u = s_best[r & 1][q];
                p = u > p ? u : p;
            }
        }
        const int wcol = int(~uint32_t(p));
        if ((wcol & (T - 1)) == t) {   // the owner: wcol = be * T + t (k <= L: a real element while the row is live)
            s_idx[slot][r] = wcol;
            s_val[slot][r] = braw;
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (e == be) key[e] = 0u;
            bk = 0;
            braw = 0;
            be = 0;
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (key[e] > bk) {
                    bk = key[e];
                    be = e;
                    braw = raw[e];
                }
        }
    }
    __syncthreads();
    if (live && t < k) {
        idx[row * ld_idx + t] = s_idx[slot][t];
        if (val) val[row * ld_val + t] = __uint_as_float(s_val[slot][t]);
    }
}

// ------------------------------------------------------------------ rank at k
struct RankTables {
    double d[TOPK_MAX_K];           // d[r] = 1 / log2(r + 2)
    double ideal[TOPK_MAX_K + 1];   // ideal[m] = d[0] + ... + d[m - 1]
};

__global__ __launch_bounds__(256) void rank_rows_kernel(const int32_t* __restrict__ idx, int64_t ld_idx,
                                                        const float* __restrict__ targets, int64_t ldt, int64_t n, int L, int k,
                                                        unsigned long long* __restrict__ hit_mask, int32_t* __restrict__ gold) {
    const int lane = int(threadIdx.x) & 63;
    const int64_t row = int64_t(blockIdx.x) * 4 + (int(threadIdx.x) >> 6);
    if (row >= n) return;   // wave-uniform; no barrier below
    const float* t = targets + row * ldt;
    int g = 0;
    for (int l0 = 0; l0 < L; l0 += 64) {
        const int l = l0 + lane;
        const bool nz = l < L && t[l] != 0.0f;
        g += __popcll(__ballot(nz));
    }
    bool hit = false;
    if (lane < k) {
        const int c = idx[row * ld_idx + lane];
        hit = c >= 0 && c < L && t[c] != 0.0f;
    }
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) {
        hit_mask[row] = mask;
        gold[row] = g;
    }
}

// thread j adds the terms of rank j + 1 over the samples of one chunk, in sample order
__global__ __launch_bounds__(64) void rank_chunk_kernel(const unsigned long long* __restrict__ hit_mask,
                                                        const int32_t* __restrict__ gold, int64_t n, int k, RankTables tab,
                                                        double* __restrict__ part_ndcg, double* __restrict__ part_recall,
                                                        int64_t* __restrict__ part_hits, int64_t* __restrict__ part_gold) {
    __shared__ double s_d[TOPK_MAX_K];
    const int j = int(threadIdx.x);
    s_d[j] = tab.d[j];
    __syncthreads();
    if (j >= k) return;
    const int64_t i0 = int64_t(blockIdx.x) * RANK_CHUNK;
    const int64_t i1 = i0 + RANK_CHUNK < n ? i0 + RANK_CHUNK : n;
    const unsigned long long upto = j >= 63 ? ~0ull : ((1ull << (j + 1)) - 1ull);
    double ndcg = 0.0, recall = 0.0;
    int64_t hits = 0, with_gold = 0;
    for (int64_t i = i0; i < i1; ++i) {
        const unsigned long long m = hit_mask[i];
        const int g = gold[i];
        hits += int64_t((m >> j) & 1ull);
        if (g > 0) {
            ++with_gold;
            unsigned long long mm = m & upto;
            const int c = __popcll(mm);
            double dcg = 0.0;
            while (mm) {   // ascending ranks
                dcg += s_d[__ffsll(mm) - 1];
                mm &= mm - 1ull;
            }
            ndcg += dcg / tab.ideal[j + 1 < g ? j + 1 : g];
            recall += double(c) / double(g);
        }
    }
    const int64_t o = int64_t(blockIdx.x) * k + j;
    part_ndcg[o] = ndcg;
    part_recall[o] = recall;
    part_hits[o] = hits;
    if (j == 0) part_gold[blockIdx.x] = with_gold;
}

__global__ __launch_bounds__(64) void rank_final_kernel(const double* __restrict__ part_ndcg, const double* __restrict__ part_recall,
                                                        const int64_t* __restrict__ part_hits,
                                                        const int64_t* __restrict__ part_gold, int64_t chunks, int k,
                                                        int64_t* __restrict__ hits_at_rank, double* __restrict__ ndcg_sum,
                                                        double* __restrict__ recall_sum, int64_t* __restrict__ n_with_gold) {
    const int j = int(threadIdx.x);
    if (j >= k) return;
    double ndcg = 0.0, recall = 0.0;
    int64_t hits = 0, with_gold = 0;
    for (int64_t c = 0; c < chunks; ++c) {   // chunk order: fixed
        ndcg += part_ndcg[c * k + j];
        recall += part_recall[c * k + j];
        hits += part_hits[c * k + j];
        if (j == 0) with_gold += part_gold[c];
    }
    hits_at_rank[j] = hits;
    ndcg_sum[j] = ndcg;
    recall_sum[j] = recall;
    if (j == 0) *n_with_gold = with_gold;
}

// ------------------------------------------------------------------ host side
inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct RankAtKLayout {
    size_t mask, gold, part_ndcg, part_recall, part_hits, part_gold, total;   // byte offsets
    int64_t chunks;
};

bool rank_at_k_layout(int64_t n, int32_t k, RankAtKLayout* out) {
    if (n <= 0 || k <= 0 || k > TOPK_MAX_K || n >= (int64_t(1) << 31)) return false;
    RankAtKLayout g{};
    g.chunks = (n + RANK_CHUNK - 1) / RANK_CHUNK;
    const size_t part = up256(size_t(g.chunks) * size_t(k) * 8);
    size_t off = 0;
    g.mask = off; off += up256(size_t(n) * 8);
    g.gold = off; off += up256(size_t(n) * 4);
    g.part_ndcg = off; off += part;
    g.part_recall = off; off += part;
    g.part_hits = off; off += part;
    g.part_gold = off; off += up256(size_t(g.chunks) * 8);
    g.total = off + 256;   // the caller's base may be anywhere: one alignment allowance
    *out = g;
    return true;
}

template <int E, int W>
void launch_topk(const float* scores, int64_t ld, int64_t n, int L, int k, int32_t* idx, int64_t ld_idx, float* val,
                 int64_t ld_val, hipStream_t s) {
    const unsigned blocks = W == 1 ? unsigned((n + 3) / 4) : unsigned(n);
    hipLaunchKernelGGL((topk_labels_kernel<E, W>), dim3(blocks), dim3(W == 1 ? 256 : 64 * W), 0, s, scores, ld, n, L, k, idx,
                       ld_idx, val, ld_val);
}

}  // namespace
}  // namespace lamp

using namespace lamp;

int lamp_topk_labels(const float* scores, int64_t ld, int64_t n_rows, int32_t L, int32_t k, int32_t* idx, int64_t ld_idx,
                     float* val, int64_t ld_val, lamp_stream_t stream) {
    if (n_rows <= 0 || L <= 0 || k <= 0 || ld < L || k > L || ld_idx < k || (val && ld_val < k)) return LAMP_E_DIMS;
    if (!scores || !idx) return LAMP_E_NULL;
    if (k > TOPK_MAX_K || L > TOPK_MAX_L || n_rows >= (int64_t(1) << 31)) return LAMP_E_UNSUPPORTED;
    hipStream_t s = hipStream_t(stream);
#define LAMP_TOPK(E, W) launch_topk<E, W>(scores, ld, n_rows, L, k, idx, ld_idx, val, ld_val, s)
    if (L <= 64) LAMP_TOPK(1, 1);
    else if (L <= 128) LAMP_TOPK(2, 1);
    else if (L <= 256) LAMP_TOPK(4, 1);
    else if (L <= 512) LAMP_TOPK(8, 1);
    else if (L <= 1024) LAMP_TOPK(16, 1);
    else if (L <= 2048) LAMP_TOPK(8, 4);
    else if (L <= 4096) LAMP_TOPK(16, 4);
    else if (L <= 8192) LAMP_TOPK(8, 16);
    else if (L <= 16384) LAMP_TOPK(16, 16);
    else LAMP_TOPK(32, 16);
#undef LAMP_TOPK
    return int(hipGetLastError());
}

size_t lamp_rank_at_k_workspace_bytes(int64_t n_rows, int32_t k) {
    RankAtKLayout g;
    return rank_at_k_layout(n_rows, k, &g) ? g.total : 0;
}

int lamp_rank_at_k(const int32_t* idx, int64_t ld_idx, const float* targets, int64_t ld_targets, int64_t n_rows, int32_t L,
                   int32_t k, const double* discount, const double* ideal, int64_t* hits_at_rank, double* ndcg_sum,
                   double* recall_sum, int64_t* n_with_gold, void* workspace, size_t workspace_bytes, lamp_stream_t stream) {
    if (n_rows <= 0 || L <= 0 || k <= 0 || ld_targets < L || k > L || ld_idx < k) return LAMP_E_DIMS;
    if (!idx || !targets || !discount || !ideal || !hits_at_rank || !ndcg_sum || !recall_sum || !n_with_gold || !workspace)
        return LAMP_E_NULL;
    if (k > TOPK_MAX_K || L > TOPK_MAX_L || n_rows >= (int64_t(1) << 31)) return LAMP_E_UNSUPPORTED;
    RankAtKLayout g;
    if (!rank_at_k_layout(n_rows, k, &g)) return LAMP_E_UNSUPPORTED;
    if (workspace_bytes < g.total) return LAMP_E_WORKSPACE;   // (g.total holds the 255 bytes `base` may move)
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
    RankTables tab{};
    for (int r = 0; r < k; ++r) tab.d[r] = discount[r];
    for (int r = 0; r <= k; ++r) tab.ideal[r] = ideal[r];
    hipStream_t s = hipStream_t(stream);
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(base + g.mask);
    int32_t* gold = reinterpret_cast<int32_t*>(base + g.gold);
    double* part_ndcg = reinterpret_cast<double*>(base + g.part_ndcg);
    double* part_recall = reinterpret_cast<double*>(base + g.part_recall);
    int64_t* part_hits = reinterpret_cast<int64_t*>(base + g.part_hits);
    int64_t* part_gold = reinterpret_cast<int64_t*>(base + g.part_gold);
    hipLaunchKernelGGL(rank_rows_kernel, dim3(unsigned((n_rows + 3) / 4)), dim3(256), 0, s, idx, ld_idx, targets, ld_targets,
                       n_rows, L, k, mask, gold);
    hipLaunchKernelGGL(rank_chunk_kernel, dim3(unsigned(g.chunks)), dim3(64), 0, s, mask, gold, n_rows, k, tab, part_ndcg,
                       part_recall, part_hits, part_gold);
    hipLaunchKernelGGL(rank_final_kernel, dim3(1), dim3(64), 0, s, part_ndcg, part_recall, part_hits, part_gold, g.chunks, k,
                       hits_at_rank, ndcg_sum, recall_sum, n_with_gold);
    return int(hipGetLastError());
}

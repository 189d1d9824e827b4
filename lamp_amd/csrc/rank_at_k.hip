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
//   label ranking   every gold label's rank among all L labels of its row, for LRAP, coverage error, ranking loss, one-error and
//               the per-sample AUC: described where it starts, below the rank-at-k kernels.
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

// ------------------------------------------------------------------ label ranking (whole-row metrics)
// For every gold label p of a row (target != 0): rank_p = #{j : key_j >= key_p} and pos_p = #{gold j : key_j >= key_p}, keys
// as order_key() makes them and compared as integers (a tie counts against p; p counts itself).  From them the row's six
// integers (n_pos, coverage = max rank_p, misordered = sum (rank_p - pos_p), tied = gold / non-gold pairs of equal key,
// top1_hit, has_nan) and lrap = (sum_p pos_p / rank_p) / n_pos in fp64 (include/lamp_hip.h has the definitions).
//   L <= 1024   a wave per row, four rows per workgroup, the row in registers as the top-k keeps it.  The gold keys are
//               compacted into LDS in column order; for every gold label the wave ballots key_j >= key_p over 64 columns at
//               a time and popcounts the mask and its AND with the chunk's gold mask: all lanes work whatever n_pos is.
//   beyond      a workgroup of 4 (L <= 4096) or 16 waves per row.  The row's keys are PARTITIONED in LDS: the gold keys in
//               column order from the front, the others behind them (their order does not matter to a count).  Thread t
//               takes the gold labels t, t + T, ... and walks the L keys with broadcast 128-bit LDS reads: the front part
//               gives pos_p, the rest the non-gold keys at or above / equal to key_p.
// The quotients pos_p / rank_p are added per thread in ascending p (p = t, t + T, ...), then over the threads by a fixed
// butterfly and over the waves in wave order: the order is a function of the row (its L and its gold columns) alone.
// top1_hit is the gold bit of the maximum of (key, lowest column) over the row, i.e. of rank 1 of lamp_topk_labels.
constexpr int LRANK_INTS = 6;    // per row: n_pos, coverage, misordered, tied, top1_hit, has_nan
constexpr int LRANK_TERMS = 3;   // per row: lrap, rloss, auc (0 for a row without both classes)
constexpr int LRANK_SUMS = 8;    // 3 fp64 sums, then 5 int64 counts

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);   // a + b == b + a: every lane ends with the same bits
    return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// (key, lowest column first, gold bit): the maximum over a row is its first-ranked element; a padding slot (key 0) never wins
__device__ __forceinline__ unsigned long long first_rank_word(uint32_t key, int col, bool gold) {
    return (static_cast<unsigned long long>(key) << 32) | (uint32_t(TOPK_MAX_L - 1 - col) << 1) | uint32_t(gold);
}

__device__ __forceinline__ void label_rank_store(int64_t row, int L, int n_p, int coverage, int misordered, int tied, int top1,
                                                 int has_nan, double quot_sum, int32_t* __restrict__ ws_ints,
                                                 double* __restrict__ ws_terms, int32_t* __restrict__ row_counts,
                                                 double* __restrict__ row_lrap) {
    const int pairs = n_p * (L - n_p);   // <= 2^28
    const double lrap = n_p ? quot_sum / double(n_p) : 1.0;
    const double rloss = pairs ? double(misordered) / double(pairs) : 0.0;
    const double auc = pairs ? 1.0 - (double(misordered) - 0.5 * double(tied)) / double(pairs) : 0.0;
    const int v[LRANK_INTS] = {n_p, coverage, misordered, tied, top1, has_nan};
#pragma unroll
    for (int i = 0; i < LRANK_INTS; ++i) {
        ws_ints[row * LRANK_INTS + i] = v[i];
        if (row_counts) row_counts[row * LRANK_INTS + i] = v[i];
    }
    ws_terms[row * LRANK_TERMS + 0] = lrap;
    ws_terms[row * LRANK_TERMS + 1] = rloss;
    ws_terms[row * LRANK_TERMS + 2] = auc;
    if (row_lrap) row_lrap[row] = lrap;
}

template <int E>
__global__ __launch_bounds__(256) void label_rank_wave_kernel(const float* __restrict__ scores, int64_t lds,
                                                              const float* __restrict__ targets, int64_t ldt, int64_t n, int L,
                                                              int32_t* __restrict__ ws_ints, double* __restrict__ ws_terms,
                                                              int32_t* __restrict__ row_counts, double* __restrict__ row_lrap) {
    __shared__ uint32_t s_pos[4][64 * E];     // the gold keys in column order; then (rank << 16) | pos of each
    const int lane = int(threadIdx.x) & 63, slot = int(threadIdx.x) >> 6;
    const int64_t row = int64_t(blockIdx.x) * 4 + slot;
    const bool live = row < n;                // a dead wave goes through with n_p = 0: the barriers below are the workgroup's
    const float* src = scores + (live ? row : 0) * lds;
    const float* tgt = targets + (live ? row : 0) * ldt;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t key[E];
    unsigned long long gmask[E];
    unsigned long long best = 0;
    bool nan = false;
    int n_p = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int col = e * 64 + lane;
        const bool in = live && col < L;
        key[e] = in ? order_key(__float_as_uint(src[col])) : 0u;
        const bool g = in && tgt[col] != 0.0f;
        gmask[e] = __ballot(g);
        if (g) s_pos[slot][n_p + __popcll(gmask[e] & below)] = key[e];
        n_p += __popcll(gmask[e]);
        const unsigned long long v = first_rank_word(key[e], col, g);
        best = v > best ? v : best;
        nan = nan || key[e] == 1u;
    }
    best = wave_max_u64(best);
    const int has_nan = __ballot(nan) != 0ull;
    __syncthreads();
    int coverage = 0, misordered = 0, tied = 0;
    for (int p = 0; p < n_p; ++p) {           // wave-uniform: every lane holds the same counts
        const uint32_t kp = s_pos[slot][p];   // >= 1: a padding slot (0) is never at or above it
        int rank = 0, pos = 0, tie = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const unsigned long long ge = __ballot(key[e] >= kp), eq = __ballot(key[e] == kp);
            rank += __popcll(ge);
            pos += __popcll(ge & gmask[e]);
            tie += __popcll(eq & ~gmask[e]);
        }
        coverage = rank > coverage ? rank : coverage;
        misordered += rank - pos;
        tied += tie;
        if (lane == 0) s_pos[slot][p] = (uint32_t(rank) << 16) | uint32_t(pos);   // rank, pos <= 1024
    }
    __syncthreads();
    double quot = 0.0;
    for (int p = lane; p < n_p; p += 64) {
        const uint32_t v = s_pos[slot][p];
        quot += double(v & 0xFFFFu) / double(v >> 16);
    }
    quot = wave_sum_f64(quot);
    if (live && lane == 0)
        label_rank_store(row, L, n_p, coverage, misordered, tied, int(best & 1ull), has_nan, quot, ws_ints, ws_terms, row_counts,
                         row_lrap);
}

// keys [a, b) of the partitioned row against kp: how many are at or above it, and (EQ) how many equal it.  a, b and the
// addresses are the same for every thread: the LDS reads are broadcasts, 128 bits at a time between the ragged ends.
// (Serving four gold labels of a thread from every read was measured, one run each, and gained nothing -- 11.9 against 11.7 ms at
// 32 x 32768, half gold: the walk is bound by its compare-and-add instructions, not by LDS -- so a thread takes one at a time.)
template <bool EQ>
__device__ __forceinline__ void label_rank_count(const uint32_t* s_key, int a, int b, uint32_t kp, int& ge, int& eq) {
    int j = a;
#pragma nounroll
    for (; j < b && (j & 3); ++j) {
        const uint32_t k = s_key[j];
        ge += k >= kp;
        if (EQ) eq += k == kp;
    }
#pragma unroll 4
    for (; j + 4 <= b; j += 4) {
        const uint4 k = *reinterpret_cast<const uint4*>(s_key + j);
        ge += (k.x >= kp) + (k.y >= kp) + (k.z >= kp) + (k.w >= kp);
        if (EQ) eq += (k.x == kp) + (k.y == kp) + (k.z == kp) + (k.w == kp);
    }
#pragma nounroll
    for (; j < b; ++j) {
        const uint32_t k = s_key[j];
        ge += k >= kp;
        if (EQ) eq += k == kp;
    }
}

template <int E, int W>
__global__ __launch_bounds__(64 * W) void label_rank_block_kernel(const float* __restrict__ scores, int64_t lds,
                                                                  const float* __restrict__ targets, int64_t ldt, int L,
                                                                  int32_t* __restrict__ ws_ints, double* __restrict__ ws_terms,
                                                                  int32_t* __restrict__ row_counts,
                                                                  double* __restrict__ row_lrap) {
    constexpr int T = 64 * W;
    __shared__ __attribute__((aligned(16))) uint32_t s_key[T * E];   // gold keys in column order, then the others
    __shared__ int s_cnt[E * W];              // gold labels of (chunk e, wave w); then their exclusive prefix in column order
    __shared__ unsigned long long s_best[W];
    __shared__ double s_quot[W];
    __shared__ int s_int[4][W];               // has_nan, coverage, misordered, tied of every wave
    __shared__ int s_np;
    const int tid = int(threadIdx.x), lane = tid & 63, w = tid >> 6;
    const int64_t row = int64_t(blockIdx.x);  // the grid is n_rows: every workgroup has a row
    const float* src = scores + row * lds;
    const float* tgt = targets + row * ldt;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t key[E];
    uint32_t gbits = 0;                       // bit e: this thread's column of chunk e is gold
    unsigned long long best = 0;
    bool nan = false;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int col = e * T + tid;
        const bool in = col < L;
        key[e] = in ? order_key(__float_as_uint(src[col])) : 0u;
        const bool g = in && tgt[col] != 0.0f;
        const unsigned long long gm = __ballot(g);
        if (lane == 0) s_cnt[e * W + w] = __popcll(gm);
        gbits |= uint32_t(g) << e;
        const unsigned long long v = first_rank_word(key[e], col, g);
        best = v > best ? v : best;
        nan = nan || key[e] == 1u;
    }
    best = wave_max_u64(best);
    const int wave_nan = __ballot(nan) != 0ull;
    if (lane == 0) {
        s_best[w] = best;
        s_int[0][w] = wave_nan;
    }
    __syncthreads();
    if (w == 0) {                             // exclusive prefix of the E W counts, 64 at a time
        int carry = 0;
        for (int i = 0; i < E * W; i += 64) {
            const int at = i + lane;
            const int c = at < E * W ? s_cnt[at] : 0;
            int x = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(x, o, 64);
                if (lane >= o) x += y;
            }
            if (at < E * W) s_cnt[at] = carry + x - c;
            carry += __shfl(x, 63, 64);
        }
        if (lane == 0) s_np = carry;
    }
    __syncthreads();
    const int n_p = s_np;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int col = e * T + tid;
        const bool g = (gbits >> e) & 1u;
        const unsigned long long gm = __ballot(g);
        const int before = s_cnt[e * W + w] + __popcll(gm & below);   // gold labels at lower columns
        if (col < L) s_key[g ? before : n_p + (col - before)] = key[e];
    }
    __syncthreads();
    int coverage = 0, misordered = 0, tied = 0;
    double quot = 0.0;
    for (int p = tid; p < n_p; p += T) {
        const uint32_t kp = s_key[p];
        int pos = 0, above = 0, tie = 0, unused = 0;
        label_rank_count<false>(s_key, 0, n_p, kp, pos, unused);
        label_rank_count<true>(s_key, n_p, L, kp, above, tie);
        const int rank = pos + above;
        quot += double(pos) / double(rank);
        coverage = rank > coverage ? rank : coverage;
        misordered += above;
        tied += tie;
    }
    quot = wave_sum_f64(quot);
    coverage = wave_max_i32(coverage);
    misordered = wave_sum_i32(misordered);
    tied = wave_sum_i32(tied);
    if (lane == 0) {
        s_quot[w] = quot;
        s_int[1][w] = coverage;
        s_int[2][w] = misordered;
        s_int[3][w] = tied;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long b = 0;
        int has_nan = 0;
        quot = 0.0;
        coverage = misordered = tied = 0;
#pragma nounroll
        for (int q = 0; q < W; ++q) {         // wave order: fixed
            b = s_best[q] > b ? s_best[q] : b;
            has_nan |= s_int[0][q];
            quot += s_quot[q];
            coverage = s_int[1][q] > coverage ? s_int[1][q] : coverage;
            misordered += s_int[2][q];
            tied += s_int[3][q];
        }
        label_rank_store(row, L, n_p, coverage, misordered, tied, int(b & 1ull), has_nan, quot, ws_ints, ws_terms, row_counts,
                         row_lrap);
    }
}

// The row terms of one chunk, added in row order: 256 rows at a time are staged in LDS by the whole workgroup (coalesced
// loads; a thread adding straight from global memory would wait out one memory latency per row), then thread j adds quantity j
// (0 .. 2 the fp64 terms, 3 .. 7 the integer counts) over them.  The order is the rows' own.
constexpr int LRANK_TILE = 256;

__global__ __launch_bounds__(LRANK_TILE) void label_rank_chunk_kernel(const int32_t* __restrict__ ws_ints,
                                                                      const double* __restrict__ ws_terms, int64_t n, int L,
                                                                      double* __restrict__ part) {
    __shared__ double s_term[LRANK_TILE][LRANK_TERMS];
    __shared__ int32_t s_count[LRANK_TILE][LRANK_SUMS - LRANK_TERMS];
    const int t = int(threadIdx.x);
    const int64_t i0 = int64_t(blockIdx.x) * RANK_CHUNK;
    const int64_t i1 = i0 + RANK_CHUNK < n ? i0 + RANK_CHUNK : n;
    double sum = 0.0;
    int64_t count = 0;
    for (int64_t base = i0; base < i1; base += LRANK_TILE) {
        const int64_t i = base + t;
        if (i < i1) {
            const int32_t* r = ws_ints + i * LRANK_INTS;
            const int n_p = r[0];
            s_count[t][0] = r[1];
            s_count[t][1] = r[4];
            s_count[t][2] = n_p > 0;
            s_count[t][3] = n_p > 0 && n_p < L;
            s_count[t][4] = r[5];
#pragma unroll
            for (int q = 0; q < LRANK_TERMS; ++q) s_term[t][q] = ws_terms[i * LRANK_TERMS + q];
        }
        __syncthreads();
        const int rows = int(i1 - base < LRANK_TILE ? i1 - base : LRANK_TILE);
        if (t < LRANK_TERMS)
            for (int r = 0; r < rows; ++r) sum += s_term[r][t];
        else if (t < LRANK_SUMS)
            for (int r = 0; r < rows; ++r) count += s_count[r][t - LRANK_TERMS];
        __syncthreads();
    }
    if (t < LRANK_TERMS) part[int64_t(blockIdx.x) * LRANK_SUMS + t] = sum;
    else if (t < LRANK_SUMS) reinterpret_cast<int64_t*>(part)[int64_t(blockIdx.x) * LRANK_SUMS + t] = count;
}

// the chunks' partial sums, added in chunk order, staged the same way
__global__ __launch_bounds__(LRANK_TILE) void label_rank_final_kernel(const double* __restrict__ part, int64_t chunks,
                                                                      double* __restrict__ sums, int64_t* __restrict__ counts) {
    __shared__ double s_part[LRANK_TILE][LRANK_SUMS];
    const int t = int(threadIdx.x);
    double sum = 0.0;
    int64_t count = 0;
    for (int64_t base = 0; base < chunks; base += LRANK_TILE) {
        const int tile = int(chunks - base < LRANK_TILE ? chunks - base : LRANK_TILE);
        for (int e = t; e < tile * LRANK_SUMS; e += LRANK_TILE) s_part[e / LRANK_SUMS][e % LRANK_SUMS] = part[base * LRANK_SUMS + e];
        __syncthreads();
        if (t < LRANK_TERMS)
            for (int c = 0; c < tile; ++c) sum += s_part[c][t];
        else if (t < LRANK_SUMS)
            for (int c = 0; c < tile; ++c) count += reinterpret_cast<const int64_t*>(&s_part[c][0])[t];
        __syncthreads();
    }
    if (t < LRANK_TERMS) sums[t] = sum;
    else if (t < LRANK_SUMS) counts[t - LRANK_TERMS] = count;
}

// ------------------------------------------------------------------ host side
inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct LabelRankLayout {
    size_t ints, terms, part, total;   // byte offsets
    int64_t chunks;
};

bool label_rank_layout(int64_t n, int32_t L, LabelRankLayout* out) {
    if (n <= 0 || L <= 0 || L > TOPK_MAX_L || n >= (int64_t(1) << 31)) return false;
    LabelRankLayout g{};
    g.chunks = (n + RANK_CHUNK - 1) / RANK_CHUNK;
    size_t off = 0;
    g.terms = off; off += up256(size_t(n) * LRANK_TERMS * 8);
    g.ints = off; off += up256(size_t(n) * LRANK_INTS * 4);
    g.part = off; off += up256(size_t(g.chunks) * LRANK_SUMS * 8);
    g.total = off + 256;   // the caller's base may be anywhere: one alignment allowance
    *out = g;
    return true;
}

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

size_t lamp_label_ranking_workspace_bytes(int64_t n_rows, int32_t L) {
    LabelRankLayout g;
    return label_rank_layout(n_rows, L, &g) ? g.total : 0;
}

int lamp_label_ranking(const float* scores, int64_t ld_scores, const float* targets, int64_t ld_targets, int64_t n_rows,
                       int32_t L, double* sums, int64_t* counts, int32_t* row_counts, double* row_lrap, void* workspace,
                       size_t workspace_bytes, lamp_stream_t stream) {
    if (n_rows <= 0 || L <= 0 || ld_scores < L || ld_targets < L) return LAMP_E_DIMS;
    if (!scores || !targets || !sums || !counts || !workspace) return LAMP_E_NULL;
    if (L > TOPK_MAX_L || n_rows >= (int64_t(1) << 31)) return LAMP_E_UNSUPPORTED;
    LabelRankLayout g;
    if (!label_rank_layout(n_rows, L, &g)) return LAMP_E_UNSUPPORTED;
    if (workspace_bytes < g.total) return LAMP_E_WORKSPACE;   // (g.total holds the 255 bytes `base` may move)
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
    hipStream_t s = hipStream_t(stream);
    int32_t* ws_ints = reinterpret_cast<int32_t*>(base + g.ints);
    double* ws_terms = reinterpret_cast<double*>(base + g.terms);
    double* part = reinterpret_cast<double*>(base + g.part);
#define LAMP_LRANK_WAVE(E)                                                                                                    \
    hipLaunchKernelGGL((label_rank_wave_kernel<E>), dim3(unsigned((n_rows + 3) / 4)), dim3(256), 0, s, scores, ld_scores,    \
                       targets, ld_targets, n_rows, L, ws_ints, ws_terms, row_counts, row_lrap)
#define LAMP_LRANK_BLOCK(E, W)                                                                                                \
    hipLaunchKernelGGL((label_rank_block_kernel<E, W>), dim3(unsigned(n_rows)), dim3(64 * W), 0, s, scores, ld_scores,       \
                       targets, ld_targets, L, ws_ints, ws_terms, row_counts, row_lrap)
    if (L <= 64) LAMP_LRANK_WAVE(1);
    else if (L <= 128) LAMP_LRANK_WAVE(2);
    else if (L <= 256) LAMP_LRANK_WAVE(4);
    else if (L <= 512) LAMP_LRANK_WAVE(8);
    else if (L <= 1024) LAMP_LRANK_WAVE(16);
    else if (L <= 2048) LAMP_LRANK_BLOCK(8, 4);
    else if (L <= 4096) LAMP_LRANK_BLOCK(16, 4);
    else if (L <= 8192) LAMP_LRANK_BLOCK(8, 16);
    else if (L <= 16384) LAMP_LRANK_BLOCK(16, 16);
    else LAMP_LRANK_BLOCK(32, 16);
#undef LAMP_LRANK_WAVE
#undef LAMP_LRANK_BLOCK
    hipLaunchKernelGGL(label_rank_chunk_kernel, dim3(unsigned(g.chunks)), dim3(LRANK_TILE), 0, s, ws_ints, ws_terms, n_rows, L, part);
    hipLaunchKernelGGL(label_rank_final_kernel, dim3(1), dim3(LRANK_TILE), 0, s, part, g.chunks, sums, counts);
    return int(hipGetLastError());
}

// The evaluation's metrics on the device (reference: utils/evals.py:208-243,283-298,316-407): per-label AUC, AUPR and recall
// at an FDR cutoff from ONE key-only sort per label column, and the integer counts behind the five thresholded figures.
//
//   key build   [n, L] row-major scores + targets -> label-major u32 keys through an LDS tile (both sides coalesced).  A score
//               in [0, 1] has an fp32 bit pattern <= 0x3F800000 that orders like an unsigned integer, so
//               key = (bits(p) << 1) | t carries the target with it: the sort needs no payload, a tie group is key >> 1, and
//               the "this column cannot be ranked" flag (NaN / out-of-range score, target other than 0 / 1) falls out of the
//               same pass.
//   sort        ascending, one segment per label.  n <= SORT_LDS_MAX: one workgroup per label, bitonic, entirely in LDS.
//               Beyond: LSD radix sort through global memory, 8-bit digits, 4 passes, ping-pong buffers; per pass a histogram
//               per (label, chunk), an exclusive scan per label in (digit, chunk) order, a stable scatter.  The route and the
//               chunking are functions of n alone.
//   curve walk  one workgroup per label streams the sorted column once from its high end (score descending): group ends,
//               tp by a scan with a carry between tiles, the previous group's end by a max-scan (positions and tp both grow),
//               then the u64 AUC numerator, the fp64 AUPR sum and the FDR candidate.
// The sorted column is a function of the column's multiset, and every sum here runs in an order fixed by n: results are
// bit-identical from run to run and under any permutation of the rows.  Nothing here allocates, synchronises or writes its
// inputs; all of it is enqueued on the caller's stream.
#include "lamp_kernels.h"

namespace lamp {
namespace {

constexpr int SORT_LDS_MAX = 32768;      // keys of one column the LDS route holds (128 KiB of the CU's 160)
constexpr int SORT_LDS_THREADS = 1024;
constexpr int RADIX_CHUNK = 4096;        // keys per (label, chunk) workgroup of the global route: 16 rounds of 256
constexpr int RADIX_ROUNDS = RADIX_CHUNK / 256;
constexpr int WALK_ITEMS = 4;            // consecutive keys per thread and tile of the curve walk
constexpr int WALK_TILE = 256 * WALK_ITEMS;
constexpr uint32_t KEY_PAD = 0xFFFFFFFFu;   // above every key (keys are <= 0x7F000001); its group id equals no real one
constexpr int COUNT_SLAB = 4096;         // labels whose counters one workgroup of the thresholded counts keeps in LDS

__device__ __forceinline__ int lane_id() { return int(threadIdx.x) & 63; }

// ------------------------------------------------------------------ key build + transpose
__global__ __launch_bounds__(256) void metric_keys_kernel(const float* __restrict__ probs, int64_t ldp,
                                                          const float* __restrict__ targets, int64_t ldt, int64_t n, int L,
                                                          uint32_t* __restrict__ keys, uint32_t* __restrict__ invalid) {
    __shared__ uint32_t tile[64][65];
    const int tx = int(threadIdx.x) & 63, ty = int(threadIdx.x) >> 6;
    const int64_t r0 = int64_t(blockIdx.x) * 64;
    const int l0 = int(blockIdx.y) * 64;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int64_t r = r0 + ty + 4 * k;
        const int l = l0 + tx;
        uint32_t key = 0;
        if (r < n && l < L) {
            const float p = probs[r * ldp + l] + 0.0f;   // -0.0 -> +0.0: the bit pattern must order like the value
            const float t = targets[r * ldt + l];
            const bool ok = p >= 0.0f && p <= 1.0f && (t == 0.0f || t == 1.0f);
            key = ok ? ((__float_as_uint(p) << 1) | (t == 1.0f ? 1u : 0u)) : 0u;
            bad |= !ok;
        }
        tile[ty + 4 * k][tx] = key;
    }
    if (bad) atomicOr(&invalid[l0 + tx], 1u);   // (bad implies l0 + tx < L)
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int l = l0 + ty + 4 * k;
        const int64_t r = r0 + tx;
        if (l < L && r < n) keys[int64_t(l) * n + r] = tile[tx][ty + 4 * k];
    }
}

// ------------------------------------------------------------------ sort, LDS route
__global__ __launch_bounds__(SORT_LDS_THREADS) void sort_lds_kernel(uint32_t* __restrict__ keys, int64_t n, int npow2) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_keys[];
    uint32_t* col = keys + int64_t(blockIdx.x) * n;
    const int tid = int(threadIdx.x);
    for (int i = tid; i < npow2; i += SORT_LDS_THREADS) s_keys[i] = i < n ? col[i] : KEY_PAD;
    __syncthreads();
    for (int k = 2; k <= npow2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (npow2 >> 1); t += SORT_LDS_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // t with a zero inserted at bit j
                const int p = i | j;
                const uint32_t a = s_keys[i], b = s_keys[p];
                if ((a > b) == ((i & k) == 0)) {
                    s_keys[i] = b;
                    s_keys[p] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < n; i += SORT_LDS_THREADS) col[i] = s_keys[i];   // the pads sorted to the end
}

// ------------------------------------------------------------------ sort, global route
// hist[(label * 256 + digit) * chunks + chunk]: digit-major, so that the exclusive scan in storage order gives every
// (digit, chunk) its first output slot of a stable pass.
__global__ __launch_bounds__(256) void radix_hist_kernel(const uint32_t* __restrict__ in, int64_t n, int chunks, int shift,
                                                         uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    const int tid = int(threadIdx.x);
    const int label = int(blockIdx.x) / chunks, chunk = int(blockIdx.x) % chunks;
    const uint32_t* col = in + int64_t(label) * n;
    h[tid] = 0;
    __syncthreads();
    const int64_t base = int64_t(chunk) * RADIX_CHUNK;
#pragma unroll 4
    for (int r = 0; r < RADIX_ROUNDS; ++r) {
        const int64_t i = base + r * 256 + tid;
        if (i < n) atomicAdd(&h[(col[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(int64_t(label) * 256 + tid) * chunks + chunk] = h[tid];
}

__global__ __launch_bounds__(256) void radix_scan_kernel(uint32_t* __restrict__ hist, int chunks) {
    __shared__ uint32_t tot[256];
    const int tid = int(threadIdx.x);
    uint32_t* h = hist + (int64_t(blockIdx.x) * 256 + tid) * chunks;
    uint32_t sum = 0;
    for (int c = 0; c < chunks; ++c) sum += h[c];
    tot[tid] = sum;
    __syncthreads();
    uint32_t run = 0;
    for (int d = 0; d < tid; ++d) run += tot[d];
    for (int c = 0; c < chunks; ++c) {
        const uint32_t v = h[c];
        h[c] = run;
        run += v;
    }
}

__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t n,
                                                            int chunks, int shift, const uint32_t* __restrict__ hist) {
    __shared__ uint32_t base[256];
    __shared__ uint32_t wcount[4][256];
    const int tid = int(threadIdx.x), lane = lane_id(), w = tid >> 6;
    const int label = int(blockIdx.x) / chunks, chunk = int(blockIdx.x) % chunks;
    const uint32_t* col = in + int64_t(label) * n;
    uint32_t* dst = out + int64_t(label) * n;
    base[tid] = hist[(int64_t(label) * 256 + tid) * chunks + chunk];
#pragma unroll
    for (int q = 0; q < 4; ++q) wcount[q][tid] = 0;
    __syncthreads();
    const int64_t cbase = int64_t(chunk) * RADIX_CHUNK;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int r = 0; r < RADIX_ROUNDS; ++r) {
        const int64_t i = cbase + r * 256 + tid;
        const bool valid = i < n;
        const uint32_t key = valid ? col[i] : 0u;
        const uint32_t d = (key >> shift) & 255u;
        // the lanes of this wave that hold the same digit: rank among them = the stable order inside the wave
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        const uint32_t rank = uint32_t(__popcll(peers & lt));
        if (valid && rank == 0) wcount[w][d] = uint32_t(__popcll(peers));
        __syncthreads();
        if (valid) {
            uint32_t off = base[d] + rank;
            for (int q = 0; q < w; ++q) off += wcount[q][d];
            if (off < n) dst[off] = key;   // (always, by the histogram this offset came from; the bound costs nothing)
        }
        __syncthreads();
        base[tid] += (wcount[0][tid] + wcount[1][tid]) + (wcount[2][tid] + wcount[3][tid]);
#pragma unroll
        for (int q = 0; q < 4; ++q) wcount[q][tid] = 0;
        __syncthreads();
    }
}

// ------------------------------------------------------------------ curve walk
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane_id() >= o) v += u;
    }
    return v;
}

__device__ __forceinline__ unsigned long long wave_incl_max(unsigned long long v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lo = __shfl_up(uint32_t(v), o, 64), hi = __shfl_up(uint32_t(v >> 32), o, 64);
        const unsigned long long u = (static_cast<unsigned long long>(hi) << 32) | lo;
        if (lane_id() >= o && u > v) v = u;
    }
    return v;
}

// Position i of the walk is array index n - 1 - i (score descending).  A group end is packed (count << 32) | tp, count = i + 1:
// both halves grow with i, so "the previous group's end" is a running maximum.
__global__ __launch_bounds__(256) void curve_walk_kernel(const uint32_t* __restrict__ keys, int64_t n64,
                                                         const uint32_t* __restrict__ invalid, double cutoff,
                                                         double* __restrict__ auc, double* __restrict__ aupr,
                                                         double* __restrict__ fdr, int64_t* __restrict__ n_pos,
                                                         int64_t* __restrict__ n_neg) {
    __shared__ uint32_t s_sum[4];
    __shared__ unsigned long long s_max[4];
    __shared__ unsigned long long r_auc[256];
    __shared__ double r_pr[256];
    __shared__ uint32_t r_fdr[256];
    const int tid = int(threadIdx.x), lane = lane_id(), w = tid >> 6;
    const uint32_t n = uint32_t(n64);
    const uint32_t* col = keys + int64_t(blockIdx.x) * n64;
    uint32_t carry_tp = 0;
    unsigned long long carry_prev = 0;
    unsigned long long acc_auc = 0;
    double acc_pr = 0.0;
    uint32_t acc_fdr = 0;
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
        uint32_t excl = carry_tp + incl - local;
        uint32_t tile_total = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < w) excl += s_sum[q];
            tile_total += s_sum[q];
        }
        // this thread's last group end
        uint32_t run = excl;
        unsigned long long last = 0;
#pragma unroll
        for (int j = 0; j < WALK_ITEMS; ++j) {
            if (k[j] != KEY_PAD) {
                run += k[j] & 1u;
                if ((k[j] >> 1) != (k[j + 1] >> 1)) last = (static_cast<unsigned long long>(i0 + j + 1) << 32) | run;
            }
        }
        const unsigned long long inclm = wave_incl_max(last);
        if (lane == 63) s_max[w] = inclm;
        const uint32_t up_lo = __shfl_up(uint32_t(inclm), 1, 64), up_hi = __shfl_up(uint32_t(inclm >> 32), 1, 64);
        unsigned long long prev = lane ? ((static_cast<unsigned long long>(up_hi) << 32) | up_lo) : 0ull;
        __syncthreads();
        if (carry_prev > prev) prev = carry_prev;
        unsigned long long tile_max = carry_prev;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned long long m = s_max[q];
            if (q < w && m > prev) prev = m;
            if (m > tile_max) tile_max = m;
        }
        run = excl;
#pragma unroll
        for (int j = 0; j < WALK_ITEMS; ++j) {
            if (k[j] != KEY_PAD) {
                run += k[j] & 1u;
                if ((k[j] >> 1) != (k[j + 1] >> 1)) {
                    const uint32_t cnt = i0 + j + 1, tp = run, fp = cnt - tp;
                    const uint32_t pcnt = uint32_t(prev >> 32), ptp = uint32_t(prev), pfp = pcnt - ptp;
                    acc_auc += static_cast<unsigned long long>(fp - pfp) * static_cast<unsigned long long>(tp + ptp);
                    const double q = double(tp) / double(cnt);
                    const double pq = pcnt ? double(ptp) / double(pcnt) : 1.0;
                    acc_pr += double(tp - ptp) * (q + pq);
                    if (1.0 - q <= cutoff && tp > acc_fdr) acc_fdr = tp;
                    prev = (static_cast<unsigned long long>(cnt) << 32) | tp;
                }
            }
        }
        carry_tp += tile_total;
        carry_prev = tile_max;
        __syncthreads();   // s_sum / s_max are rewritten by the next tile
    }
    r_auc[tid] = acc_auc;
    r_pr[tid] = acc_pr;
    r_fdr[tid] = acc_fdr;
    __syncthreads();
    if (tid == 0) {
        unsigned long long a = 0;
        double pr = 0.0;
        uint32_t f = 0;
        for (int q = 0; q < 256; ++q) {   // thread order: fixed
            a += r_auc[q];
            pr += r_pr[q];
            f = r_fdr[q] > f ? r_fdr[q] : f;
        }
        const uint32_t P = carry_tp, N = n - carry_tp;
        const bool bad = invalid[blockIdx.x] != 0;
        const double nan = __builtin_nan("");
        auc[blockIdx.x] = (bad || P == 0 || N == 0) ? nan : double(a) / double(2ull * P * N);
        aupr[blockIdx.x] = (bad || P == 0) ? nan : pr / (2.0 * double(P));
        fdr[blockIdx.x] = (bad || P == 0) ? nan : double(f) / double(P);
        if (n_pos) n_pos[blockIdx.x] = bad ? 0 : int64_t(P);
        if (n_neg) n_neg[blockIdx.x] = bad ? 0 : int64_t(N);
    }
}

// ------------------------------------------------------------------ thresholded counts
// One wave per row, 64 rows per wave: the per-sample counts are ballots, the per-label counts collect in LDS (a set prediction
// or a gold label is rare) and reach memory with one integer add per touched label and workgroup.
__global__ __launch_bounds__(256) void threshold_counts_kernel(const float* __restrict__ probs, int64_t ldp,
                                                               const float* __restrict__ targets, int64_t ldt, int64_t n, int L,
                                                               float threshold, int* __restrict__ lab_tp, int* __restrict__ lab_fp,
                                                               int* __restrict__ lab_fn, int* __restrict__ ex_tp,
                                                               int* __restrict__ ex_pred, int* __restrict__ ex_gold,
                                                               int* __restrict__ ex_mis) {
    __shared__ int s_cnt[3][COUNT_SLAB];
    const int tid = int(threadIdx.x), lane = lane_id(), w = tid >> 6;
    const int l_lo = int(blockIdx.y) * COUNT_SLAB;
    const int l_hi = l_lo + COUNT_SLAB < L ? l_lo + COUNT_SLAB : L;
    for (int i = tid; i < 3 * COUNT_SLAB; i += 256) (&s_cnt[0][0])[i] = 0;
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
                pred = (p != p ? 0.0f : p) >= threshold;
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

// ------------------------------------------------------------------ host side
inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct RankLayout {
    size_t keys_a, keys_b, hist, invalid, total;   // byte offsets; keys_b == hist == 0-sized on the LDS route
    int chunks;
    bool global_route;
};

// 0 = the shape is not served
bool rank_layout(int64_t n, int32_t L, RankLayout* out) {
    if (n <= 0 || L <= 0 || n >= (int64_t(1) << 31)) return false;
    RankLayout g{};
    g.global_route = n > SORT_LDS_MAX;
    g.chunks = g.global_route ? int((n + RADIX_CHUNK - 1) / RADIX_CHUNK) : 0;
    if (g.global_route && int64_t(g.chunks) * L >= (int64_t(1) << 31)) return false;
    const size_t keys = up256(size_t(n) * size_t(L) * sizeof(uint32_t));
    size_t off = 0;
    g.keys_a = off; off += keys;
    g.keys_b = off; off += g.global_route ? keys : 0;
    g.hist = off; off += g.global_route ? up256(size_t(L) * 256 * size_t(g.chunks) * sizeof(uint32_t)) : 0;
    g.invalid = off; off += up256(size_t(L) * sizeof(uint32_t));
    g.total = off + 256;   // the caller's base may be anywhere: one alignment allowance
    *out = g;
    return true;
}

AttrOnce g_sort_lds_attr;

}  // namespace
}  // namespace lamp

using namespace lamp;

// The sequence lamp_ranking_metrics and lamp_tune_thresholds (thresholds.hip) share: the workspace layout, the key build, the
// LDS or radix sort of every label column and the per-label `invalid` flags.  The caller has checked dimensions and pointers;
// LAMP_E_UNSUPPORTED / LAMP_E_WORKSPACE come back before anything is launched.
size_t lamp::rank_sort_workspace_bytes(int64_t n, int32_t L) {
    RankLayout g;
    return rank_layout(n, L, &g) ? g.total : 0;
}

int lamp::rank_sort_columns(const float* probs, int64_t ld_probs, const float* targets, int64_t ld_targets, int64_t n, int32_t L,
                            void* workspace, size_t workspace_bytes, lamp_stream_t stream, RankSorted* out) {
    RankLayout g;
    if (!rank_layout(n, L, &g)) return LAMP_E_UNSUPPORTED;
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
    if (workspace_bytes < g.total) return LAMP_E_WORKSPACE;   // (g.total holds the 255 bytes `base` may have moved)
    hipStream_t s = hipStream_t(stream);
    uint32_t* keys_a = reinterpret_cast<uint32_t*>(base + g.keys_a);
    uint32_t* keys_b = reinterpret_cast<uint32_t*>(base + g.keys_b);
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + g.hist);
    uint32_t* invalid = reinterpret_cast<uint32_t*>(base + g.invalid);
    if (hipError_t e = hipMemsetAsync(invalid, 0, size_t(L) * sizeof(uint32_t), s)) return int(e);
    const int64_t row_tiles = (n + 63) / 64;
    const int label_tiles = (L + 63) / 64;
    if (label_tiles > 65535) return LAMP_E_UNSUPPORTED;
    hipLaunchKernelGGL(metric_keys_kernel, dim3(unsigned(row_tiles), unsigned(label_tiles)), dim3(256), 0, s, probs, ld_probs,
                       targets, ld_targets, n, L, keys_a, invalid);
    const uint32_t* sorted = keys_a;
    if (!g.global_route) {
        int npow2 = 1;
        while (npow2 < n) npow2 <<= 1;
        const size_t lds = size_t(npow2) * sizeof(uint32_t);
        if (lds > 48 * 1024)
            if (int e = g_sort_lds_attr.set(reinterpret_cast<const void*>(sort_lds_kernel), size_t(SORT_LDS_MAX) * sizeof(uint32_t)))
                return e;
        hipLaunchKernelGGL(sort_lds_kernel, dim3(unsigned(L)), dim3(SORT_LDS_THREADS), lds, s, keys_a, n, npow2);
    } else {
        const unsigned blocks = unsigned(int64_t(g.chunks) * L);
        uint32_t* src = keys_a;
        uint32_t* dst = keys_b;
        for (int pass = 0; pass < 4; ++pass) {   // keys have 31 significant bits
            hipLaunchKernelGGL(radix_hist_kernel, dim3(blocks), dim3(256), 0, s, src, n, g.chunks, 8 * pass, hist);
            hipLaunchKernelGGL(radix_scan_kernel, dim3(unsigned(L)), dim3(256), 0, s, hist, g.chunks);
            hipLaunchKernelGGL(radix_scatter_kernel, dim3(blocks), dim3(256), 0, s, src, dst, n, g.chunks, 8 * pass, hist);
            uint32_t* t = src;
            src = dst;
            dst = t;
        }
        sorted = src;   // an even number of passes: keys_a again
    }
    out->keys = sorted;
    out->invalid = invalid;
    return 0;
}

size_t lamp_ranking_metrics_workspace_bytes(int64_t n_rows, int32_t L) {
    return rank_sort_workspace_bytes(n_rows, L);
}

int lamp_ranking_metrics(const float* probs, int64_t ld_probs, const float* targets, int64_t ld_targets, int64_t n_rows, int32_t L,
                         double fdr_cutoff, double* auc, double* aupr, double* fdr_recall, int64_t* n_pos, int64_t* n_neg,
                         void* workspace, size_t workspace_bytes, lamp_stream_t stream) {
    if (n_rows <= 0 || L <= 0 || ld_probs < L || ld_targets < L) return LAMP_E_DIMS;
    if (!probs || !targets || !auc || !aupr || !fdr_recall || !workspace) return LAMP_E_NULL;
    RankSorted r;
    if (int e = rank_sort_columns(probs, ld_probs, targets, ld_targets, n_rows, L, workspace, workspace_bytes, stream, &r)) return e;
    hipStream_t s = hipStream_t(stream);
    const uint32_t* sorted = r.keys;
    const uint32_t* invalid = r.invalid;
    hipLaunchKernelGGL(curve_walk_kernel, dim3(unsigned(L)), dim3(256), 0, s, sorted, n_rows, invalid, fdr_cutoff, auc, aupr,
                       fdr_recall, n_pos, n_neg);
    return int(hipGetLastError());
}

int lamp_threshold_counts(const float* probs, int64_t ld_probs, const float* targets, int64_t ld_targets, int64_t n_rows,
                          int32_t L, float threshold, int32_t* label_tp, int32_t* label_fp, int32_t* label_fn,
                          int32_t* sample_tp, int32_t* sample_pred, int32_t* sample_gold, int32_t* sample_mismatch,
                          lamp_stream_t stream) {
    if (n_rows <= 0 || L <= 0 || ld_probs < L || ld_targets < L) return LAMP_E_DIMS;
    if (!probs || !targets || !label_tp || !label_fp || !label_fn || !sample_tp || !sample_pred || !sample_gold ||
        !sample_mismatch)
        return LAMP_E_NULL;
    const int64_t row_blocks = (n_rows + 255) / 256;
    const int slabs = (L + COUNT_SLAB - 1) / COUNT_SLAB;
    // the per-label counts are int32: a label of 2^31 rows could not hold its own count
    if (n_rows >= (int64_t(1) << 31) || slabs > 65535) return LAMP_E_UNSUPPORTED;
    hipStream_t s = hipStream_t(stream);
    for (int32_t* p : {label_tp, label_fp, label_fn})
        if (hipError_t e = hipMemsetAsync(p, 0, size_t(L) * sizeof(int32_t), s)) return int(e);
    for (int32_t* p : {sample_tp, sample_pred, sample_gold, sample_mismatch})
        if (hipError_t e = hipMemsetAsync(p, 0, size_t(n_rows) * sizeof(int32_t), s)) return int(e);
    hipLaunchKernelGGL(threshold_counts_kernel, dim3(unsigned(row_blocks), unsigned(slabs)), dim3(256), 0, s, probs, ld_probs,
                       targets, ld_targets, n_rows, L, threshold, label_tp, label_fp, label_fn, sample_tp, sample_pred,
                       sample_gold, sample_mismatch);
    return int(hipGetLastError());
}

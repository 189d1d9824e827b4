// The live encoder's self-attention on the PACKED token rows (lamp_fwd_options: LAMP_FWD_PACKED_ENCODER): queries as ragged as
// keys.  Packed layout of one micro-batch of nb samples, extents from the device-side SeqPlan (no host read-back):
//     rows off[b] .. off[b] + plen[b] - 1   sample b's positions 0 .. plen[b] - 1 (interior PAD tokens keep their row)
//     row  n_tok + b                        sample b's ONE PAD row: every skipped position of a sample holds the same
//                                           row-wise result at every layer (zero input, same key set, row-local tail)
// Sample b's queries are its plen[b] rows and its PAD row; its keys are its plen[b] rows under its pad bits.  One wave per
// query row, keys strided over the lanes (scores in LDS), then P.V with the output columns over the lanes: plain fp32 FMA in
// a fixed order that depends on the sample's own rows only, so a sample's bits do not depend on T, on B or on the batch.
#include "lamp_kernels.h"

namespace lamp {

namespace {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// rows n_tok + b <- emb[PAD] (+ pos_table[0]); *count <- n_tok + nb.  One wave per sample.
__global__ __launch_bounds__(256) void pad_rows_kernel(const float* __restrict__ emb, const float* __restrict__ pos_table, int d,
                                                       int nb, SeqPlan sp, float* __restrict__ x, int* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int b = int(blockIdx.x) * 4 + int(threadIdx.x >> 6);
    if (b >= nb) return;
    const int n_tok = sp.off[nb];
    if (b == 0 && lane == 0) *count = n_tok + nb;
    float* o = x + (int64_t(n_tok) + b) * d;
    for (int c = lane; c < d; c += 64) o[c] = emb[c] + (pos_table ? pos_table[c] : 0.f);
}

// enc_output[b, j, :] <- packed row off[b] + j (j < plen[b]) or the sample's PAD row.  One wave per position; block 0 also
// returns the plan's hand-off words to "no epoch" (what the packed route's last LayerNorm does in the dead mode).
__global__ __launch_bounds__(256) void scatter_rows_kernel(const float* __restrict__ x, int d, int nb, int T, SeqPlan sp,
                                                           float* __restrict__ y) {
    if (sp.granules && blockIdx.x == 0)
        for (int i = threadIdx.x; i < 2 * nb + 2; i += 256) sp.granules[i] = 0ull;
    const int lane = threadIdx.x & 63;
    const int64_t flat = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (flat >= int64_t(nb) * T) return;
    const int b = int(flat / T), j = int(flat - int64_t(b) * T);
    const int64_t row = j < sp.plen[b] ? int64_t(sp.off[b]) + j : int64_t(sp.off[nb]) + b;
    const float4* s = reinterpret_cast<const float4*>(x + row * d);
    float4* o = reinterpret_cast<float4*>(y + flat * d);
    for (int c = lane; c < d / 4; c += 64) o[c] = s[c];
}

struct RaggedParams {
    const float *Q, *K, *V;   // [rows, H * dk | H * dv] packed projections
    float* O;                 // [rows, H * dv]
    int nb, H, T, dk, dv;
    float scale;              // 1 / sqrt(dk)
    SeqPlan sp;
};

// grid: (ceil((T + 1) / 4), H, nb); wave w of block x handles query slot 4 x + w of (sample, head): slot q < plen is the
// sample's row q, slot plen its PAD row, later slots do not exist.  LDS: per wave dk floats of q and T floats of scores.
__global__ __launch_bounds__(256) void attn_ragged_self_kernel(RaggedParams p) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z, h = blockIdx.y;
    const int slot = int(blockIdx.x) * 4 + wave;
    const int n = p.sp.plen[b];
    if (slot > n) return;
    const int64_t row0 = p.sp.off[b];
    const int64_t qrow = slot < n ? row0 + slot : int64_t(p.sp.off[p.nb]) + b;
    const int hdk = p.H * p.dk, hdv = p.H * p.dv;
    float* qs = lds + size_t(wave) * (p.dk + p.T);
    float* sc = qs + p.dk;
    const float* q = p.Q + qrow * hdk + h * p.dk;
    for (int c = lane; c < p.dk; c += 64) qs[c] = q[c];
    __builtin_amdgcn_wave_barrier();
    const unsigned* bits = p.sp.padbits + size_t(b) * p.sp.words;
    float m = -INFINITY;
    for (int k = lane; k < n; k += 64) {
        const float4* kr = reinterpret_cast<const float4*>(p.K + (row0 + k) * hdk + h * p.dk);
        float acc = 0.f;
        for (int c = 0; c < p.dk / 4; ++c) {
            const float4 kv = kr[c];
            acc = fmaf(qs[4 * c], kv.x, acc);
            acc = fmaf(qs[4 * c + 1], kv.y, acc);
            acc = fmaf(qs[4 * c + 2], kv.z, acc);
            acc = fmaf(qs[4 * c + 3], kv.w, acc);
        }
        const bool blocked = (bits[k >> 5] >> (k & 31)) & 1u;
        const float s = blocked ? -INFINITY : acc * p.scale;
        sc[k] = s;
        m = fmaxf(m, s);
    }
    m = wave_max(m);
    float l = 0.f;
    for (int k = lane; k < n; k += 64) {
        const float e = __expf(sc[k] - m);   // every key blocked (or none at all): -inf - -inf, NaN as the reference gives
        sc[k] = e;
        l += e;
    }
    l = wave64_sum(l);
    if (n == 0) l = __builtin_nanf("");
    __builtin_amdgcn_wave_barrier();
    float* o = p.O + qrow * hdv + h * p.dv;
    for (int c = lane; c < p.dv; c += 64) {
        const float* v = p.V + row0 * hdv + h * p.dv + c;
        float acc = 0.f;
        for (int k = 0; k < n; ++k) acc = fmaf(sc[k], v[int64_t(k) * hdv], acc);
        o[c] = acc / l;
    }
}

}  // namespace

bool attn_ragged_applies(int T, int dk, int dv) {
    return dk <= 128 && dv <= 128 && !(dk & 3) && !(dv & 3) && size_t(4) * (size_t(dk) + T) * sizeof(float) <= 65536;
}

int launch_pad_rows(const float* emb, const float* pos_table, int d, int nb, const SeqPlan& sp, float* x, int* count,
                    hipStream_t s) {
    if (!emb || !x || !count || nb <= 0 || d <= 0) return LAMP_E_NULL;
    hipLaunchKernelGGL(pad_rows_kernel, dim3(unsigned((nb + 3) / 4)), dim3(256), 0, s, emb, pos_table, d, nb, sp, x, count);
    return int(hipGetLastError());
}

int launch_scatter_rows(const float* x, int d, int nb, int T, const SeqPlan& sp, float* y, hipStream_t s) {
    if (!x || !y) return LAMP_E_NULL;
    if ((d & 3) || !aligned16(x) || !aligned16(y)) return LAMP_E_ALIGN;
    const int64_t blocks = (int64_t(nb) * T + 3) / 4;
    if (blocks > 0x7fffffffLL) return LAMP_E_DIMS;
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(unsigned(blocks)), dim3(256), 0, s, x, d, nb, T, sp, y);
    return int(hipGetLastError());
}

int launch_attn_ragged_self(const float* Q, const float* K, const float* V, float* O, int nb, int H, int T, int dk, int dv,
                            const SeqPlan& sp, hipStream_t s) {
    if (!Q || !K || !V || !O) return LAMP_E_NULL;
    if (nb <= 0 || nb > 65535 || H <= 0 || H > 65535 || T <= 0) return LAMP_E_DIMS;
    if (!attn_ragged_applies(T, dk, dv)) return LAMP_E_UNSUPPORTED;
    if (!aligned16(K)) return LAMP_E_ALIGN;
    const double flops = 2.0 * nb * H * double(T) * T * (dk + dv);
    ProfScope prof(LAMP_K_ATTN, flops, 4.0 * nb * H * double(T) * 2 * (dk + dv), s);
    RaggedParams p{Q, K, V, O, nb, H, T, dk, dv, float(1.0 / sqrt(double(dk))), sp};
    const size_t lds = size_t(4) * (size_t(dk) + T) * sizeof(float);
    hipLaunchKernelGGL(attn_ragged_self_kernel, dim3(unsigned((T + 1 + 3) / 4), unsigned(H), unsigned(nb)), dim3(256), lds, s, p);
    return int(hipGetLastError());
}

}  // namespace lamp

// The one-hot genomics front end of GraphEncoder (lamp/Encoders.py:46-51,68-73):
//
//   y1 = conv1(E[src]^T)[:, :, :T]   Conv1d(9, d, 16, padding 8): the input is one-hot, so conv1 is a GATHER from the
//                                    weights-only tap table T1[v, t, :] = sum_ci E[v, ci] W1[:, ci, t] (lamp_onehot_frontend.t1)
//   P  = max_pool1d(relu(dropout(y1)), 2, 2)                          -> T2 = T / 2 rows
//   X  = relu(conv2(P)[:, :, :T2])^T + position_enc(src_pos[:, :T2])   Conv1d(d, d, 16, padding 8)
//
// Channel-last, every sample's P zero-padded by 8 rows in front and 8 behind (Tp = T2 + 16 rows), the 16 input rows that
// conv2's output q reads are CONTIGUOUS: row q of the im2col matrix is the 16 d floats starting at padded row q.  conv2 is
// therefore an implicit GEMM with K = 16 d and a row stride of d against W2 repacked [co][t][ci] (conv_pack_kernel), and
// so is its input gradient (the ReLU-masked dY, padded the same way, against the flipped repack [ci][15 - t][co]).
//
// conv_window_kernel: 128 x 128 output tile per 256-thread workgroup, K in steps of 32 staged global -> registers -> LDS
// (the next step's loads in flight under the current step's MFMAs), each wave a 64 x 64 sub-tile of 2 x 2
// v_mfma_f32_32x32x2_f32 blocks.  Each lane reads four consecutive k of its row with one ds_read_b128 and feeds component j
// to MFMA step j (the same k permutation on both operands, gemm.hip).  The k order of every output element is fixed by K
// alone, so a sample's rows are bit-identical for every batch size and micro-batch split.
#include "lamp_kernels.h"

namespace lamp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------- front end
// a[p][c] = relu(dropout(y1[p][c])) of sample b, p < T.  Out-of-range tokens give NaN (as the embedding gathers do).
__device__ __forceinline__ float4 front_act(const int64_t* __restrict__ seq, int T, int p, const float* __restrict__ t1,
                                            int n_vocab, const float* __restrict__ b1, int d, int c, int64_t e0,
                                            const DropoutSpec& drop) {
    float4 y = *reinterpret_cast<const float4*>(b1 + c);
    bool bad = false;
#pragma unroll 4
    for (int t = 0; t < 16; ++t) {
        const int j = p + t - 8;
        if (j < 0 || j >= T) continue;
        const int64_t v = seq[j];
        if (v < 0 || v >= n_vocab) { bad = true; continue; }
        const float4 w = *reinterpret_cast<const float4*>(t1 + (v * 16 + t) * int64_t(d) + c);
        y.x += w.x; y.y += w.y; y.z += w.z; y.w += w.w;
    }
    if (bad) y = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
    if (drop.threshold) y = drop4(y, e0, drop);
    // ReLU that lets a NaN through (torch.relu does), so an invalid token poisons its positions instead of zeroing them
    auto relu = [](float v) { return (v > 0.f || v != v) ? v : 0.f; };
    return make_float4(relu(y.x), relu(y.y), relu(y.z), relu(y.w));
}

// pair max with max_pool1d's choice: the first element wins ties (and a NaN is propagated)
__device__ __forceinline__ float pmax(float a, float b) { return (b > a || b != b) ? b : a; }

// xpad [nb * Tp + 16, d]: row b * Tp + 8 + q = P[b][q]; the 8 rows before and after each sample and the 16 trailing rows are 0.
// Dropout element index of y1[b][p][c]: (b0 + b) * T * d + p * d + c (channel-last, b0 = first sample of this call).
__global__ __launch_bounds__(256) void front_fwd_kernel(const int64_t* __restrict__ seq, int nb, int T, int T2,
                                                        const float* __restrict__ t1, int n_vocab, const float* __restrict__ b1,
                                                        int d, DropoutSpec drop, int64_t e_base, float* __restrict__ xpad) {
    const int c4 = d / 4, Tp = T2 + 16;
    const int64_t total = (int64_t(nb) * Tp + 16) * c4;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += int64_t(gridDim.x) * 256) {
        const int64_t row = i / c4;
        const int c = int(i - row * c4) * 4;
        const int b = int(row / Tp), r = int(row - int64_t(b) * Tp);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < nb && r >= 8 && r < 8 + T2) {
            const int q = r - 8;
            const int64_t* s = seq + int64_t(b) * T;
            const int64_t e0 = e_base + (int64_t(b) * T + 2 * q) * d + c;
            const float4 a0 = front_act(s, T, 2 * q, t1, n_vocab, b1, d, c, e0, drop);
            const float4 a1 = front_act(s, T, 2 * q + 1, t1, n_vocab, b1, d, c, e0 + d, drop);
            v = make_float4(pmax(a0.x, a1.x), pmax(a0.y, a1.y), pmax(a0.z, a1.z), pmax(a0.w, a1.w));
        }
        *reinterpret_cast<float4*>(xpad + row * d + c) = v;
    }
}

// Backward of pool, ReLU and dropout: dz[b][p][c] = gradient of y1[b][p][c] (p < T), from dP [nb, T2, d] (ld d).
__global__ __launch_bounds__(256) void front_bwd_kernel(const int64_t* __restrict__ seq, int nb, int T, int T2,
                                                        const float* __restrict__ t1, int n_vocab, const float* __restrict__ b1,
                                                        int d, DropoutSpec drop, const float* __restrict__ dP,
                                                        float* __restrict__ dz) {
    const int c4 = d / 4;
    const int64_t total = int64_t(nb) * T * c4;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += int64_t(gridDim.x) * 256) {
        const int64_t row = i / c4;
        const int c = int(i - row * c4) * 4;
        const int b = int(row / T), p = int(row - int64_t(b) * T);
        const int q = p >> 1;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < T2) {
            const int64_t* s = seq + int64_t(b) * T;
            const int64_t e0 = (int64_t(b) * T + 2 * q) * d + c;
            const float4 a0 = front_act(s, T, 2 * q, t1, n_vocab, b1, d, c, e0, drop);
            const float4 a1 = front_act(s, T, 2 * q + 1, t1, n_vocab, b1, d, c, e0 + d, drop);
            const float4 up = *reinterpret_cast<const float4*>(dP + (int64_t(b) * T2 + q) * d + c);
            const bool first = (p & 1) == 0;
            const float4 a = first ? a0 : a1;
            // the pair's winner (first on ties) takes the gradient; ReLU passes it where the output is > 0; dropout scales
            // the kept elements
            auto pick = [&](float x0, float x1, float ax, float u) {
                const bool win0 = !(x1 > x0 || x1 != x1);
                return (win0 == first && ax > 0.f) ? (drop.threshold ? u * drop.scale : u) : 0.f;
            };
            g = make_float4(pick(a0.x, a1.x, a.x, up.x), pick(a0.y, a1.y, a.y, up.y), pick(a0.z, a1.z, a.z, up.z),
                            pick(a0.w, a1.w, a.w, up.w));
        }
        *reinterpret_cast<float4*>(dz + row * d + c) = g;
    }
}

// Partial tap-table gradients: partial[chunk][v][t][c] = sum over the rows (b, p) of `chunk` with src[b][p + t - 8] == v of
// dz[b][p][c].  One thread per (t, c); the row order inside a chunk and the chunk split depend on (nb, T) only.
constexpr int DT1_ROWS = 256;
constexpr int MAX_VOCAB = 16;
__global__ __launch_bounds__(256) void front_dt1_kernel(const int64_t* __restrict__ seq, int nb, int T, int n_vocab, int d,
                                                        const float* __restrict__ dz, float* __restrict__ partial) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 16 * d) return;
    const int t = idx / d, c = idx - t * d;
    const int64_t rows = int64_t(nb) * T;
    const int64_t r0 = int64_t(blockIdx.y) * DT1_ROWS;
    const int64_t r1 = r0 + DT1_ROWS < rows ? r0 + DT1_ROWS : rows;
    float acc[MAX_VOCAB];
#pragma unroll
    for (int v = 0; v < MAX_VOCAB; ++v) acc[v] = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
        const int b = int(r / T), p = int(r - int64_t(b) * T);
        const int j = p + t - 8;
        if (j < 0 || j >= T) continue;
        const int64_t tok = seq[int64_t(b) * T + j];
        const float g = dz[r * d + c];
#pragma unroll
        for (int v = 0; v < MAX_VOCAB; ++v) acc[v] += tok == v ? g : 0.f;
    }
    float* o = partial + int64_t(blockIdx.y) * n_vocab * 16 * d;
#pragma unroll
    for (int v = 0; v < MAX_VOCAB; ++v)
        if (v < n_vocab) o[(int64_t(v) * 16 + t) * d + c] = acc[v];
}

// ---------------------------------------------------------------- weight repack
// flip = 0: packed[co][t][ci] = w[co][ci][t]          (conv2 forward)
// flip = 1: packed[ci][t][co] = w[co][ci][taps-1-t]   (its input gradient)
__global__ __launch_bounds__(256) void conv_pack_kernel(const float* __restrict__ w, int c_out, int c_in, int taps, int flip,
                                                        float* __restrict__ packed) {
    const int64_t total = int64_t(c_out) * c_in * taps;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += int64_t(gridDim.x) * 256) {
        if (!flip) {
            const int64_t co = i / (int64_t(taps) * c_in);
            const int rem = int(i - co * taps * c_in);
            const int t = rem / c_in, ci = rem - t * c_in;
            packed[i] = w[(co * c_in + ci) * taps + t];
        } else {
            const int64_t ci = i / (int64_t(taps) * c_out);
            const int rem = int(i - ci * taps * c_out);
            const int t = rem / c_out, co = rem - t * c_out;
            packed[i] = w[(int64_t(co) * c_in + ci) * taps + (taps - 1 - t)];
        }
    }
}

// ---------------------------------------------------------------- conv as an implicit GEMM
// out[m][n] = act(sum_k x[row(m) * c_in + k] * w[n][k] + bias[n]) + pos[src_pos[b * pos_ld + q]][n],  k < K = taps * c_in,
// m = b * rows_out + q, row(m) = b * rows_in + q.  relu_out (nullable) receives act(...) before the position row.
constexpr int CV_BM = 128, CV_BN = 128, CV_BK = 32, CV_LDS = CV_BK + 4;

__global__ __launch_bounds__(256) void conv_window_kernel(ConvWindowParams p) {
    __shared__ float4 lds_a[CV_BM * CV_LDS / 4];
    __shared__ float4 lds_b[CV_BN * CV_LDS / 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = int64_t(blockIdx.x) * CV_BM;
    const int n0 = blockIdx.y * CV_BN;
    const int M_last = int(p.M - 1);

    // staging: thread tid moves rows tid / 8 + 32 i, k quad tid % 8, of both tiles
    auto a_row = [&](int i) {
        int64_t m = m0 + tid / 8 + 32 * i;
        if (m > M_last) m = M_last;
        const int64_t b = m / p.rows_out, q = m - b * p.rows_out;
        return p.x + (b * p.rows_in + q) * p.c_in + (tid & 7) * 4;
    };
    auto b_row = [&](int i) {
        int n = n0 + tid / 8 + 32 * i;
        if (n > p.N - 1) n = p.N - 1;
        return p.w + int64_t(n) * p.K + (tid & 7) * 4;
    };
    const float *ga0 = a_row(0), *ga1 = a_row(1), *ga2 = a_row(2), *ga3 = a_row(3);
    const float *gb0 = b_row(0), *gb1 = b_row(1), *gb2 = b_row(2), *gb3 = b_row(3);
    float4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;
#define CV_LOAD(k0)                                                                                  \
    ra0 = *reinterpret_cast<const float4*>(ga0 + (k0)); ra1 = *reinterpret_cast<const float4*>(ga1 + (k0)); \
    ra2 = *reinterpret_cast<const float4*>(ga2 + (k0)); ra3 = *reinterpret_cast<const float4*>(ga3 + (k0)); \
    rb0 = *reinterpret_cast<const float4*>(gb0 + (k0)); rb1 = *reinterpret_cast<const float4*>(gb1 + (k0)); \
    rb2 = *reinterpret_cast<const float4*>(gb2 + (k0)); rb3 = *reinterpret_cast<const float4*>(gb3 + (k0));
#define CV_STASH()                                                                                      \
    lds_a[st] = ra0; lds_a[st + 32 * CV_LDS / 4] = ra1; lds_a[st + 64 * CV_LDS / 4] = ra2; lds_a[st + 96 * CV_LDS / 4] = ra3; \
    lds_b[st] = rb0; lds_b[st + 32 * CV_LDS / 4] = rb1; lds_b[st + 64 * CV_LDS / 4] = rb2; lds_b[st + 96 * CV_LDS / 4] = rb3;
    const int st = ((tid / 8) * CV_LDS) / 4 + (tid & 7);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = p.K / CV_BK;
    CV_LOAD(0)
    CV_STASH()
    __syncthreads();
    const int fr = lane & 31, fh = lane >> 5;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) { CV_LOAD((kt + 1) * CV_BK) }
#pragma unroll
        for (int cc = 0; cc < CV_BK / 8; ++cc) {
            float4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = lds_a[((wm * 64 + i * 32 + fr) * CV_LDS) / 4 + 2 * cc + fh];
                fb[i] = lds_b[((wn * 64 + i * 32 + fr) * CV_LDS) / 4 + 2 * cc + fh];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[j].w, acc[i][j], 0, 0, 0);
                }
        }
        __syncthreads();
        if (kt + 1 < nk) {
            CV_STASH()
            __syncthreads();
        }
    }

#undef CV_LOAD
#undef CV_STASH
    // epilogue: lane holds column n = lane & 31 of each 32 x 32 block, rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 64 + j * 32 + fr;
        if (n >= p.N) continue;
        const float bias = p.bias ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                if (m >= p.M) continue;
                float v = acc[i][j][r] + bias;
                if (p.relu) v = v > 0.f ? v : 0.f;
                if (p.relu_out) p.relu_out[m * p.N + n] = v;
                if (p.pos_table) {
                    const int64_t b = m / p.rows_out, q = m - b * p.rows_out;
                    const int64_t ps = p.src_pos[b * p.pos_ld + q];
                    v += (ps >= 0 && ps < p.n_position) ? p.pos_table[ps * p.N + n] : __builtin_nanf("");
                }
                p.out[m * p.ldo + n] = v;
            }
    }
}

// dZ [nb * Tp + 16, d] = dY * (relu_out > 0) in the padded layout of xpad (8 zero rows before, 8 after each sample, 16 trailing)
__global__ __launch_bounds__(256) void relu_bwd_pad_kernel(const float* __restrict__ dy, const float* __restrict__ relu_out,
                                                           int nb, int T2, int d, float* __restrict__ dz) {
    const int c4 = d / 4, Tp = T2 + 16;
    const int64_t total = (int64_t(nb) * Tp + 16) * c4;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += int64_t(gridDim.x) * 256) {
        const int64_t row = i / c4;
        const int c = int(i - row * c4) * 4;
        const int b = int(row / Tp), r = int(row - int64_t(b) * Tp);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < nb && r >= 8 && r < 8 + T2) {
            const int64_t src = (int64_t(b) * T2 + r - 8) * d + c;
            const float4 g = *reinterpret_cast<const float4*>(dy + src);
            const float4 o = *reinterpret_cast<const float4*>(relu_out + src);
            v = make_float4(o.x > 0.f ? g.x : 0.f, o.y > 0.f ? g.y : 0.f, o.z > 0.f ? g.z : 0.f, o.w > 0.f ? g.w : 0.f);
        }
        *reinterpret_cast<float4*>(dz + row * d + c) = v;
    }
}

// ---------------------------------------------------------------- launchers
static unsigned grid_for(int64_t items) {
    const int64_t g = (items + 255) / 256;
    return unsigned(g < 8192 ? (g > 0 ? g : 1) : 8192);
}

int launch_front_fwd(const int64_t* seq, int nb, int T, const float* t1, int n_vocab, const float* b1, int d, float p_drop,
                     uint32_t seed, int64_t e_base, float* xpad, hipStream_t s) {
    if (nb <= 0 || T < 2 || d <= 0 || n_vocab <= 0 || n_vocab > MAX_VOCAB) return LAMP_E_DIMS;
    if (d & 3) return LAMP_E_UNSUPPORTED;
    if (!seq || !t1 || !b1 || !xpad) return LAMP_E_NULL;
    if (!aligned16(t1) || !aligned16(b1) || !aligned16(xpad)) return LAMP_E_ALIGN;
    const int T2 = T / 2;
    const int64_t items = (int64_t(nb) * (T2 + 16) + 16) * (d / 4);
    ProfScope prof(LAMP_K_EMBED, 2.0 * 16 * double(nb) * 2 * T2 * d, 4.0 * double(items) * 4, s);
    hipLaunchKernelGGL(front_fwd_kernel, dim3(grid_for(items)), dim3(256), 0, s, seq, nb, T, T2, t1, n_vocab, b1, d,
                       make_dropout(p_drop, seed), e_base, xpad);
    return int(hipGetLastError());
}

int launch_conv_window(const ConvWindowParams& p, hipStream_t s) {
    // every output row reads K / c_in consecutive input rows from b * rows_in + q: they must stay inside the sample's rows
    if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.c_in <= 0 || p.rows_out <= 0) return LAMP_E_DIMS;
    if (p.K % p.c_in || p.rows_in < p.rows_out + p.K / p.c_in - 1) return LAMP_E_DIMS;
    if ((p.K % CV_BK) || (p.c_in & 3) || (p.ldo < p.N)) return LAMP_E_UNSUPPORTED;
    if (!p.x || !p.w || !p.out || (p.pos_table && !p.src_pos)) return LAMP_E_NULL;
    if (!aligned16(p.x) || !aligned16(p.w)) return LAMP_E_ALIGN;
    const int64_t gm = (p.M + CV_BM - 1) / CV_BM;
    if (gm > 0x7fffffffLL) return LAMP_E_DIMS;
    ProfScope prof(LAMP_K_GEMM, 2.0 * double(p.M) * p.N * p.K, 4.0 * (double(p.M) * p.K / 16 + double(p.N) * p.K + double(p.M) * p.N), s);
    hipLaunchKernelGGL(conv_window_kernel, dim3(unsigned(gm), unsigned((p.N + CV_BN - 1) / CV_BN)), dim3(256), 0, s, p);
    return int(hipGetLastError());
}

int launch_conv_pack(const float* w, int c_out, int c_in, int taps, int flip, float* packed, hipStream_t s) {
    if (c_out <= 0 || c_in <= 0 || taps <= 0) return LAMP_E_DIMS;
    if (!w || !packed) return LAMP_E_NULL;
    hipLaunchKernelGGL(conv_pack_kernel, dim3(grid_for(int64_t(c_out) * c_in * taps)), dim3(256), 0, s, w, c_out, c_in, taps,
                       flip, packed);
    return int(hipGetLastError());
}

int launch_relu_bwd_pad(const float* dy, const float* relu_out, int nb, int T2, int d, float* dz, hipStream_t s) {
    if (nb <= 0 || T2 <= 0 || d <= 0) return LAMP_E_DIMS;
    if (d & 3) return LAMP_E_UNSUPPORTED;
    if (!dy || !relu_out || !dz) return LAMP_E_NULL;
    if (!aligned16(dy) || !aligned16(relu_out) || !aligned16(dz)) return LAMP_E_ALIGN;
    hipLaunchKernelGGL(relu_bwd_pad_kernel, dim3(grid_for((int64_t(nb) * (T2 + 16) + 16) * (d / 4))), dim3(256), 0, s, dy,
                       relu_out, nb, T2, d, dz);
    return int(hipGetLastError());
}

int64_t front_dt1_chunks(int nb, int T) { return (int64_t(nb) * T + DT1_ROWS - 1) / DT1_ROWS; }

int launch_front_bwd(const int64_t* seq, int nb, int T, const float* t1, int n_vocab, const float* b1, int d, float p_drop,
                     uint32_t seed, const float* dP, float* dz, float* partial, hipStream_t s) {
    if (nb <= 0 || T < 2 || d <= 0 || n_vocab <= 0 || n_vocab > MAX_VOCAB) return LAMP_E_DIMS;
    if (d & 3) return LAMP_E_UNSUPPORTED;
    if (!seq || !t1 || !b1 || !dP || !dz || !partial) return LAMP_E_NULL;
    if (!aligned16(t1) || !aligned16(b1) || !aligned16(dP) || !aligned16(dz)) return LAMP_E_ALIGN;
    const int64_t chunks = front_dt1_chunks(nb, T);
    if (chunks > 65535) return LAMP_E_DIMS;
    const int64_t items = int64_t(nb) * T * (d / 4);
    hipLaunchKernelGGL(front_bwd_kernel, dim3(grid_for(items)), dim3(256), 0, s, seq, nb, T, T / 2, t1, n_vocab, b1, d,
                       make_dropout(p_drop, seed), dP, dz);
    if (hipError_t e = hipGetLastError()) return int(e);
    hipLaunchKernelGGL(front_dt1_kernel, dim3(unsigned((16 * d + 255) / 256), unsigned(chunks)), dim3(256), 0, s, seq, nb, T,
                       n_vocab, d, dz, partial);
    return int(hipGetLastError());
}

}  // namespace lamp

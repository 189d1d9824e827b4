// fp32-in / fp32-out GEMM  C_s = act(A . W_s^T + bias_s) + R  on the bf16 matrix pipe of CDNA4 (v_mfma_f32_16x16x32_bf16): every fp32
// operand is split into bf16 pieces and every fp32 product is replaced by a few bf16 products accumulated in fp32 -- the "treat each
// float32 as the sum of three bfloat16 numbers" meaning of torch.set_float32_matmul_precision('high').  gfx950 has no TF32 and its
// fp32 matrix pipe runs at 1/16 of the bf16 one, so three (or six) bf16 products can still be cheaper than one fp32 product.
//
//   split:  h = bf16(x),  m = bf16(x - h),  l = bf16(x - h - m)        (round to nearest even; h + m + l carries 24 mantissa bits)
//   nprod = 3:  a.w ~= a_m w_h + a_h w_m + a_h w_h                     (only the h and m planes are staged)
//   nprod = 6:  a.w ~= a_l w_h + a_h w_l + a_m w_m + a_m w_h + a_h w_m + a_h w_h
// per 32-wide k-chunk, in exactly this order (smallest terms first), in fp32: the cross terms on one accumulator chain, the h.h
// products on a second, the two added once after the last chunk.
//
// Same contract as launch_gemm (gemm.hip): K-contiguous operands, 1-4 weight segments sharing A, bias / ReLU / residual, the gathered
// residual, a device-side row count (m_dev, A_dense), any K / lda / ldw that are multiples of 4 (columns past K are staged as zeros),
// odd N / ldc through the scalar epilogue.  Operands stay fp32 in memory: each tile is split while it is staged into LDS -- no
// pre-split weight copies, no workspace.
//
// Bit rule, as in gemm.hip: an output element's bits depend on (K, nprod) alone.  Every tile of the menu is built from the same
// 16x16x32 block, the same BK = 32 and the same product order, with no split over K; the tile is chosen from the launch's shape, which
// therefore never changes a bit, and rows are independent (a NaN row of A stays in its own row of C).
//
// The one semantic deviation from the fp32 kernel: a non-finite operand.  x = inf gives h = inf and m = bf16(inf - inf) = NaN, so the
// product is NaN where fp32 arithmetic gives inf.  (NaN operands give NaN in both.)
#include <type_traits>

#include "lamp_kernels.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

namespace lamp {

namespace {

constexpr int SBK = 32;        // k per staged tile = k of one MFMA
constexpr int SLS = SBK + 8;   // LDS row stride in bf16: 80 bytes, an odd number of 16-byte slots per row

template <int BM, int BN, int WAVES_M, int WAVES_N, int NPLANE>
struct SplitTile {
    static constexpr int NT = WAVES_M * WAVES_N * 64;
    static constexpr int WTM = BM / WAVES_M;
    static constexpr int WTN = BN / WAVES_N;
    static constexpr int MI = WTM / 16;
    static constexpr int NI = WTN / 16;
    static constexpr int A_LD = BM * SBK / 4 / NT;   // float4 loads per thread per tile
    static constexpr int B_LD = BN * SBK / 4 / NT;
    static constexpr int LDS_BYTES = NPLANE * (BM + BN) * SLS * 2;
    static_assert(WTM % 16 == 0 && WTN % 16 == 0, "wave tile must be a multiple of the MFMA block");
    static_assert((BM * SBK / 4) % NT == 0 && (BN * SBK / 4) % NT == 0, "staging must divide evenly");
    static_assert(LDS_BYTES <= 64 * 1024, "static LDS");
};

// x -> bf16 pieces (NPLANE of them), round to nearest even
template <int NPLANE>
__device__ __forceinline__ void split_store(float4 v, __bf16* dst, int plane_stride) {
    const float x[4] = {v.x, v.y, v.z, v.w};
    bf16x4 h, m, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h[e] = (__bf16)x[e];
        const float r = x[e] - (float)h[e];
        m[e] = (__bf16)r;
        if constexpr (NPLANE == 3) l[e] = (__bf16)(r - (float)m[e]);
    }
    *reinterpret_cast<bf16x4*>(dst) = h;
    *reinterpret_cast<bf16x4*>(dst + plane_stride) = m;
    if constexpr (NPLANE == 3) *reinterpret_cast<bf16x4*>(dst + 2 * plane_stride) = l;
}

// One tile per workgroup.  VEC: bias / residual / C move as 16-byte accesses; RGATHER: the residual is gathered from the embedding
// tables (GemmParams::rg_tok), VEC only.
template <int BM, int BN, int WAVES_M, int WAVES_N, int NPLANE, bool VEC, bool RGATHER>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void gemm_split_kernel(GemmParams p, int tiles_n_seg, int tiles_n, int tiles_m) {
    using T = SplitTile<BM, BN, WAVES_M, WAVES_N, NPLANE>;
    static_assert(!RGATHER || VEC, "the gathered residual reads its tables 16 bytes at a time");
    __shared__ __attribute__((aligned(16))) __bf16 As[NPLANE * BM * SLS];   // [plane][row][SLS]
    __shared__ __attribute__((aligned(16))) __bf16 Bs[NPLANE * BN * SLS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int l15 = lane & 15, hi = lane >> 4;   // row within a 16x16 block, which 8 consecutive k this lane's fragment covers

    // Row count from device memory (ragged batches): the launch was sized for the host's upper bound p.M
    int64_t M = p.M;
    if (p.m_dev) {
        M = *p.m_dev;
        if (M > p.M) M = p.M;
        tiles_m = int((M + BM - 1) / BM);
    }
    const int nwg = tiles_m * tiles_n;
    if (int(blockIdx.x) >= nwg) return;
    // Placement only (see gemm.hip): each XCD gets a contiguous range of items; inside it groups of 8 row-panels are walked
    // column-panel by column-panel, so the tiles in flight on one L2 share a few panels of A and W.
    const int item = xcd_remap(blockIdx.x, nwg);
    constexpr int GROUP_M = 8;
    const int group_sz = GROUP_M * tiles_n;
    const int grp = item / group_sz;
    const int in_grp = item - grp * group_sz;
    const int first_m = grp * GROUP_M;
    const int gm = tiles_m - first_m < GROUP_M ? tiles_m - first_m : GROUP_M;
    const int tn_all = in_grp / gm;
    const int tm = first_m + (in_grp - tn_all * gm);
    const int seg = tn_all / tiles_n_seg;
    const int tn = tn_all - seg * tiles_n_seg;
    const int64_t m0 = int64_t(tm) * BM;
    const int n0 = tn * BN;
    const int rows_m = int(M - m0 < BM ? M - m0 : BM);   // valid rows / columns of this tile
    const int rows_n = p.N - n0 < BN ? p.N - n0 : BN;

    const int lda = int(p.lda), ldw = int(p.ldw);
    const float* Abase = p.A;
    if (p.A_dense) {
        if (p.m_dev[0] == p.m_dev[1]) Abase = p.A_dense;
    }
    // rows past the tile's valid rows fall outside the descriptor and read as 0; columns past K are steered out of range below
    const __amdgpu_buffer_rsrc_t rsA = make_rsrc(Abase + m0 * p.lda, (uint64_t(rows_m - 1) * lda + p.K) * 4u);
    const __amdgpu_buffer_rsrc_t rsW = make_rsrc(p.W[seg] + int64_t(n0) * p.ldw, (uint64_t(rows_n - 1) * ldw + p.K) * 4u);

    // Two fp32 accumulator chains per output element: `acc` takes the h.h products (the value itself), `lo` every cross term (2^-8 of
    // it and below); lo is added to acc once, after the last k-step.  The cross terms' rounding errors are then 2^-8 of an ulp of
    // the result each, and the main chain rounds once per 32 k instead of once per product.
    f32x4 acc[T::MI][T::NI], lo[T::MI][T::NI];
#pragma unroll
    for (int i = 0; i < T::MI; ++i)
#pragma unroll
        for (int j = 0; j < T::NI; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = lo[i][j][r] = 0.f;

    constexpr int C4 = SBK / 4;   // float4 per tile row
    float4 ra[T::A_LD], rb[T::B_LD];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < T::A_LD; ++i) {
            const int idx = tid + i * T::NT;
            const int row = idx / C4, k = k0 + (idx % C4) * 4;
            ra[i] = bload4(rsA, k < p.K ? unsigned(row * lda + k) * 4u : OOB, 0);
        }
#pragma unroll
        for (int i = 0; i < T::B_LD; ++i) {
            const int idx = tid + i * T::NT;
            const int row = idx / C4, k = k0 + (idx % C4) * 4;
            rb[i] = bload4(rsW, k < p.K ? unsigned(row * ldw + k) * 4u : OOB, 0);
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < T::A_LD; ++i) {
            const int idx = tid + i * T::NT;
            split_store<NPLANE>(ra[i], As + (idx / C4) * SLS + (idx % C4) * 4, BM * SLS);
        }
#pragma unroll
        for (int i = 0; i < T::B_LD; ++i) {
            const int idx = tid + i * T::NT;
            split_store<NPLANE>(rb[i], Bs + (idx / C4) * SLS + (idx % C4) * 4, BN * SLS);
        }
    };
    // The products are issued TRANSPOSED, as in gemm.hip -- W fragment as the MFMA's A operand, activation fragment as its B operand --
    // so lane (m = lane & 15, hi) owns four CONSECUTIVE output columns 4 hi + r of ITS output row m.
    auto compute = [&]() {
        const __bf16* a = As + (wm * T::WTM + l15) * SLS + hi * 8;
        const __bf16* b = Bs + (wn * T::WTN + l15) * SLS + hi * 8;
        bf16x8 fa[NPLANE][T::MI], fb[NPLANE][T::NI];
#pragma unroll
        for (int q = 0; q < NPLANE; ++q) {
#pragma unroll
            for (int i = 0; i < T::MI; ++i) fa[q][i] = *reinterpret_cast<const bf16x8*>(a + q * BM * SLS + i * 16 * SLS);
#pragma unroll
            for (int j = 0; j < T::NI; ++j) fb[q][j] = *reinterpret_cast<const bf16x8*>(b + q * BN * SLS + j * 16 * SLS);
        }
        // (activation plane, weight plane) of each product, smallest first; planes: 0 = h, 1 = m, 2 = l.  The product is the outer
        // loop: consecutive MFMAs go to different accumulators, every accumulator still sees its products in this order.
        //   t:   0    1    2    3    4    5
        //   a:   l    h    m    m    h    h
        //   w:   h    l    m    h    m    h
#pragma unroll
        for (int t = NPLANE == 3 ? 0 : 3; t < 6; ++t) {
            const int qa = t == 0 ? 2 : (t == 2 || t == 3) ? 1 : 0;
            const int qw = t == 1 ? 2 : (t == 2 || t == 4) ? 1 : 0;
#pragma unroll
            for (int i = 0; i < T::MI; ++i)
#pragma unroll
                for (int j = 0; j < T::NI; ++j) {
                    const bf16x8 w = fb[qw < NPLANE ? qw : 0][j], a = fa[qa < NPLANE ? qa : 0][i];
                    if (t < 5) lo[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, lo[i][j], 0, 0, 0);
                    else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, acc[i][j], 0, 0, 0);
                }
        }
    };

    const int nk = (p.K + SBK - 1) / SBK;
    gload(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();   // the previous step's fragment reads are done
        lstore();
        __syncthreads();
        if (kt + 1 < nk) gload((kt + 1) * SBK);   // in flight under the MFMAs
        compute();
    }

#pragma unroll
    for (int i = 0; i < T::MI; ++i)
#pragma unroll
        for (int j = 0; j < T::NI; ++j) acc[i][j] += lo[i][j];

    // Epilogue (gemm.hip's, one register quad per block).  Stores to rows past M fall outside the descriptor and are dropped by the
    // hardware; columns past N are steered to an out-of-range offset.
    const int ldc = int(p.ldc), ldr = int(p.ldr);
    const bool has_r = RGATHER || p.R != nullptr;
    const bool read_r = !RGATHER && p.R != nullptr;
    const __amdgpu_buffer_rsrc_t rsR =
        make_rsrc(read_r ? p.R + m0 * p.ldr + n0 : p.A, read_r ? (uint64_t(rows_m - 1) * ldr + rows_n) * 4u : 0);
    const float* bias = p.bias[seg];
    const __amdgpu_buffer_rsrc_t rsBias = make_rsrc(bias ? bias + n0 : p.A, bias ? uint64_t(rows_n) * 4u : 0);
    const __amdgpu_buffer_rsrc_t rsC = make_rsrc(p.C[seg] + m0 * p.ldc + n0, (uint64_t(rows_m - 1) * ldc + rows_n) * 4u);
    const int lrow0 = wm * T::WTM + l15;
    const int lcol0 = wn * T::WTN + 4 * hi;
    auto load4 = [&](__amdgpu_buffer_rsrc_t rs, unsigned off, int lcol) -> float4 {   // off in floats; lcol: first column
        if constexpr (VEC) return bload4(rs, lcol < rows_n ? off * 4u : OOB, 0);
        float4 v;
        v.x = bload1(rs, lcol + 0 < rows_n ? (off + 0) * 4u : OOB);
        v.y = bload1(rs, lcol + 1 < rows_n ? (off + 1) * 4u : OOB);
        v.z = bload1(rs, lcol + 2 < rows_n ? (off + 2) * 4u : OOB);
        v.w = bload1(rs, lcol + 3 < rows_n ? (off + 3) * 4u : OOB);
        return v;
    };
#pragma unroll
    for (int i = 0; i < T::MI; ++i) {
        const int lrow = lrow0 + i * 16;
        // gathered residual: this lane's row's table rows (a row past the tile's rows reads table row 0: its stores are dropped)
        const float* ge = nullptr;
        const float* gp = nullptr;
        if constexpr (RGATHER) {
            const bool in = lrow < rows_m;
            const int tk = in ? p.rg_tok[m0 + lrow] : 0, ps = (in && p.rg_pos_table) ? p.rg_pos[m0 + lrow] : 0;
            ge = p.rg_emb + int64_t(tk) * p.N + n0;
            gp = p.rg_pos_table ? p.rg_pos_table + int64_t(ps) * p.N + n0 : nullptr;
        }
#pragma unroll
        for (int j = 0; j < T::NI; ++j) {
            const int lcol = lcol0 + j * 16;
            const float4 bv = load4(rsBias, unsigned(lcol), lcol);
            float4 v = make_float4(acc[i][j][0] + bv.x, acc[i][j][1] + bv.y, acc[i][j][2] + bv.z, acc[i][j][3] + bv.w);
            if (p.relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
            if (has_r) {
                float4 res = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (RGATHER) {
                    if (lcol < rows_n) {   // emb[tok][col] (+ pos[p][col]): the add the gather kernel would have done
                        res = *reinterpret_cast<const float4*>(ge + lcol);
                        if (gp) {
                            const float4 w = *reinterpret_cast<const float4*>(gp + lcol);
                            res.x += w.x; res.y += w.y; res.z += w.z; res.w += w.w;
                        }
                    }
                } else {
                    res = load4(rsR, unsigned(lrow * ldr + lcol), lcol);
                }
                v = make_float4(v.x + res.x, v.y + res.y, v.z + res.z, v.w + res.w);
            }
            const unsigned off = unsigned(lrow * ldc + lcol);
            if constexpr (VEC) {
                bstore4(rsC, lcol < rows_n ? off * 4u : OOB, v);
            } else {
                bstore1(rsC, lcol + 0 < rows_n ? (off + 0) * 4u : OOB, v.x);
                bstore1(rsC, lcol + 1 < rows_n ? (off + 1) * 4u : OOB, v.y);
                bstore1(rsC, lcol + 2 < rows_n ? (off + 2) * 4u : OOB, v.z);
                bstore1(rsC, lcol + 3 < rows_n ? (off + 3) * 4u : OOB, v.w);
            }
        }
    }
}

template <int BM, int BN, int WAVES_M, int WAVES_N, int NPLANE, bool VEC, bool RGATHER>
int launch_split2(const GemmParams& p, hipStream_t s) {
    using T = SplitTile<BM, BN, WAVES_M, WAVES_N, NPLANE>;
    // 32-bit in-tile byte offsets
    const int64_t ldmax = p.lda > p.ldw ? (p.lda > p.ldc ? p.lda : p.ldc) : (p.ldw > p.ldc ? p.ldw : p.ldc);
    if (ldmax * (BM > BN ? BM : BN) * 4 >= 0x7fffffffLL || (p.R && p.ldr * BM * 4 >= 0x7fffffffLL)) return LAMP_E_UNSUPPORTED;
    const int64_t tiles_m = (p.M + BM - 1) / BM;
    const int tiles_n_seg = (p.N + BN - 1) / BN;
    const int tiles_n = tiles_n_seg * p.nseg;
    const int64_t nwg = tiles_m * tiles_n;
    if (nwg > 0x7fffffffLL) return LAMP_E_DIMS;
    hipLaunchKernelGGL((gemm_split_kernel<BM, BN, WAVES_M, WAVES_N, NPLANE, VEC, RGATHER>), dim3((unsigned)nwg), dim3(T::NT), 0, s, p,
                       tiles_n_seg, tiles_n, int(tiles_m));
    return int(hipGetLastError());
}

template <int BM, int BN, int WAVES_M, int WAVES_N, int NPLANE>
int launch_split(const GemmParams& p, hipStream_t s) {
    if (p.rg_tok) {
        if (!p.vec_epilogue) return LAMP_E_UNSUPPORTED;   // the caller's rule: gemm_gathered_residual_ok
        return launch_split2<BM, BN, WAVES_M, WAVES_N, NPLANE, true, true>(p, s);
    }
    if (p.vec_epilogue) return launch_split2<BM, BN, WAVES_M, WAVES_N, NPLANE, true, false>(p, s);
    return launch_split2<BM, BN, WAVES_M, WAVES_N, NPLANE, false, false>(p, s);
}

// Tile choice from the launch's shape only (never a result bit, see the head of the file): the largest tile that still gives every
// CU (256) two workgroups, since the largest tile moves the fewest operand bytes per product; below that, the small tile, which puts
// the most waves on a short launch (the decoder's M = B * L row counts).
template <int NPLANE>
int launch_menu(const GemmParams& p, hipStream_t s) {
    auto tiles = [&](int bm, int bn) { return ((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn) * p.nseg; };
    if (tiles(128, 128) >= 512) return launch_split<128, 128, 2, 4, NPLANE>(p, s);   // 8 waves of 64x32: 4x2 blocks
    if (tiles(64, 64) >= 512) return launch_split<64, 64, 2, 2, NPLANE>(p, s);       // waves 32x32: 2x2 blocks
    return launch_split<32, 64, 1, 4, NPLANE>(p, s);                                 // waves 32x16: 2x1 blocks
}

}  // namespace

int launch_gemm_split(const GemmParams& p_in, int nprod, hipStream_t s) {
    GemmParams p = p_in;
    if (nprod != 3 && nprod != 6) return LAMP_E_UNSUPPORTED;
    if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.nseg < 1 || p.nseg > GEMM_MAX_SEG) return LAMP_E_DIMS;
    if ((p.K & 3) || (p.lda & 3) || (p.ldw & 3)) return LAMP_E_ALIGN;
    if (!p.A || (p.A_dense && !p.m_dev)) return LAMP_E_NULL;
    if (p.rg_tok && (p.R || !p.rg_emb || p.nseg != 1 || (p.rg_pos_table && !p.rg_pos))) return LAMP_E_UNSUPPORTED;
    if (p.rg_tok && (!aligned16(p.rg_emb) || (p.rg_pos_table && !aligned16(p.rg_pos_table)))) return LAMP_E_ALIGN;
    if (!aligned16(p.A) || (p.A_dense && !aligned16(p.A_dense))) return LAMP_E_ALIGN;
    for (int i = 0; i < p.nseg; ++i) {
        if (!p.W[i] || !p.C[i]) return LAMP_E_NULL;
        if (!aligned16(p.W[i])) return LAMP_E_ALIGN;
    }
    // the algorithmic FLOPs of the product, as the fp32 launch counts them (not x nprod)
    const double flops = 2.0 * double(p.M) * p.N * p.nseg * p.K;
    const double bytes = 4.0 * (double(p.M) * p.K + double(p.N) * p.nseg * p.K +
                                double(p.M) * p.N * p.nseg * ((p.R || p.rg_tok) ? 2 : 1));
    ProfScope prof(LAMP_K_GEMM, flops, bytes, s);
    p.trace = nullptr;
    p.walk_gn = 0;
    bool vec = !(p.N & 3) && !(p.ldc & 3) && (!p.R || (!(p.ldr & 3) && aligned16(p.R)));
    for (int i = 0; i < p.nseg; ++i) vec = vec && aligned16(p.C[i]) && (!p.bias[i] || aligned16(p.bias[i]));
    p.vec_epilogue = vec ? 1 : 0;
    return nprod == 3 ? launch_menu<2>(p, s) : launch_menu<3>(p, s);
}

}  // namespace lamp

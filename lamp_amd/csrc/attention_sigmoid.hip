// Fused masked SIGMOID attention  O = sigmoid(mask(Q K^T * inv_temperature)) V  in exact fp32 on v_mfma_f32_16x16x4_f32
// (reference: lamp/SubLayers.py:17-25,39 -- ScaledDotProductAttention(attn_type='sigmoid'): nn.Sigmoid() on the masked scores,
// blocked entries at sigmoid(-inf) = 0, NO row normalisation).  One kernel for every shape with d_k, d_v <= 128.
//
// No key is coupled to another: no running maximum, no rescale, no log-sum-exp.  A row without one allowed key is 0 (not NaN),
// a key split is a plain sum, and the maps come out of the same single pass (no lse, no normalising launch).
//
// Work decomposition (attention_small.hip's, simplified; the code the kernels share is attn16_frag.h): a wave owns ONE
// 16-query block and a share of its 16-key tiles; a
// workgroup is always four waves = 4 / ksplit query blocks x ksplit key shares (ksplit is a launch argument, not a template axis:
// 3 head widths x 4 mask kinds = 12 instantiations).  Both products are TRANSPOSED, so the query sits on the lane (column =
// lane & 15) in both accumulators and register r of S^T (key 4 * (lane >> 4) + r of the tile) is directly the B operand of PV
// step r.  The Q block (pre-scaled by log2(e) / temperature) sits in LDS; a wave's K tile is fetched with coalesced, range-checked
// buffer loads one tile ahead (compiler-tracked: no hand-counted waits) and staged through a wave-private LDS block; V goes
// straight to registers.  p = rcp(1 + exp2(-s)) on the hardware transcendentals, then SELECTED to exactly 0 for blocked keys and
// keys past the sample's extent.  The key shares' partial O^T are added by the first share in share order through LDS.
//
// Bits: the key split is a function of the sample's own key count (kv_len[b], else lk) -- never of B -- and under
// LAMP_MASK_SELF_RAGGED without per-sample key counts it is 1, so that neither lq nor lk enters.  Tiles past a sample's last
// key add exact zeros to accumulators that are never -0.0 (p >= 0, accumulators start at +0).
#include "attn16_frag.h"

namespace lamp {

namespace {

constexpr int SG_WAVES = 4;

template <int DP, int MK>
__global__ __launch_bounds__(SG_WAVES * 64, 2) void attn_sigmoid_kernel(AttnParams p, int ksplit) {
    constexpr int DKC = DP / 16;   // 16-wide k chunks of the QK^T product (one b128 fragment each)
    constexpr int DV8 = DP / 16;   // floats of a V row per lane = number of 16-row blocks of O^T
    constexpr int QS = DP + ATTN16_PAD;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int QB = SG_WAVES / ksplit;
    const int qb = wave / ksplit, ks = wave % ksplit;   // wave-uniform
    const int nqg = (p.lq + 16 * QB - 1) / (16 * QB);
    const int item = xcd_remap(blockIdx.x, gridDim.x);  // the query groups of one (sample, head) stay on one XCD
    const int qgrp = item % nqg;
    const int bh = item / nqg;
    const int h = bh % p.H, b = bh / p.H;
    const int q0 = (qgrp * QB + qb) * 16;
    const int qi = q0 + l15;
    const bool wave_active = q0 < p.lq;
    const int qc = qi < p.lq ? qi : p.lq - 1;
    const bool has_v = p.V != nullptr;   // false: maps only

    const int q_r = int(p.lay.q_r), k_r = int(p.lay.k_r), v_r = int(p.lay.v_r);
    // this sample's keys: all lk, or (ragged batches) its own count and its first row in the packed K / V matrices.  The
    // descriptors end at the sample's last key: rows past it read as zeros.
    const int lk_b = __builtin_amdgcn_readfirstlane(p.kv_len ? p.kv_len[b] : p.lk);
    const int row0 = __builtin_amdgcn_readfirstlane(p.kv_len ? p.kv_off[b] : 0);
    const int64_t k_row0 = p.kv_len ? int64_t(row0) * k_r : int64_t(b) * p.lay.k_b;
    const int64_t v_row0 = p.kv_len ? int64_t(row0) * v_r : int64_t(b) * p.lay.v_b;
    const __amdgpu_buffer_rsrc_t rsQ = make_rsrc(p.Q + int64_t(b) * p.lay.q_b + int64_t(h) * p.lay.q_h,
                                                 (uint64_t(p.lq - 1) * q_r + p.dk) * 4u);
    const __amdgpu_buffer_rsrc_t rsK = attn16_rsrc_rows(p.K + k_row0 + int64_t(h) * p.lay.k_h, lk_b, k_r, p.dk);
    const __amdgpu_buffer_rsrc_t rsV =
        attn16_rsrc_rows(has_v ? p.V + v_row0 + int64_t(h) * p.lay.v_h : p.K, lk_b, v_r, p.dv, has_v);
    const __amdgpu_buffer_rsrc_t rsM =
        MK == LAMP_MASK_BITS_U32
            ? make_rsrc(static_cast<const unsigned*>(p.mask) + int64_t(b) * p.m_sb,
                        (uint64_t(p.lq - 1) * uint64_t(p.m_sq) + (p.lk + 31) / 32) * 4u)
        : MK == LAMP_MASK_U8
            ? make_rsrc(static_cast<const unsigned char*>(p.mask) + int64_t(b) * p.m_sb,
                        uint64_t(p.lq - 1) * uint64_t(p.m_sq) + p.lk)
        : MK == LAMP_MASK_KEY_TOKENS_I64
            ? make_rsrc(static_cast<const long long*>(p.mask) + int64_t(b) * p.m_sb, uint64_t(p.lk) * 8u)
            : make_rsrc(p.K, 0);

    // ---- Q block -> LDS (pre-scaled); the ksplit waves of a block share the copy work ----
    float* Qs = smem + qb * 16 * QS;
    float* Ks = smem + (QB + wave) * 16 * QS;   // this wave's K tile
    {
        constexpr int C4 = DP / 4;
        const int per_wave = 16 * C4 / ksplit;   // float4 per wave
        for (int i = lane; i < per_wave; i += 64) {
            const int idx = ks * per_wave + i;
            const int row = idx / C4, c = (idx - row * C4) * 4;
            const int q = q0 + row;
            const float4 v = bload4(rsQ, (q < p.lq && c < p.dk) ? unsigned(q * q_r + c) * 4u : OOB, 0);
            *reinterpret_cast<float4*>(Qs + row * QS + c) =
                make_float4(v.x * p.scale_log2e, v.y * p.scale_log2e, v.z * p.scale_log2e, v.w * p.scale_log2e);
        }
    }
    __syncthreads();

    // 16-key tiles to visit.  With the map write-out every column of the map row has to be produced: all tiles of the padded
    // length, and no tile list.  Otherwise the sample's own tiles, or -- shared masks with a tile list (per 32-query block, 32-key
    // tiles) -- only the listed ones: a skipped tile holds blocked pairs only, i.e. probabilities of exactly 0.
    const int nt_b = (lk_b + 15) / 16;
    const int nt = p.P ? (p.lk + 15) / 16 : nt_b;
    const int* tl = (p.tiles && !p.P) ? p.tiles + int64_t(q0 >> 5) * p.tiles_stride : nullptr;   // wave-uniform
    const int n_idx = tl ? 2 * tl[0] : nt;
    auto tile_at = [&](int idx) { return idx < n_idx ? (tl ? 2 * tl[1 + (idx >> 1)] + (idx & 1) : idx) : nt; };   // nt: past the end
    // key shares in use: what the launcher would choose for THIS sample's key count (<= ksplit, sized for the padded length)
    const int shares = attn16_key_shares(nt_b);
    const int ks_eff = shares < ksplit ? shares : ksplit;

    float4 kg[DKC];        // the NEXT tile's K rows in flight (coalesced: row = i * RPI + lane / C4K, float4 lane % C4K)
    constexpr int C4K = DP / 4, RPI = 64 / C4K;
    float vf[4][DV8];      // V[kt*16 + 4g + r][.]: block e of O^T holds the d_v columns given at the store below
    unsigned mbits = 0;    // bit r = key (kt*16 + 4g + r) is blocked for this lane's query (one tile ahead)

    const unsigned k_voff = (lane % C4K) * 4 < p.dk ? unsigned((lane / C4K) * k_r + (lane % C4K) * 4) * 4u : OOB;
    auto load_k = [&](int kt) {
#pragma unroll
        for (int i = 0; i < DKC; ++i) kg[i] = bload4(rsK, k_voff, unsigned((kt * 16 + i * RPI) * k_r) * 4u);
    };
    auto stage_k = [&]() {   // registers -> this wave's LDS block (its reads of the previous tile are behind us: in order)
        const int c = (lane % C4K) * 4;
#pragma unroll
        for (int i = 0; i < DKC; ++i) *reinterpret_cast<float4*>(Ks + (i * RPI + lane / C4K) * QS + c) = kg[i];
    };
    constexpr int DVW = DV8 == 8 ? 4 : DV8;
    const unsigned v_voff = DVW * l15 < p.dv ? unsigned(4 * g * v_r + DVW * l15) * 4u : OOB;
    const unsigned v_voff2 = 64 + DVW * l15 < p.dv ? unsigned(4 * g * v_r + DVW * l15) * 4u + 256u : OOB;
    auto load_v = [&](int kt) { attn16_load_v<DP>(vf, rsV, v_voff, v_voff2, kt, v_r); };
    const unsigned m_voff = unsigned(int64_t(qc) * p.m_sq) * 4u;
    auto load_mask = [&](int kt) {
        const int kbase = kt * 16 + 4 * g;
        if constexpr (MK == LAMP_MASK_BITS_U32) {
            // the row's mask word (two tiles per word; past the row: 0); the lane group's four bits are taken in blocked_bits()
            mbits = __builtin_amdgcn_raw_buffer_load_b32(rsM, kt < nt ? m_voff : OOB, unsigned(kt >> 1) * 4u, 0);
        } else if constexpr (MK == LAMP_MASK_U8) {
            const unsigned mo = unsigned(int64_t(qc) * p.m_sq) + unsigned(kbase);
            unsigned m = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) m |= (bload_u8(rsM, (kt < nt && kbase + r < p.lk) ? mo + r : OOB) != 0 ? 1u : 0u) << r;
            mbits = m;
        } else if constexpr (MK == LAMP_MASK_KEY_TOKENS_I64) {
            unsigned m = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r)  // past lk: reads 0 == PAD == blocked (selected to 0 below anyway)
                m |= (bload_u64(rsM, kt < nt ? unsigned(kbase + r) * 8u : OOB) == 0 ? 1u : 0u) << r;
            mbits = m;
        }
    };
    // this lane's four blocked bits of tile kt: the mask's, and the keys past the sample's last key
    auto blocked_bits = [&](int kt) -> unsigned {
        const int valid = lk_b - kt * 16;
        const unsigned tail = valid >= 16 ? 0u : (0xffffu << (valid > 0 ? valid : 0)) & 0xffffu;   // scalar
        unsigned word = tail;
        if constexpr (MK == LAMP_MASK_BITS_U32) word |= mbits >> ((kt & 1) * 16);
        if constexpr (MK == LAMP_MASK_BITS_U32 || MK == LAMP_MASK_NONE) return (word >> (4 * g)) & 0xfu;
        return (mbits | (tail >> (4 * g))) & 0xfu;
    };
    auto scores = [&](f32x4& s) { attn16_scores<DP>(Qs, Ks, l15, g, f32x4{0.f, 0.f, 0.f, 0.f}, s); };

    f32x4 o[DV8];
#pragma unroll
    for (int e = 0; e < DV8; ++e) o[e] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (wave_active && ks < ks_eff && ks < n_idx) {
        float* Prow = p.P ? p.P + (int64_t(h) * p.P_batch + p.P_b0 + b) * int64_t(p.lq) * p.lk + int64_t(qc) * p.lk : nullptr;
        int kt = tile_at(ks);
        load_k(kt);
        load_mask(kt);
        if (has_v) load_v(kt);
        for (int idx = ks; idx < n_idx; idx += ks_eff) {
            const int kn = tile_at(idx + ks_eff);   // past the end: range-checked zeros
            f32x4 s;
            stage_k();       // the tile requested one iteration ago: registers -> LDS, read back as fragments by scores()
            scores(s);
            const unsigned blk = blocked_bits(kt);
            // pin the order "MFMAs of this tile, THEN the next tile's loads into the registers they just freed"
            __builtin_amdgcn_sched_barrier(0);
            load_k(kn);      // flies under the sigmoid + PV
            load_mask(kn);
            // s is in the log2 domain (Q pre-scaled by log2 e / temperature): sigmoid = 1 / (1 + 2^-s).  exp2 overflows to +inf
            // for s < -128 (rcp -> 0) and flushes to 0 for s > 126 (rcp -> 1); blocked keys are SELECTED to exactly 0.
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pr = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-s[r]));
                s[r] = (blk >> r) & 1u ? 0.f : pr;
            }
            if (Prow) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kt * 16 + 4 * g + r;
                    if (qi < p.lq && key < p.lk) Prow[key] = s[r];
                }
            }
            if (has_v) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int e = 0; e < DV8; ++e)
                        o[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[r][e], s[r], o[e], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                load_v(kn);      // flies under the next QK^T
            }
            kt = kn;
        }
    }
    if (!has_v) return;   // maps only (kernel-uniform)

    if (ksplit > 1) {
        // ---- add the key shares' partial results (lane-local positions, share order) ----
        constexpr int CW = DV8 * 4 * 64;   // floats per wave: the o blocks as float4 per lane
        __syncthreads();                   // every wave is done with its Q block and K tile: the region is reused
        float* mine = smem + wave * CW;
#pragma unroll
        for (int e = 0; e < DV8; ++e)
            *reinterpret_cast<float4*>(mine + (e * 64 + lane) * 4) = make_float4(o[e][0], o[e][1], o[e][2], o[e][3]);
        __syncthreads();
        if (ks == 0 && wave_active) {
            for (int s2 = 1; s2 < ks_eff; ++s2) {
                const float* other = smem + (wave + s2) * CW;
#pragma unroll
                for (int e = 0; e < DV8; ++e) {
                    const float4 v = *reinterpret_cast<const float4*>(other + (e * 64 + lane) * 4);
                    o[e][0] += v.x; o[e][1] += v.y; o[e][2] += v.z; o[e][3] += v.w;
                }
            }
        }
    }
    if (!(wave_active && ks == 0) || qi >= p.lq) return;

    // ---- store: lane (query, g), register r, block e  <->  O[query][DVW*(4g + r) + (e % DVW) + 64*(e / DVW)] ----
    float* Orow = p.O + int64_t(b) * p.lay.o_b + int64_t(h) * p.lay.o_h + int64_t(qi) * p.lay.o_r;
    const bool vec = ((p.lay.o_b | p.lay.o_h | p.lay.o_r) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.O) & 15u) == 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int e0 = 0; e0 < DV8; e0 += DVW) {
            const int col = DVW * (4 * g + r) + 64 * (e0 / DVW);
            if (col >= p.dv) continue;
            if (DVW == 4 && vec) {
                *reinterpret_cast<float4*>(Orow + col) = make_float4(o[e0][r], o[e0 + (DVW > 1 ? 1 : 0)][r],
                                                                     o[e0 + (DVW > 2 ? 2 : 0)][r], o[e0 + (DVW > 3 ? 3 : 0)][r]);
            } else {
#pragma unroll
                for (int e = 0; e < DVW; ++e) Orow[col + e] = o[e0 + e][r];
            }
        }
    }
}

template <int DP, int MK>
int launch_sigmoid_mk(const AttnParams& p, int ksplit, hipStream_t s) {
    const int QB = SG_WAVES / ksplit;   // Q blocks + one K tile per wave (>= the merge)
    return attn16_launch<attn_sigmoid_kernel<DP, MK>, attn16_lds_bytes(SG_WAVES, SG_WAVES, DP, DP / 16)>(
        p, QB, SG_WAVES, attn16_lds_bytes(QB, SG_WAVES, DP, ksplit > 1 ? DP / 16 : 0), s, ksplit);
}

template <int DP>
int launch_sigmoid_dp(const AttnParams& p, int ksplit, hipStream_t s) {
    switch (p.mask_kind) {
        case LAMP_MASK_U8: return launch_sigmoid_mk<DP, LAMP_MASK_U8>(p, ksplit, s);
        case LAMP_MASK_KEY_TOKENS_I64: return launch_sigmoid_mk<DP, LAMP_MASK_KEY_TOKENS_I64>(p, ksplit, s);
        case LAMP_MASK_BITS_U32: return launch_sigmoid_mk<DP, LAMP_MASK_BITS_U32>(p, ksplit, s);
        default: return launch_sigmoid_mk<DP, LAMP_MASK_NONE>(p, ksplit, s);
    }
}

}  // namespace

// Called by launch_attn (attention.hip) behind its argument checks, for AttnParams::act == LAMP_ATTN_SIGMOID and d_k, d_v <= 128.
int launch_attn_sigmoid(const AttnParams& p, hipStream_t s) {
    if (p.tiles && (p.m_sb != 0 || (p.mask_kind != LAMP_MASK_U8 && p.mask_kind != LAMP_MASK_BITS_U32)))
        return LAMP_E_UNSUPPORTED;  // the sparsity hint belongs to shared masks
    // Key shares from the (padded) key count; the kernel lowers them per sample from kv_len[b].  Padded self-attention without
    // per-sample key counts: lk is only the padded length, and a split chosen from it would tie a sample's bits to its batch.
    int ksplit = attn16_key_shares((p.lk + 15) / 16);
    if (p.self_ragged && !p.kv_len) ksplit = 1;
    const int dmax = p.dk > p.dv ? p.dk : p.dv;
    if (dmax <= 32) return launch_sigmoid_dp<32>(p, ksplit, s);
    if (dmax <= 64) return launch_sigmoid_dp<64>(p, ksplit, s);
    return launch_sigmoid_dp<128>(p, ksplit, s);
}

}  // namespace lamp

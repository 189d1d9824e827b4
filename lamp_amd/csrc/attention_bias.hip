// Fused BIASED softmax attention  O = softmax_k(Q K^T * inv_temperature + bias[q][k]) V  in exact fp32 on v_mfma_f32_16x16x4_f32:
// the weighted label graph (lamp_mask kind LAMP_MASK_BIAS_F32).  softmax(s + log w) = w exp(s) / sum w exp(s): a bias of log w
// re-weights the label -> label attention by w, a bias of -inf is the reference's mask (lamp/Decoders.py:140-147), and a row
// whose entries are all -inf comes out NaN as masked_fill + softmax gives.  One kernel for every shape with
// d_k, d_v <= 128; heads share the bias, samples share it (stride_b == 0) or bring their own.
//
// Work decomposition and operand paths are attention_sigmoid.hip's (the code the kernels share is attn16_frag.h): a wave
// owns ONE 16-query block and a share of its 16-key
// tiles, a workgroup is four waves = 4 / ksplit query blocks x ksplit key shares (ksplit is a launch argument), both products
// are TRANSPOSED (query on the lane = lane & 15, register r of S^T = key 4 * (lane >> 4) + r of the tile = B operand of PV step
// r), the Q block sits in LDS pre-scaled by log2(e) / temperature, K tiles are fetched one tile ahead with range-checked buffer
// loads and staged through a wave-private LDS block, V goes straight to registers, waits are compiler-tracked.  The lane's four
// bias values of a tile are ONE 16-byte load (rows are ld floats apart, ld % 4 == 0), one tile ahead like K.
//
// What softmax adds is attention_small.hip's online form on the same fragments: running maximum (equal in a query's four lane
// groups), lazy rescale, per-group partial row sums.  Everything is in the exp2 domain: the bias is multiplied by log2(e) when
// it is added (-inf stays -inf), blocked scores are exactly -inf, and every maximum that is subtracted is replaced by 0 while it
// still is -inf, so that inf - inf never happens: a tile whose 16 keys are all blocked for a query adds exp2(-inf) = 0 to its sum
// and leaves its maximum and accumulators as they were.  Keys past lk count as blocked.
//
// PM = 0: O only.  PM = 2 (training forward): additionally the scaled, biased scores (log2 domain) into the map buffer and each
// row's log2-sum-exp into lse; softmax_from_scores_kernel (attention.hip) then normalises in place.  PM = 1 (maps without lse):
// exactly normalised maps in two passes of one unsplit wave -- row maximum and sum first, then P = exp2(s - m) / l written once
// and, with V, multiplied into O as it is.
//
// Bits: the key split is a function of lk alone (never of B), partial results combine in share order through LDS.
#include "attn16_frag.h"

namespace lamp {

namespace {

constexpr int BS_WAVES = 4;
constexpr float BS_LOG2E = 1.4426950408889634f;

template <int DP, int PM>
__global__ __launch_bounds__(BS_WAVES * 64, 2) void attn_bias_kernel(AttnParams p, int ksplit) {
    constexpr int DKC = DP / 16;   // 16-wide k chunks of the QK^T product (one b128 fragment each)
    constexpr int DV8 = DP / 16;   // floats of a V row per lane = number of 16-row blocks of O^T
    constexpr int QS = DP + ATTN16_PAD;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int QB = BS_WAVES / ksplit;
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
    const bool has_v = p.V != nullptr;   // false (PM == 1 only): maps only

    const int q_r = int(p.lay.q_r), k_r = int(p.lay.k_r), v_r = int(p.lay.v_r);
    const __amdgpu_buffer_rsrc_t rsQ = make_rsrc(p.Q + int64_t(b) * p.lay.q_b + int64_t(h) * p.lay.q_h,
                                                 (uint64_t(p.lq - 1) * q_r + p.dk) * 4u);
    const __amdgpu_buffer_rsrc_t rsK = make_rsrc(p.K + int64_t(b) * p.lay.k_b + int64_t(h) * p.lay.k_h,
                                                 (uint64_t(p.lk - 1) * k_r + p.dk) * 4u);
    const __amdgpu_buffer_rsrc_t rsV = make_rsrc(has_v ? p.V + int64_t(b) * p.lay.v_b + int64_t(h) * p.lay.v_h : p.K,
                                                 has_v ? (uint64_t(p.lk - 1) * v_r + p.dv) * 4u : 0);
    // bias rows are m_sq floats apart and read in whole 16-byte groups: the last group of a row may reach past lk (inside the
    // row's padding, launch_attn checked m_sq % 4 == 0); what it holds there is never used (keys past lk are blocked)
    const __amdgpu_buffer_rsrc_t rsB = make_rsrc(static_cast<const float*>(p.mask) + int64_t(b) * p.m_sb,
                                                 (uint64_t(p.lq - 1) * uint64_t(p.m_sq) + uint64_t((p.lk + 3) & ~3)) * 4u);

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

    const int nt = (p.lk + 15) / 16;   // every tile is visited: a bias has no tile list

    float4 kg[DKC];        // the NEXT tile's K rows in flight (coalesced: row = i * RPI + lane / C4K, float4 lane % C4K)
    constexpr int C4K = DP / 4, RPI = 64 / C4K;
    float vf[4][DV8];      // V[kt*16 + 4g + r][.]: block e of O^T holds the d_v columns given at the store below
    float4 bg = make_float4(0.f, 0.f, 0.f, 0.f);   // bias[query][kt*16 + 4g + r], one tile ahead

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
    const unsigned b_voff = unsigned(int64_t(qc) * p.m_sq + 4 * g) * 4u;
    auto load_bias = [&](int kt) {   // past the last tile / the row's last group: zeros (those keys are blocked below anyway)
        bg = bload4(rsB, (kt < nt && kt * 16 + 4 * g < p.lk) ? b_voff + unsigned(kt) * 64u : OOB, 0);
    };
    auto scores = [&](f32x4& s) { attn16_scores<DP>(Qs, Ks, l15, g, f32x4{0.f, 0.f, 0.f, 0.f}, s); };
    // the tile's scaled scores plus bias * log2(e), -inf for the keys past lk (bg is consumed: the next tile's may be requested)
    auto add_bias = [&](int kt, f32x4& s) {
        const int kbase = kt * 16 + 4 * g;
        const float bb[4] = {bg.x, bg.y, bg.z, bg.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = kbase + r < p.lk ? fmaf(bb[r], BS_LOG2E, s[r]) : -INFINITY;
    };

    f32x4 o[DV8];
#pragma unroll
    for (int e = 0; e < DV8; ++e) o[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_part = 0.f;   // m_run: this query's running maximum (equal in its 4 lane groups)
    constexpr float RESCALE_THR = 32.0f;
    const bool working = wave_active && ks < nt;
    float* Prow = (PM != 0 && p.P) ? p.P + (int64_t(h) * p.P_batch + p.P_b0 + b) * int64_t(p.lq) * p.lk + int64_t(qc) * p.lk
                                   : nullptr;

    if constexpr (PM == 1) {
        // ---- pass 1 (unsplit): the row's exact maximum and sum ----
        if (working) {
            load_k(0);
            load_bias(0);
            for (int kt = 0; kt < nt; ++kt) {
                f32x4 s;
                stage_k();
                scores(s);
                __builtin_amdgcn_sched_barrier(0);
                load_k(kt + 1);
                add_bias(kt, s);
                load_bias(kt + 1);
                const float tmax = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
                if (__any(tmax > m_run)) {
                    const float m_new = fmaxf(m_run, group_max(tmax));
                    l_part *= __builtin_amdgcn_exp2f(m_run - ((m_new == -INFINITY) ? 0.f : m_new));
                    m_run = m_new;
                }
                const float m_use = (m_run == -INFINITY) ? 0.f : m_run;
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] = __builtin_amdgcn_exp2f(s[r] - m_use);
                l_part += (s[0] + s[1]) + (s[2] + s[3]);
            }
        }
        const float inv_l = 1.0f / group_sum(l_part);   // l = 0 (fully blocked row): 0 * inf = NaN, like torch
        const float m_use = (m_run == -INFINITY) ? 0.f : m_run;
        // ---- pass 2: P = exp2(s - m) / l, written once and multiplied into O as it is ----
        if (working) {
            load_k(0);
            load_bias(0);
            if (has_v) load_v(0);
            for (int kt = 0; kt < nt; ++kt) {
                f32x4 s;
                stage_k();
                scores(s);
                __builtin_amdgcn_sched_barrier(0);
                load_k(kt + 1);
                add_bias(kt, s);
                load_bias(kt + 1);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[r] = __builtin_amdgcn_exp2f(s[r] - m_use) * inv_l;
                    const int key = kt * 16 + 4 * g + r;
                    if (qi < p.lq && key < p.lk) Prow[key] = s[r];
                }
                if (has_v) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int e = 0; e < DV8; ++e)
                            o[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[r][e], s[r], o[e], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    load_v(kt + 1);
                }
            }
        }
        if (!has_v) return;   // maps only (kernel-uniform)
    } else {
        if (working) {
            int kt = ks;
            load_k(kt);
            load_bias(kt);
            load_v(kt);
            for (; kt < nt; kt += ksplit) {
                const int kn = kt + ksplit;   // past the end: range-checked zeros
                f32x4 s;
                stage_k();       // the tile requested one iteration ago: registers -> LDS, read back as fragments by scores()
                scores(s);
                // pin the order "MFMAs of this tile, THEN the next tile's loads into the registers they just freed"
                __builtin_amdgcn_sched_barrier(0);
                load_k(kn);      // flies under softmax + PV
                add_bias(kt, s);
                load_bias(kn);
                if constexpr (PM == 2) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int key = kt * 16 + 4 * g + r;
                        if (qi < p.lq && key < p.lk) Prow[key] = s[r];
                    }
                }
                const float tmax = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
                if (__any(tmax > m_run + RESCALE_THR)) {
                    const float m_new = fmaxf(m_run, group_max(tmax));
                    const float alpha = __builtin_amdgcn_exp2f(m_run - ((m_new == -INFINITY) ? 0.f : m_new));
                    l_part *= alpha;
                    m_run = m_new;
#pragma unroll
                    for (int e = 0; e < DV8; ++e)
#pragma unroll
                        for (int r = 0; r < 4; ++r) o[e][r] *= alpha;
                }
                const float m_use = (m_run == -INFINITY) ? 0.f : m_run;
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] = __builtin_amdgcn_exp2f(s[r] - m_use);
                l_part += (s[0] + s[1]) + (s[2] + s[3]);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int e = 0; e < DV8; ++e)
                        o[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[r][e], s[r], o[e], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                load_v(kn);      // flies under the next QK^T
            }
        }

        if (ksplit > 1) {
            // ---- merge the key shares' partial results (lane-local positions, share order) ----
            constexpr int CW = (DV8 * 4 + 4) * 64;  // floats per wave: o blocks as float4 per lane, then (m, l, -, -) per lane
            __syncthreads();                        // every wave is done with its Q block and K tile: the region is reused
            float* mine = smem + wave * CW;
#pragma unroll
            for (int e = 0; e < DV8; ++e)
                *reinterpret_cast<float4*>(mine + (e * 64 + lane) * 4) = make_float4(o[e][0], o[e][1], o[e][2], o[e][3]);
            *reinterpret_cast<float4*>(mine + (DV8 * 64 + lane) * 4) = make_float4(m_run, l_part, 0.f, 0.f);
            __syncthreads();
            if (ks == 0 && wave_active) {
                float m_all = m_run;
                for (int s2 = 1; s2 < ksplit; ++s2) m_all = fmaxf(m_all, smem[(wave + s2) * CW + (DV8 * 64 + lane) * 4]);
                const float m_use = (m_all == -INFINITY) ? 0.f : m_all;
                const float w0 = exp2f(m_run - m_use);   // a share without one allowed key: exp2(-inf) = 0 on zeros
                l_part *= w0;
#pragma unroll
                for (int e = 0; e < DV8; ++e)
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[e][r] *= w0;
                for (int s2 = 1; s2 < ksplit; ++s2) {
                    const float* other = smem + (wave + s2) * CW;
                    const float4 ml = *reinterpret_cast<const float4*>(other + (DV8 * 64 + lane) * 4);
                    const float ws = exp2f(ml.x - m_use);
                    l_part = fmaf(ml.y, ws, l_part);
#pragma unroll
                    for (int e = 0; e < DV8; ++e) {
                        const float4 v = *reinterpret_cast<const float4*>(other + (e * 64 + lane) * 4);
                        o[e][0] = fmaf(v.x, ws, o[e][0]);
                        o[e][1] = fmaf(v.y, ws, o[e][1]);
                        o[e][2] = fmaf(v.z, ws, o[e][2]);
                        o[e][3] = fmaf(v.w, ws, o[e][3]);
                    }
                }
                m_run = m_all;
            }
        }
    }
    if (!(wave_active && ks == 0)) return;
    float inv_l = 1.0f;   // PM == 1: O was accumulated from normalised probabilities
    if constexpr (PM != 1) {
        const float l_run = group_sum(l_part);   // the four lane groups of a query hold disjoint keys
        if constexpr (PM == 2) {
            // row log2-sum-exp of the biased scores: probabilities = exp2(score - lse).  A fully blocked row has
            // l = 0 -> lse = -inf -> exp2(-inf - -inf) = NaN, as the reference's softmax gives.
            if (g == 0 && qi < p.lq)
                p.lse[(int64_t(h) * p.B + b) * int64_t(p.lq) + qi] = ((m_run == -INFINITY) ? 0.f : m_run) + log2f(l_run);
        }
        inv_l = 1.0f / l_run;   // l = 0 (fully blocked row): 0 * inf = NaN, like torch
    }
    if (qi >= p.lq) return;

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
                *reinterpret_cast<float4*>(Orow + col) =
                    make_float4(o[e0][r] * inv_l, o[e0 + (DVW > 1 ? 1 : 0)][r] * inv_l, o[e0 + (DVW > 2 ? 2 : 0)][r] * inv_l,
                                o[e0 + (DVW > 3 ? 3 : 0)][r] * inv_l);
            } else {
#pragma unroll
                for (int e = 0; e < DVW; ++e) Orow[col + e] = o[e0 + e][r] * inv_l;
            }
        }
    }
}

template <int DP, int PM>
int launch_bias_pm(const AttnParams& p, int ksplit, hipStream_t s) {
    const int QB = BS_WAVES / ksplit;
    constexpr int MERGE_F4 = DP / 16 + 1;   // a wave's merge record: its o blocks, then (m, l, -, -)
    return attn16_launch<attn_bias_kernel<DP, PM>, attn16_lds_bytes(BS_WAVES, BS_WAVES, DP, MERGE_F4)>(
        p, QB, BS_WAVES, attn16_lds_bytes(QB, BS_WAVES, DP, ksplit > 1 ? MERGE_F4 : 0), s, ksplit);
}

template <int DP>
int launch_bias_dp(const AttnParams& p, int ksplit, hipStream_t s) {
    if (p.P && p.lse) return launch_bias_pm<DP, 2>(p, ksplit, s);
    if (p.P) return launch_bias_pm<DP, 1>(p, 1, s);   // exact two-pass maps: one wave walks all of a row's keys
    return launch_bias_pm<DP, 0>(p, ksplit, s);
}

}  // namespace

// Called by launch_attn (attention.hip) behind its argument checks, for AttnParams::mask_kind == LAMP_MASK_BIAS_F32 and
// d_k, d_v <= 128 (softmax, no tile list, no ragged keys).
int launch_attn_bias(const AttnParams& p, hipStream_t s) {
    const int ksplit = attn16_key_shares((p.lk + 15) / 16);   // a function of lk alone
    const int dmax = p.dk > p.dv ? p.dk : p.dv;
    if (dmax <= 32) return launch_bias_dp<32>(p, ksplit, s);
    if (dmax <= 64) return launch_bias_dp<64>(p, ksplit, s);
    return launch_bias_dp<128>(p, ksplit, s);
}

}  // namespace lamp

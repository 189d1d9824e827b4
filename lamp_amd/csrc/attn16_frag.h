// The 16-query x 16-key fragment path shared by the three small-tile attention kernels: attn16_kernel (attention_small.hip,
// masked softmax), attn_sigmoid_kernel (attention_sigmoid.hip) and attn_bias_kernel (attention_bias.hip, biased softmax), all
// exact fp32 on v_mfma_f32_16x16x4_f32.  The kernels keep what is their own (masks, activation, bias, map write-out, the shape
// of their key loops).  Below is the one copy of what they have in common AND what hipcc compiles, called from here, to
// exactly the machine code of the same text written in place (tools/chain_isa_diff.py).  That is less than the kernels share in
// design: index decode, the Q / mask descriptors, Q staging, load_k / stage_k, the online-softmax tile update, the share
// merge and the O store all changed the register allocation or the schedule of some instantiation when they moved into
// functions, and stay written out in each kernel.
//
// Work decomposition.  A wave owns ONE 16-query block and a share of its 16-key tiles; a workgroup is QB query blocks x
// key shares (merged lane-locally through LDS at the end).  Both products are TRANSPOSED, so the query sits on the lane
// (column = lane & 15 = l15) in both accumulators, and register r of S^T (key 4 * g + r of the tile, g = lane >> 4) is directly
// the B operand of PV step r.  The Q block (16 x d_k, pre-scaled by log2(e) / temperature) sits in LDS and is re-read per key
// tile as b128 fragments.  A wave's K tile is fetched one tile ahead with coalesced, range-checked buffer loads (whole rows per
// instruction; compiler-tracked: no hand-counted waits) and staged through a wave-private LDS block; V goes straight to
// registers.  DP is the padded head width (32, 64 or 128): DP / 16 k chunks of QK^T, DP / 16 sixteen-row blocks of O^T.
//
// Loads of the key loop carry NO per-tile vector arithmetic (a vector instruction costs matrix-pipe time on gfx950,
// profiles/r05_mfma_chain.txt): the lane's offset inside a tile is a loop invariant with the head-dimension check folded in
// (OOB + anything < 2^31 stays out of range), the tile's / row's base rides in the SCALAR offset, which the descriptor's
// range check covers (tools/probes/lds_dma_oob.hip) -- rows past the sample's last key read as zeros without a test.
#pragma once
#include "lamp_kernels.h"

namespace lamp {

// LDS row padding of the Q block / K tiles: 8 floats.  With 4 (rounds 2-3) the sixteen lanes ds_read_b128 serves together
// -- rows 0-3 and 12-15 at one k-quad, rows 4-11 at the next (MI355X_MICROARCH.md, LDS lane groups) -- met two by two on a
// 16-byte slot: 29 % of the kernel's LDS cycles were bank conflicts (profiles/r02_attn_ta_pmc.txt); with 8 none do.
#ifndef LAMP_LDS_PAD16
#define LAMP_LDS_PAD16 8
#endif
constexpr int ATTN16_PAD = LAMP_LDS_PAD16;
// Key shares for nt sixteen-key tiles (measured, profiles/r02_attn_variants.txt): four from 12 tiles on (reuters enc-dec: 19),
// two from 4 (reuters' 90-label self-attention: 6; bibtex 7 / 10), else one.  The launchers size the workgroup with it from the
// (padded) key count; with ragged keys the kernels lower it per sample from the sample's own count.
// A macro under the function: attn16_kernel needs the rule with its compile-time share count as the cap, in place (through a
// function call hipcc orders that kernel's prologue differently).
#define ATTN16_KEY_SHARES(nt, cap) ((nt) >= 12 ? ((cap) < 4 ? (cap) : 4) : ((nt) >= 4 ? 2 : 1))
__host__ __device__ inline int attn16_key_shares(int nt) { return ATTN16_KEY_SHARES(nt, 4); }

// Exchange across the four lane groups of a query (lanes l, l^16, l^32, l^48) with gfx950's row-swap instructions instead
// of __shfl_xor (= ds_bpermute through the LDS crossbar, ~100 cycles a step):
//   v_permlane16_swap a, b  swaps the odd 16-lane rows of a with the even rows of b;  v_permlane32_swap a, b swaps the
//   upper half of a with the lower half of b.  Starting from a = b = v, a and b then hold the two partners of every lane.
// (Inline asm: the builtins return their second result equal to the first in hipcc 7.2 -- DESIGN.md 4.4.  Only used in
// the rescale branch and after the key loop, where the scheduling barrier an asm statement implies costs nothing.)
// The s_nop pairs: hipcc cannot see inside an asm statement, so the wait states it would insert between a VALU write and
// a permlane swap reading it (and between the swap and its consumers) are spelled out.
__device__ __forceinline__ void swap16(float& a, float& b) {
    asm volatile("s_nop 3\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 3" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void swap32(float& a, float& b) {
    asm volatile("s_nop 3\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 3" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float group_max(float v) {  // max over the 4 lane groups
    float a = v, b = v;
    swap16(a, b);
    a = fmaxf(a, b);
    b = a;
    swap32(a, b);
    return fmaxf(a, b);
}
__device__ __forceinline__ float group_sum(float v) {  // (v[l] + v[l^16]) + (v[l^32] + v[l^48]), the pairing of the xor butterfly
    float a = v, b = v;
    swap16(a, b);
    a = a + b;
    b = a;
    swap32(a, b);
    return a + b;
}

// ---- K / V descriptors ----
// `rows` rows of d floats, `stride` floats apart: the descriptor ends with the last row, so rows past it read as zeros
// (never another sample's, never NaNs); no rows, or a matrix that is not there (maps only: no V): an empty descriptor
__device__ __forceinline__ __amdgpu_buffer_rsrc_t attn16_rsrc_rows(const float* base, int rows, int stride, int d,
                                                                   bool present = true) {
    return make_rsrc(base, (present && rows > 0) ? (uint64_t(rows - 1) * stride + d) * 4u : 0);
}
// ---- V: straight to registers ----
// V columns of a lane: DVW consecutive floats per load, the 16 lanes of a group side by side (whole cache lines per
// row and instruction).  d = 128 takes two such loads 64 columns apart: block e of O^T then holds the d_v columns
// {4 i + e} (e < 4) and {64 + 4 i + e - 4} (e >= 4), i = the block's row index -- see the kernels' stores.
// vf[r][.] = V[kt * 16 + 4 g + r][the lane's columns]
template <int DP>
__device__ __forceinline__ void attn16_load_v(float (&vf)[4][DP / 16], __amdgpu_buffer_rsrc_t rsV, unsigned v_voff,
                                              unsigned v_voff2, int kt, int v_r) {
    constexpr int DV8 = DP / 16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned so = unsigned((kt * 16 + r) * v_r) * 4u;
        if constexpr (DV8 == 8) {
            const float4 a = bload4(rsV, v_voff, so);
            const float4 c2 = bload4(rsV, v_voff2, so);
            vf[r][0] = a.x; vf[r][1] = a.y; vf[r][2] = a.z; vf[r][3] = a.w;
            vf[r][4] = c2.x; vf[r][5] = c2.y; vf[r][6] = c2.z; vf[r][7] = c2.w;
        } else if constexpr (DV8 == 4) {
            const float4 a = bload4(rsV, v_voff, so);
            vf[r][0] = a.x; vf[r][1] = a.y; vf[r][2] = a.z; vf[r][3] = a.w;
        } else {
            const f32x2 a = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rsV, v_voff, so, 0));
            vf[r][0] = a.x; vf[r][1] = a.y;
        }
    }
}

// ---- the QK^T product ----
// S^T = K Q^T for the tile staged in Ks (two accumulator chains, summed: the dependent-issue latency of the 16x16x4 MFMA
// is 40 cycles against 32 of issue).  s0 is the first chain's initial value: zeros, or -inf for blocked keys.
template <int DP>
__device__ __forceinline__ void attn16_scores(const float* Qs, const float* Ks, int l15, int g, f32x4 s0, f32x4& s) {
    constexpr int QS = DP + ATTN16_PAD;
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f};
#ifdef LAMP_SETPRIO   // experiment (profiles/r04_setprio.txt): raised wave priority around the QK^T and PV MFMA runs
    __builtin_amdgcn_s_setprio(1);
#endif
    const float* qp = Qs + l15 * QS + 4 * g;   // lane (query l15, group g): Q[q][16c + 4g + j]
    const float* kp = Ks + l15 * QS + 4 * g;   // lane (key   l15, group g): K[k][16c + 4g + j]
#pragma unroll
    for (int c = 0; c < DP / 16; c += 2) {
        const float4 qa = *reinterpret_cast<const float4*>(qp + 16 * c);
        const float4 qb2 = *reinterpret_cast<const float4*>(qp + 16 * c + 16);
        const float4 ka = *reinterpret_cast<const float4*>(kp + 16 * c);
        const float4 kb = *reinterpret_cast<const float4*>(kp + 16 * c + 16);
        s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ka.x, qa.x, s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kb.x, qb2.x, s1, 0, 0, 0);
        s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ka.y, qa.y, s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kb.y, qb2.y, s1, 0, 0, 0);
        s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ka.z, qa.z, s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kb.z, qb2.z, s1, 0, 0, 0);
        s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ka.w, qa.w, s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kb.w, qb2.w, s1, 0, 0, 0);
    }
#ifdef LAMP_SETPRIO
    __builtin_amdgcn_s_setprio(0);
#endif
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = s0[r] + s1[r];
}
// ---- launch (host) ----
// Dynamic LDS of a workgroup of `waves` waves over qb query blocks: the Q blocks + one K tile per wave, or -- later, in the
// same region -- the merge records of merge_f4 float4 per lane (0: one key share, no merge), whichever is larger.
constexpr size_t attn16_lds_bytes(int qb, int waves, int dp, int merge_f4) {
    const size_t qk = size_t(qb + waves) * 16 * (dp + ATTN16_PAD) * sizeof(float);
    const size_t merge = size_t(waves) * merge_f4 * 4 * 64 * sizeof(float);
    return qk > merge ? qk : merge;
}
// One workgroup of `waves` waves per qb query blocks of every (sample, head), lds bytes of dynamic LDS; LDS_MAX = the most this
// instantiation is ever launched with (raised once per device where it is beyond the 64 KiB default).
template <auto KERN, size_t LDS_MAX, class... Extra>
int attn16_launch(const AttnParams& p, int qb, int waves, size_t lds, hipStream_t s, Extra... extra) {
    if constexpr (LDS_MAX > 65536) {
        static AttrOnce once;
        if (int e = once.set(reinterpret_cast<const void*>(KERN), LDS_MAX)) return e;
    }
    const int64_t nwg = int64_t((p.lq + 16 * qb - 1) / (16 * qb)) * p.H * p.B;
    if (nwg > 0x7fffffffLL) return LAMP_E_DIMS;
    hipLaunchKernelGGL(KERN, dim3(unsigned(nwg)), dim3(waves * 64), lds, s, p, extra...);
    return int(hipGetLastError());
}

}  // namespace lamp

// Row-split pair toolkit of the level-0 chain kernels (vv_chain.hip: chain_rs_c320_kernel, chain_front_rs_c320_kernel; design notes there).
// A block = 128 tokens = 8 waves = 4 token groups x 2 row halves behind one weight ring; the two waves of a pair (wave, pw = wave ^ 4) own the same
// 32 tokens and split every [64 x 64] slab by rows.  Everything here is a free function on the kernel's own locals; the kernels keep one-line lambdas
// that bind those locals.  The spellings are the ones that leave the device code of both kernels as it was (profiles/fused_shared_isa.txt): rs_sync
// calls the kernel's `issue` lambda, not rs_issue, and rs_swap_full / rs_layer_norm take even the wave ids BY REFERENCE, as a lambda captures them (by
// value, or with the ring state in a struct, instructions moved).
#pragma once
#include <type_traits>
#include "vv_fused_common.h"

constexpr int RS_NS = 10, RS_AH = 6, RS_SLAB = 8192, RS_XBUF = 40960;      // ring slots, slabs in flight, bytes per slab, pair-exchange buffer

using BODY = std::false_type; using TAIL = std::true_type;      // TAIL: the stream may run out of slabs to issue in this group
using NOX = std::false_type; using XCH = std::true_type;        // XCH: the step also publishes LDS writes of this wave
using NOPRE = std::false_type; using PRE = std::true_type;      // PRE: the caller has already made the group's first step
using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>; using I4 = std::integral_constant<int, 4>;
using N5 = std::integral_constant<int, 5>; using N10 = std::integral_constant<int, 10>; using N25 = std::integral_constant<int, 25>;

// ---- the weight ring: every wave copies 1 KB of every slab (sbase = stream + wave * 1024 + lane * 16)
__device__ __forceinline__ void rs_issue(const unsigned char* sbase, unsigned char* ring, const int wave, int& issued, int& islot) {
    glds16_asm(sbase + (int64_t)issued * RS_SLAB, ring + islot * RS_SLAB + wave * 1024);
    ++issued;
    islot = islot + 1 == RS_NS ? 0 : islot + 1;
}
// one synchronisation step in front of NI slabs: issue NI more, wait until all but the newest RS_AH have landed (this wave's share), meet.
// XCHG: LDS writes of this wave (an exchange) have to be complete before the barrier.  TOTAL: slabs in the kernel's stream.  issue(): the kernel's rs_issue.
template <int TOTAL, int NI, bool IS_TAIL, bool XCHG, typename ISSUE>
__device__ __forceinline__ void rs_sync(ISSUE&& issue, int& issued) {
    if constexpr (IS_TAIL) {
        if (issued + NI <= TOTAL) {
#pragma unroll
            for (int i = 0; i < NI; ++i) issue();
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        } else {
            while (issued < TOTAL) issue();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    } else {
#pragma unroll
        for (int i = 0; i < NI; ++i) issue();
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    }
    if constexpr (XCHG) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}
static_assert(RS_AH == 6, "rs_sync waits with vmcnt(6): one LDS-DMA per wave and slab, RS_AH slabs in flight");
__device__ __forceinline__ const unsigned char* rs_slab(const unsigned char* ring, int& cslot) {      // the consumed-slot walk
    const unsigned char* s = ring + cslot * RS_SLAB;
    cslot = cslot + 1 == RS_NS ? 0 : cslot + 1;
    return s;
}
__device__ __forceinline__ void rs_meet() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); }      // exchange-only barrier (no slab)

// ---- fragments
template <typename T>
__device__ __forceinline__ uint4 rs_frag(const f32x4& lo, const f32x4& hi) {
    return make_uint4(pack2<T>(lo[0], lo[1]), pack2<T>(lo[2], lo[3]), pack2<T>(hi[0], hi[1]), pack2<T>(hi[2], hi[3]));
}
__device__ __forceinline__ uint4 rs_sel(const bool hi, const uint4& a, const uint4& b) { return hi ? b : a; }      // wave-uniform select
// first of the 4 channels of trunk register t[j][.][0..3]: channel = 64 rb + 32 hf + 16 rt + 4 lg + r, j = 2 rb + rt
__device__ __forceinline__ int rs_chan(const int j, const int hf, const int lg) { return 64 * (j >> 1) + 32 * hf + 16 * (j & 1) + 4 * lg; }

// ---- row-split slab groups: this wave's two row tiles (2 hf, 2 hf + 1) of N [64 x 64] slabs
struct WF2 { uint4 w[2][2]; };      // [kk][rt]
__device__ __forceinline__ void rs_load(const unsigned char* s, const int rs_off /* hf * 4096 + li * 128 */, const int lg, const int sw /* li & 7 */, WF2& f) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int off = ((kk * 4 + lg) ^ sw) << 4;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) f.w[kk][rt] = *(const uint4*)(s + rs_off + rt * 2048 + off);
    }
}
template <typename T>
__device__ __forceinline__ void rs_fma(const WF2& f, f32x4* acc /* [2][2] = [rt][tt] */, const uint4 (&x0)[2], const uint4 (&x1)[2]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) acc[rt * 2 + tt] = T::mfma(f.w[kk][rt], kk ? x1[tt] : x0[tt], acc[rt * 2 + tt]);
}
// N slabs, a step in front of every pair: acc_of(i)[rt][tt] += own row tiles x (x0_of(i), x1_of(i)) = the two k steps of the activation row.
// sync(ni, tail, xch): the kernel's binding of rs_sync; next(f): fragments of the next slab of the ring, rs_load(rs_slab(..), .., f).
template <typename T, int N, bool IS_PRE, typename TAILT, typename SYNC, typename NEXT, typename ACC, typename X0, typename X1>
__device__ __forceinline__ void rs_group(SYNC&& sync, NEXT&& next, ACC&& acc_of, X0&& x0_of, X1&& x1_of, TAILT tail) {
    WF2 f[2];
    if constexpr (!IS_PRE) { if constexpr (N >= 2) sync(I2{}, tail, NOX{}); else sync(I1{}, tail, NOX{}); }
    next(f[0]);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (i + 1 < N) {
            if (((i + 1) & 1) == 0) { if (i + 2 < N) sync(I2{}, tail, NOX{}); else sync(I1{}, tail, NOX{}); }
            next(f[(i + 1) & 1]);
        }
        rs_fma<T>(f[i & 1], acc_of(i), x0_of(i), x1_of(i));
        if (i + 1 < N) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
    }
}

// ---- pair exchange.  xmine / xpart = xbuf + (wave / pw) * 5120 + lane * 16: the fragment a lane needs from its partner is the one the same lane holds
// full swap of the partners' halves: a0 / a1 <- (own k steps, partner's) for both token tiles (two rounds through the 40 KB buffer)
__device__ __forceinline__ void rs_swap_full(const uint4 (&own)[5][2], uint4 (&a0)[5][2], uint4 (&a1)[5][2], unsigned char* const& xmine, const unsigned char* const& xpart, const bool& hi) {
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        if (tt) rs_meet();      // the partner has read round 0
#pragma unroll
        for (int rb = 0; rb < 5; ++rb) *(uint4*)(xmine + rb * 1024) = own[rb][tt];
        rs_meet();
#pragma unroll
        for (int rb = 0; rb < 5; ++rb) {
            const uint4 o = *(const uint4*)(xpart + rb * 1024);
            a0[rb][tt] = rs_sel(hi, own[rb][tt], o);
            a1[rb][tt] = rs_sel(hi, o, own[rb][tt]);
        }
    }
}
// pair-merged LayerNorm over 320 channels: own[rb][tt] = h16(LN(t) g + b) of this wave's channels = k step 2 rb + hf of the row.  Each wave's (mean, M2)
// over its 160 channels goes through sbuf ([8 waves][64 lanes] float4) and is merged with the partner's by Chan's formula.  prm: the kernel's parameter block in LDS, goff / boff: gamma and beta in it.
// (The tail's two LayerNorms; the front spells its one out in place, like the MFMA loop of rs_group: vv_chain.hip at chain_front_rs_c320_kernel.)
template <typename T, int NP>
__device__ __forceinline__ void rs_layer_norm(const f32x4 (&t)[10][2], const float (&prm)[NP], const int& goff, const int& boff, float (&sbuf)[2048], const int& wave, const int& pw,
                                              const int& lane, const int& hf, const int& lg, uint4 (&own)[5][2]) {
    float mloc[2], m2loc[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 10; ++j) s += (t[j][tt][0] + t[j][tt][1]) + (t[j][tt][2] + t[j][tt][3]);
        s += __shfl_xor(s, 16); s += __shfl_xor(s, 32);
        mloc[tt] = s * (1.0f / 160);
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 10; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float d = t[j][tt][r] - mloc[tt]; q += d * d; }
        q += __shfl_xor(q, 16); q += __shfl_xor(q, 32);
        m2loc[tt] = q;
    }
    *(float4*)(sbuf + (wave * 64 + lane) * 4) = make_float4(mloc[0], m2loc[0], mloc[1], m2loc[1]);
    rs_meet();
    const float4 o4 = *(const float4*)(sbuf + (pw * 64 + lane) * 4);
    const float om[2] = {o4.x, o4.z}, oq[2] = {o4.y, o4.w};
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const float mean = 0.5f * (mloc[tt] + om[tt]), dm = mloc[tt] - om[tt];
        const float rstd = rsqrtf((m2loc[tt] + oq[tt] + 80.0f * dm * dm) * (1.0f / 320) + 1e-5f);
#pragma unroll
        for (int rb = 0; rb < 5; ++rb) {
            f32x4 y[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = 2 * rb + h, c = rs_chan(j, hf, lg);
                const float4 g = *(const float4*)(prm + goff + c), b = *(const float4*)(prm + boff + c);
                y[h][0] = (t[j][tt][0] - mean) * rstd * g.x + b.x; y[h][1] = (t[j][tt][1] - mean) * rstd * g.y + b.y;
                y[h][2] = (t[j][tt][2] - mean) * rstd * g.z + b.z; y[h][3] = (t[j][tt][3] - mean) * rstd * g.w + b.w;
            }
            own[rb][tt] = rs_frag<T>(y[0], y[1]);
        }
    }
}

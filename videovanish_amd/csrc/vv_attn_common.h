// Shared by the attention translation units (vv_attn.hip, vv_attn32.hip): which kernel a launch takes (host), which (batch, head, query tile) a block works
// on and where its tensors start.
#pragma once
#include "vv_lds_dma.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// The dispatcher's decisions, as host functions that read only the parameter fields (pointers as null / non-null flags): vv_attention launches the route
// attn_route returns and vv_attention_route reports it -- one copy of the rules.  The reasons for the thresholds stand at the launches (attn_dispatch in
// vv_attn.hip, attn40_launch / attn80_launch in vv_attn32.hip).

// the 77-key cross-attention shape: fewer than 128 keys and not self-attention
inline bool attn_is_cross(const vv_attn_params& p) { return p.Nkv < 128 && p.Nq != p.Nkv; }

// the 32x32x16 kernels (vv_attn32.hip): a VV_ATTN_ROUTE_MFMA32_* code, or 0 when the shape is left to the 16x16x32 kernels.  They take self-attention (or any
// Nq / Nkv that is not the cross shape) over at least 64 keys, not the short shapes; d = 40: 64 queries per wave from 1024 queries; d = 80: from 512 queries
inline int attn_route_mfma32(const vv_attn_params& p) {
    if ((p.Nq <= 32 && p.Nkv <= 32) || attn_is_cross(p) || p.Nkv < 64) return 0;
    const int ragged = p.Nkv % 64 ? VV_ATTN_ROUTE_RAGGED : 0;
    if (p.D == 40) return (p.Nq >= 1024 ? VV_ATTN_ROUTE_MFMA32_D40_Q2 : VV_ATTN_ROUTE_MFMA32_D40) | ragged;
    if (p.D == 80 && p.Nq >= 512) return VV_ATTN_ROUTE_MFMA32_D80 | ragged;
    return 0;
}

// the 16x16x32 kernels (vv_attn.hip) for a built head dim
inline int attn_route_generic(const vv_attn_params& p) {
    if (p.D >= 512) return p.Nq >= 256 ? VV_ATTN_ROUTE_D512_W8 : VV_ATTN_ROUTE_D512_W4;
    if (p.Nq <= 32 && p.Nkv <= 32) return (p.D >= 128 && p.Nq > 16) ? VV_ATTN_ROUTE_SHORT_2W : VV_ATTN_ROUTE_SHORT;
    if (p.D <= 80) return (p.D <= 64 ? VV_ATTN_ROUTE_DMA64 : VV_ATTN_ROUTE_REG80) | (attn_is_cross(p) ? VV_ATTN_ROUTE_CROSS : 0);
    if (p.D == 256 && (int64_t)p.B * p.heads * ((p.Nq + 127) / 128) <= 128) return VV_ATTN_ROUTE_W8x16;
    if (p.D == 160 && p.Nq >= 256) return VV_ATTN_ROUTE_W8x16;
    return VV_ATTN_ROUTE_W4x32;
}

// queries per block of a route
inline int attn_route_block_queries(const int route) {
    switch (route & ~15) {
        case VV_ATTN_ROUTE_SHORT: case VV_ATTN_ROUTE_SHORT_2W: return 32;
        case VV_ATTN_ROUTE_D512_W4: return 64;
        case VV_ATTN_ROUTE_MFMA32_D40_Q2: case VV_ATTN_ROUTE_MFMA32_D80: return 256;
        default: return 128;      // DMA64, REG80, W4x32, W8x16, D512_W8, MFMA32_D40
    }
}

// argument checks + route: a VV_ATTN_ROUTE_* code (> 0) or the VV_E_* code the launch is refused with (message set)
inline int attn_route(const vv_attn_params* pp, const int dtype) {
    if (!pp) VV_FAIL(VV_E_ARG, "vv_attention: null params");
    const vv_attn_params& p = *pp;
    if (!p.q || !p.k || !p.v || !p.o) VV_FAIL(VV_E_ARG, "vv_attention: null pointer");
    if (p.B <= 0 || p.heads <= 0 || p.Nq <= 0 || p.Nkv <= 0) VV_FAIL(VV_E_ARG, "vv_attention: empty problem");
    if ((p.q_rs | p.k_rs | p.v_rs | p.o_rs | p.q_bs | p.k_bs | p.v_bs | p.o_bs) & 3) VV_FAIL(VV_E_ARG, "vv_attention: strides must be multiples of 4 elements (q/k/v: 8)");
    if ((p.q_rs | p.k_rs | p.v_rs | p.q_bs | p.k_bs | p.v_bs | p.q_hs | p.k_hs | p.v_hs) & 7) VV_FAIL(VV_E_ARG, "vv_attention: q/k/v strides must be multiples of 8 elements");
    if (p.o_hs & 3) VV_FAIL(VV_E_ARG, "vv_attention: o_hs must be a multiple of 4 elements");
    if (dtype != VV_BF16 && dtype != VV_F16) VV_FAIL(VV_E_ARG, "vv_attention: bad dtype");
    if (p.lse && p.D == 40) VV_FAIL(VV_E_UNSUPPORTED, "vv_attention: lse output is not available at D = 40");
    switch (p.D) {
        case 32: case 40: case 64: case 80: case 128: case 160: case 256: case 512: break;
        default: VV_FAIL(VV_E_UNSUPPORTED, "vv_attention: head dim %d not built (32,40,64,80,128,160,256,512)", p.D);
    }
    int route = (p.D == 40 || p.D == 80) ? attn_route_mfma32(p) : 0;
    if (!route) route = attn_route_generic(p);
    const int bq = attn_route_block_queries(route);
    if ((int64_t)p.B * p.heads * ((p.Nq + bq - 1) / bq) > 0x7fffffff) VV_FAIL(VV_E_ARG, "vv_attention: grid too large");
    return route;
}

// XCD-aware decode: blocks i and i+8 share an XCD (and its L2).  Give every XCD its own (batch, head) pairs and walk
// that pair's query tiles on it, so the pair's K/V (re-read by every query tile) stays resident in ONE 4 MiB L2.
__device__ __forceinline__ void attn_block_decode(const vv_attn_params& p, const int nqt, int& qt, int& hd, int& b) {
    const int nbh = p.B * p.heads;
    const int full = (nbh / 8) * 8;                       // pairs handled in XCD-striped rounds of 8
    const int bid = blockIdx.x;
    int bh;
    if (bid < full * nqt) { const int xcd = bid & 7, idx = bid >> 3; bh = (idx / nqt) * 8 + xcd; qt = idx % nqt; }
    else { const int r = bid - full * nqt; bh = full + r / nqt; qt = r % nqt; }
    hd = bh % p.heads; b = bh / p.heads;
}

// where (batch b, head hd) of a q / k / v / o tensor starts, in elements; a head stride of 0 = heads side by side inside a row (D apart)
template <int D>
__device__ __forceinline__ unsigned short* attn_head_base(const void* base, const int b, const int64_t bs, const int hd, const int64_t hs) {
    return (unsigned short*)base + (int64_t)b * bs + (int64_t)hd * (hs ? hs : D);
}

}  // namespace

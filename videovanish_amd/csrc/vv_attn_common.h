// Shared by the attention translation units (vv_attn.hip, vv_attn32.hip): which (batch, head, query tile) a block works on and where its tensors start.
#pragma once
#include "vv_lds_dma.h"

namespace {

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

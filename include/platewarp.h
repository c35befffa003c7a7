/* platewarp.h -- C ABI of the clean-plate warp entry points of libvvhip.so (videovanish_amd/csrc/vv_platewarp.hip; Python binding:
 * videovanish_amd/platewarp_bind.py; settings, fit and tables: videovanish_amd/platewarp.py; host restatement: tests/platewarp_ref.py;
 * DESIGN.md section 28).
 *
 * Conventions are those of vvhip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL = the null stream), the
 * return value is 0 = launched (or nothing to launch) or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched),
 * and vvw_last_error() gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).  Nothing here
 * reads the environment.
 *
 * The rules (they are the ABI).  vvalign.h's tracker gives one integer translation per frame against a held key; what follows refines it to
 * one affine map per frame and fills on a canvas built through that map.  All arithmetic is integer.
 *   S.  Search (vvw_search), on the level-0 planes of vvalign.h's packed pyramid: frame t's record starts at pyr + t * stride, its luma plane
 *       Y [H][W] at byte 0 and its valid plane ({0, 1}) at byte H * W.  track [T][8] int32 is vva_track's: off[t] = (track[t][0], track[t][1])
 *       = (x, y), key_t = track[t][2], frame t is TRACKED when track[t][3] == 1; only these four ints are read.
 *       Frame t's plane is cut into nby = H / block rows of nbx = W / block whole blocks of block x block pixels anchored at the origin
 *       (integer division: partial edge blocks are dropped; no block at all is legal and launches nothing).
 *       A block is USABLE when frame t is tracked, 0 <= key_t < T, key_t != t, every pixel of the block is valid, and its activity
 *       sum |Y[y][x + 1] - Y[y][x]| + sum |Y[y + 1][x] - Y[y][x]| (both pixels inside the block) is at least min_texture * block^2.
 *       d0 = off[t] - off[key_t], in 64 bits.  A candidate is (dx, dy) with |dx|, |dy| <= search.  It is VALID when every pixel p of the block,
 *       moved to p + d0 + (dx, dy), lies inside the key's plane and is valid there.  Its cost is sum |Yk[p + d0 + d] - Yt[p]| over the block.
 *       The winner is the lexicographic minimum of (cost, dx^2 + dy^2, dy, dx) over the valid candidates: no order of evaluation enters.
 *       rec [T][nby][nbx][4] int32 gets (dx, dy, 1, cost) when the block is usable, a valid candidate exists and the winner's cost is at most
 *       max_residual * block^2; otherwise (0, 0, 0, 0).  Every int is written.
 *       stats [T][4] int64, cleared first, exact integer atomics: [0] the usable blocks, [1] the used blocks, [2] the sum of the used blocks'
 *       costs, [3] the sum of their |dx| + |dy|.
 *       Every frame of the segment is searched in one launch: no frame depends on another.
 *   M.  Maps.  A map is 6 int64 (ax, bx, cx, ay, by, cy) in fixed point with VVW_FRAC_BITS fraction bits; it takes the integer point (x, y) to
 *       ((ax + bx x + cx y + 2^19) >> 20, (ay + by x + cy y + 2^19) >> 20), the sums taken modulo 2^64 and read as two's complement, >> the
 *       arithmetic shift.  Maps are data: every content is legal, and every place a map leads to is bounds-checked before it is read.
 *       fwd[t] takes a pixel of frame t to the canvas, inv[t] takes a canvas pixel to frame t; canvas coordinates are absolute (they may be
 *       negative), the canvas box holds the canvas pixels [cy0, cy0 + ch) x [cx0, cx0 + cw).
 *   P.  Place (vvw_place).  The canvas pixel c of frame b reads the frame pixel p = inv[b](c).  When tracked[b] != 0 and p lies inside the
 *       frame: canvas = the frame's 3 bytes at p, dil_c = dil at p, invalid_c = 0.  Otherwise: zeros, dil_c = 0, invalid_c = 255.
 *   U.  Unplace (vvw_unplace).  For the frame pixel p of frame t, c = fwd[t](p).  p is FILLED when tracked[t] != 0, dil[t][p] != 0, c lies in
 *       the canvas box, dil_c[t][c] != 0 and dil_out_c[t][c] == 0.  dil_out[t][p] = 0 when p is filled, else dil[t][p].  The patch holds the
 *       frame pixels [py0, py0 + ph) x [px0, px0 + pw) (inside the frame): the canvas' 3 bytes at c when p is filled, else zeros.
 * With maps that are integer translations (bx = cy = 2^20, cx = by = 0, ax and ay multiples of 2^20), P and U give the bytes of
 * vva_place_masks, of the host's slices of the frames, and of vva_unplace_mask.
 */
#ifndef PLATEWARP_H
#define PLATEWARP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVW_ABI_VERSION 1
#define VVW_FRAC_BITS 20
#define VVW_MAX_SEARCH 8
#define VVW_MAX_T 65535
#define VVW_MAX_PIXELS (1 << 24)
#define VVW_TRACK_INTS 8
#define VVW_REC_INTS 4
#define VVW_NSTAT 4
#define VVW_MAP_INTS 6

int vvw_abi_version(void);
const char* vvw_last_error(void);

/* Rule S.  pyr [T][stride] u8 (stride >= 2 H W), track [T][8] int32, rec [T][H / block][W / block][4] int32, stats [T][4] int64.  One wave per
 * block; the block and the key's search area (luma and valid) are staged in LDS, every read of the key's plane is bounds-checked, whatever
 * track holds.  Every int of rec and of stats is written, nothing else; with H < block or W < block only stats is cleared (rec has no element
 * then and may be null).  Null pointer,
 * T, H, W < 1, block < 1, search < 0, min_texture < 0, max_residual < 0 -> -1; block not 16 or 32, search > VVW_MAX_SEARCH, min_texture > 510,
 * max_residual > 255, T > VVW_MAX_T, H * W > VVW_MAX_PIXELS, stride < 2 H W -> -2. */
int vvw_search(const uint8_t* pyr, int64_t stride, const int32_t* track, int T, int H, int W, int block, int search, int min_texture, int max_residual,
               int32_t* rec, int64_t* stats, void* stream);

/* Rules M, P.  frames [B][H][W][3] u8, dil [B][H][W] u8, inv [B][6] int64, tracked [B] u8, canvas [B][ch][cw][3] u8, dil_c and invalid_c
 * [B][ch][cw] u8: a batch of the segment's frames and the rows of the canvas that belong to them.  One thread per canvas pixel.  Every byte
 * of the three outputs is written, nothing else.  Null pointer, B, H, W, ch, cw < 1 -> -1; B > VVW_MAX_T, H * W > VVW_MAX_PIXELS,
 * ch * cw >= 2^31 -> -2. */
int vvw_place(const uint8_t* frames, const uint8_t* dil, const int64_t* inv, const uint8_t* tracked, int B, int H, int W, int cy0, int cx0, int ch,
              int cw, uint8_t* canvas, uint8_t* dil_c, uint8_t* invalid_c, void* stream);

/* Rules M, U.  canvas [T][ch][cw][3] u8, dil_c and dil_out_c [T][ch][cw] u8, dil [T][H][W] u8, fwd [T][6] int64, tracked [T] u8, patch
 * [T][ph][pw][3] u8, dil_out [T][H][W] u8 (not dil).  One thread per frame pixel.  Every byte of patch and of dil_out is written, nothing
 * else.  Null pointer, a size < 1, a patch box that leaves the frame (py0 < 0, px0 < 0, py0 + ph > H, px0 + pw > W), dil_out == dil -> -1;
 * T > VVW_MAX_T, H * W > VVW_MAX_PIXELS, ch * cw >= 2^31 -> -2. */
int vvw_unplace(const uint8_t* canvas, const uint8_t* dil_c, const uint8_t* dil_out_c, const uint8_t* dil, const int64_t* fwd, const uint8_t* tracked,
                int T, int H, int W, int cy0, int cx0, int ch, int cw, int py0, int px0, int ph, int pw, uint8_t* patch, uint8_t* dil_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif

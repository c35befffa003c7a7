/* vvalign.h -- C ABI of the clean-plate alignment entry points of libvvhip.so (videovanish_amd/csrc/vv_align.hip; Python binding:
 * videovanish_amd/align_hip.py; host: videovanish_amd/platealign.py, infill.plate_fill(acfg=); rules: DESIGN.md section 17).
 *
 * Conventions are those of vvhip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL = the null stream), the
 * return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched), and vva_last_error()
 * gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).
 *
 * THE RULES.  The clean-plate fill of vvplate.h needs the background at the same place in every frame.  A camera that pans or tilts shows it at
 * another place; this unit finds, per frame, ONE integer translation and lays the frames' masks out on a common canvas on which vvplate.h's
 * kernels run unchanged.  All arithmetic is integer, so the device result equals a host restatement bit for bit.  One call works on ONE
 * segment (the frames between two cuts), frames 0 .. T - 1: frames [T][H][W][3] u8, dil [T][H][W] u8 (non-zero = masked).
 *
 *   LUMA AND PYRAMID.  Level 0: Y = (77 R + 150 G + 29 B + 128) >> 8 (the luma of vvspans.h), valid = (dil == 0).  Level l has H_l = H >> l
 *   rows and W_l = W >> l columns: Y_l = (a + b + c + d + 2) >> 2 over the 2 x 2 children at (2y, 2x) .. (2y + 1, 2x + 1) of level l - 1, valid
 *   when all four children are; an odd last row or column of the finer level is dropped.  The caller picks the coarsest level L it uses:
 *   the largest l <= levels with min(H, W) >> l >= 16 (platealign.coarsest_level).
 *   THE PACKED BUFFER: pyr [T][S] u8, S = vva_frame_bytes(H, W, L) = sum over l = 0 .. L of 2 H_l W_l.  Inside a frame's record level l starts at
 *   o_l = sum over j < l of 2 H_j W_j: the Y plane [H_l][W_l] at o_l, the valid plane [H_l][W_l] (1 / 0) at o_l + H_l W_l.
 *
 *   COST of a displacement d = (dx, dy) of frame t against key k at level l: over the pixels (x, y) of frame t's plane with (x + dx, y + dy)
 *   inside the key's plane and both valid, sad = sum |Yk[y + dy][x + dx] - Yt[y][x]| and n = their number.  d is ELIGIBLE when
 *   100 n >= min_overlap H_l W_l.  a is BETTER than b when sad_a n_b < sad_b n_a in 64 bits (H W <= 2^24 keeps sad < 2^32 and n <= 2^24: exact);
 *   on equality the smaller (dx - cx)^2 + (dy - cy)^2 wins, then the smaller dy, then the smaller dx; c = (cx, cy) is the search centre.
 *
 *   SEARCH.  The centre at level L is the prediction divided by 2^L, rounded toward zero; level L searches c +- radius in x and y; every
 *   finer level searches +- 1 round twice the best of the level above.  A level without an eligible candidate LOSES the frame.
 *
 *   TRACK.  off[0] = (0, 0), tracked[0] = 1, key_1 = 0.  For t >= 1: q = the last tracked frame before t, the prediction is
 *   off[q] - off[key_t]; tracked[t] holds when the best d of level 0 has sad <= max_residual n; then off[t] = off[key_t] + d, otherwise
 *   off[t] = off[q] (kept for the record only).  key_{t+1} = t when tracked[t] and (4 |off[t].x - off[key_t].x| > W or 4 |off[t].y - off[key_t].y|
 *   > H), else key_t.  The content of frame t at (x, y) sits on the canvas at (x + off[t].x, y + off[t].y).
 *
 *   THE RECORD: track [T][8] int32 = dx, dy, key, tracked, sad_lo, sad_hi, n, level.  A finished frame holds off[t] in (dx, dy), key_t,
 *   tracked 1 / 0, the 64-bit sad (low and high word) and n of its level-0 best and level 0; a lost frame holds sad = n = 0 and the level that
 *   lost it; frame 0 holds (0, 0, 0, 1, 0, 0, 0, 0).  A frame IN PROGRESS holds the centre of the level to search next in (dx, dy), key_t,
 *   tracked = VVA_IN_PROGRESS and that level; vva_sad and vva_pick do nothing for a frame that is not in progress at the level they are called
 *   for, so every launch of a segment can be enqueued before the first one has run.
 */
#ifndef VVALIGN_H
#define VVALIGN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVA_ABI_VERSION 1
#define VVA_MAX_LEVELS 6
#define VVA_MAX_RADIUS 8
#define VVA_MAX_PIXELS (1 << 24)
#define VVA_MAX_T 65535
#define VVA_IN_PROGRESS (-1)
#define VVA_TRACK_INTS 8

int vva_abi_version(void);
const char* vva_last_error(void);

/* S of the packed buffer for levels 0 .. L, or a negative code.  Host arithmetic only.  H, W < 1, L < 0 -> -1; H * W > VVA_MAX_PIXELS,
 * L > VVA_MAX_LEVELS, min(H, W) >> L < 1 -> -2 (these hold for every function below that takes H, W and L). */
int64_t vva_frame_bytes(int H, int W, int L);

/* Luma and pyramid of B frames: frames [B][H][W][3] u8, dil [B][H][W] u8 -> pyr [B][S] (the records of these frames inside a segment's
 * buffer).  L + 1 launches.  B < 1 -> -1. */
int vva_pyramid(const uint8_t* frames, const uint8_t* dil, int B, int H, int W, int L, uint8_t* pyr, void* stream);

/* (sad, n) of every candidate of level `level` of frame t against its key: centre and key are read from track[t] on the device.  acc
 * [(2 r + 1)^2][2] uint64 = (sad, n), candidate (dx, dy) = (cx + i - r, cy + j - r) at index j (2 r + 1) + i; cleared first; left at zero
 * when frame t is not in progress at `level` or its record's key is not in [0, T).  T < 1, t outside [0, T), level outside [0, L], r < 0 -> -1;
 * T > VVA_MAX_T, r > VVA_MAX_RADIUS -> -2. */
int vva_sad(const uint8_t* pyr, const int32_t* track, int T, int H, int W, int L, int t, int level, int r, uint64_t* acc, void* stream);

/* The order, eligibility, acceptance and key rules on vva_sad's acc of the same (t, level, r): writes track[t] (the centre of level - 1, the
 * lost frame's record, or at level 0 the final record) and, when frame t is finished by it and t + 1 < T, the in-progress record of frame
 * t + 1 (key_{t+1}, the centre of level L).  min_overlap outside [1, 100], max_residual outside [0, 255] -> -1; the rest as vva_sad. */
int vva_pick(const uint64_t* acc, int32_t* track, int T, int H, int W, int L, int t, int level, int r, int min_overlap, int max_residual,
             void* stream);

/* The whole segment: writes the records of frame 0 and (in progress) frame 1, then for t = 1 .. T - 1 and level = L .. 0 vva_sad and vva_pick
 * (radius at level L, 1 below), all on `stream` with no host synchronisation in between.  acc: scratch of (2 radius + 1)^2 * 2 uint64 (at
 * least 18).  radius < 1 -> -1; the rest as vva_pick.  Launches per segment: see vva_track_launches. */
int vva_track(const uint8_t* pyr, int32_t* track, uint64_t* acc, int T, int H, int W, int L, int radius, int min_overlap, int max_residual,
              void* stream);

/* Kernel launches and memsets vva_track enqueues for T frames and levels 0 .. L (host arithmetic only). */
int64_t vva_track_launches(int T, int L);

/* dil [T][H][W] + track + the canvas box (cy0, cx0 = the canvas coordinates of its first row and column; ch rows, cw columns) -> dil_c,
 * invalid_c [T][ch][cw] u8.  The canvas pixel (cy0 + j, cx0 + i) of a tracked frame t that lies inside the frame, i.e. at frame pixel
 * (cy0 + j - off[t].y, cx0 + i - off[t].x), gets dil_c = dil there and invalid_c = 0; every other one, and every pixel of a frame whose
 * record is not tracked == 1, dil_c = 0 and invalid_c = 255.  ch, cw < 1 -> -1; ch * cw >= 2^31 -> -2. */
int vva_place_masks(const uint8_t* dil, const int32_t* track, int T, int H, int W, int cy0, int cx0, int ch, int cw, uint8_t* dil_c,
                    uint8_t* invalid_c, void* stream);

/* Back to frame coordinates: dil_out [T][H][W] (not dil) = dil_out_c at the pixel's canvas place for a tracked frame's pixel inside the
 * canvas box, dil itself everywhere else (outside the box, and the whole of an untracked frame). */
int vva_unplace_mask(const uint8_t* dil_out_c, const uint8_t* dil, const int32_t* track, int T, int H, int W, int cy0, int cx0, int ch, int cw,
                     uint8_t* dil_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif

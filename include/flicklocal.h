/* flicklocal.h -- C ABI of the block-matched inpaint deflicker entry points of libvvhip.so (videovanish_amd/csrc/vv_flicklocal.hip; Python
 * binding: videovanish_amd/flicklocal_bind.py; settings: videovanish_amd/deflickerlocal.py; host restatement: tests/deflickerlocal_ref.py;
 * DESIGN.md section 26).
 *
 * Conventions are those of vvhip.h: every pointer is a DEVICE pointer, `stream` is a hipStream_t passed as void* (NULL = the null stream), the
 * return value is 0 = launched or a negative code (-1 bad argument, -2 unsupported, -3 launch failed; nothing launched), and vvk_last_error()
 * gives the message of the calling thread's last failure (the string vv_last_error() of vvhip.h returns).  Nothing here reads the environment.
 *
 * The rule (it is the ABI) is vvflicker.h's sigma filter along time, read along one integer displacement per small block and per temporal
 * neighbour, found by block matching on the window's own pixels.  Everything of vvflicker.h and vvflickalign.h holds: x_t(p), the windows,
 * `offsets`, `track` (off[t] = (track[t][0], track[t][1]) = (x, y); frame t is TRACKED when track[t][3] == 1; only these three ints of a record
 * are read), lost frames, rules 3 to 5.  An all-zero, all-tracked track stands for "no tracker".  The additions:
 *   D.  e_t = offsets[t] + (off[t].y, off[t].x), and D(t, s) = e_t - e_s (y with y, x with x), taken in 64 bits: the pixel (yy, xx) of frame
 *       t's window lies over (yy, xx) + D(t, s) of frame s's window.
 *   B.  Blocks.  Frame t's window is cut into blocks of block x block pixels anchored at the window's origin: nby = ceil(h / block), nbx =
 *       ceil(w / block); the block (by, bx) holds the pixels [by block, min(h, (by + 1) block)) x [bx block, min(w, (bx + 1) block)): edge
 *       blocks hold the pixels that exist.
 *   S.  Search (vvk_search).  For every frame t, every slot k = s - t + radius with 0 <= k <= 2 radius, and every block: a candidate is
 *       (dy, dx) with |dy|, |dx| <= search.  It is VALID when every pixel (yy, xx) of the block, displaced to (yy, xx) + D(t, s) + (dy, dx),
 *       lies inside [0, h) x [0, w) of frame s's window.  Its cost is the sum of |x_s(q)_c - x_t(p)_c| over the block's pixels and the three
 *       channels, plus lam * (|dy| + |dx|).  The winner is the lexicographic minimum of (cost, dy^2 + dx^2, dy, dx) over the valid
 *       candidates, so it does not depend on the order in which they are tried.
 *       mv [T][2 radius + 1][nby][nbx][4] int32 gets (dy, dx, 1, cost) of the winner, and (0, 0, 0, 0) when s == t, when s lies outside
 *       0 .. T - 1, when t or s is not tracked, or when no candidate is valid.  Every int of mv is written.
 *       stats [T][2 radius + 1][6] int64, cleared first, exact integer atomics: [0] the blocks with a winner, [1] the winners with a non-zero
 *       vector, [2] the sum of |dy| + |dx|, [3] the largest max(|dy|, |dx|) (an atomic max), [4] the sum of the winners' costs, [5] the sum of
 *       the zero candidate's cost over the blocks where that candidate is valid.
 *   2''. Samples (vvk_hold).  vvflickalign.h's rule 2' with one change: the place of candidate s for the frame pixel p is q = p + off[t] -
 *       off[s] + (dy, dx), in window coordinates (yy, xx) + D(t, s) + (dy, dx), with (dy, dx, used, .) = mv[t][k][yy / block][xx / block];
 *       the candidate is taken only when `used` == 1 (and both frames are tracked, s != t, q inside frame s's window, the gate passes).
 *       mv is data: every int32 content is legal, the sum is taken in 64 bits.
 * The gate, the rounded mean, out, the 12 sums and the lost-frame rule are unchanged, so |out_c - x_t(p)_c| <= tol still holds by construction:
 * the failure mode stays "not smoothed", never "ghosted".  With every record (0, 0, 1, .) vvk_hold gives vvc_hold's bytes and sums.  Nothing
 * crosses the ends of the clip call.
 */
#ifndef FLICKLOCAL_H
#define FLICKLOCAL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VVK_ABI_VERSION 1
#define VVK_MAX_RADIUS 4
#define VVK_MAX_T 65535
#define VVK_TRACK_INTS 8
#define VVK_MAX_SEARCH 8
#define VVK_MAX_LAM 65535   /* a cost stays below 2^31: 16 * 16 * 3 * 255 + 16 * 65535 */
#define VVK_MV_INTS 4
#define VVK_NSTAT 6

int vvk_abi_version(void);
const char* vvk_last_error(void);

/* Rules D, B, S.  win [T][h][w][3] u8, offsets [T][2] int32 (oy, ox), track [T][8] int32, mv [T][2 radius + 1][nby][nbx][4] int32, stats
 * [T][2 radius + 1][6] int64.  One wave per block; the reference blocks and the search area of frame s are staged in LDS, every read of win
 * is bounds-checked against the window of the frame it comes from, whatever offsets and track hold.  Every int of mv and of stats is written,
 * nothing else.  Null pointer, a size <= 0, radius < 0, block <= 0, search < 0, lam < 0 -> -1; block not 8 or 16, search > VVK_MAX_SEARCH,
 * lam > VVK_MAX_LAM, radius > VVK_MAX_RADIUS, T > VVK_MAX_T, h * w >= 2^31, T * (2 radius + 1) * nby * ceil(nbx / 256) >= 2^31 (the workgroups) -> -2. */
int vvk_search(const uint8_t* win, const int* offsets, const int32_t* track, int T, int h, int w, int radius, int block, int search, int lam,
               int32_t* mv, int64_t* stats, void* stream);

/* Rule 2'' and vvflicker.h's rules 3 - 5.  win, offsets, track as above, mv [T][2 radius + 1][nby][nbx][4] int32 (any content), mask2d
 * [T][H0][W0] u8, out [T][h][w][3] u8 (not win), sums [T][12] int64.  One thread per output pixel, vvc_hold's gather form with the block's
 * record read per neighbour.  Reads of win are bounds-checked against the window of the frame they come from and reads of the mask against
 * the frame, whatever offsets, track and mv hold.  Every byte of out and of sums is written, nothing else.  Null pointer, a size <= 0, h > H0,
 * w > W0, radius < 0, block <= 0, tol < 0, out == win -> -1; block not 8 or 16, radius > VVK_MAX_RADIUS, tol > 255, T > VVK_MAX_T,
 * h * w >= 2^31 -> -2. */
int vvk_hold(const uint8_t* win, const int* offsets, const int32_t* track, const int32_t* mv, const uint8_t* mask2d, int T, int H0, int W0, int h,
             int w, int radius, int block, int tol, uint8_t* out, int64_t* sums, void* stream);

#ifdef __cplusplus
}
#endif
#endif

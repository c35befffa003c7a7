"""The orchestration of one diffuerase.run_infill_on_frames call after the dilation: the mask clean-up (clean_masks), the overlay masking
(overlay_mask), the shadow masking (shadow_mask), the clean-plate fill (plate_fill), the temporal plan (span_plan, run_spans), and for each clip the windows (region_plans, run_clip), ONE crop -> prior -> model
sequence (run_windows) and ONE closing step (finish).  The full frame is no window, roi= "static" / "follow" one, the "-regions" spellings
several.  The closing step is one loop over the windows; in it the opt-in seam stages run on each window's pixels before they are pasted: the
deflicker along time (with its alignment along a translation tracked per clip call and along block-matched vectors), the tone fit to the ring round the mask, the grain the
ring's originals have and the model's pixels lack, the membrane that carries the ring's difference original - model into the hole.  Each stage
reports per clip call; tone_report, grain_report, seam_blend_report, deflicker_report, deflicker_align_report, deflicker_local_report and detail_report assemble a call's
report from them.  The stages (weights, prior, model) come from the caller as a Stages record; nothing here is module state.  Rules and reasons: DESIGN.md
§10, §11, §12, §13, §14, §15, §16, §17, §18, §19, §21, §23, §24, §26, §27."""
import dataclasses
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import align_hip, blend_hip, deflicker, deflickeralign, deflickerlocal, detailmatch, detailmatch_bind, flickalign_hip, flicker_hip, flicklocal_bind, grain_hip, grainmatch, grainshape, grainshape_bind, hip, mask_hip, overlaymask, overlaymask_bind, plate_hip, platealign, platefill, plategrain_hip, platetone, platetone_bind, platewarp, platewarp_bind, seamblend, shadow_hip, shadowmask, spans_hip, tone_hip, tonematch
from . import roi as roi_plan
from . import spans as span_planner


class Stages(NamedTuple):
    load_model: Callable    # ()
    load_prior: Callable    # (), after load_model
    run_prior: Callable     # (frames, masks, progress) -> prior frames
    run_model: Callable     # (frames, masks, prior frames, progress) -> inpainted frames (None: a frame another rank holds)


REGION_TILE = 16        # px: the occupancy grid the regions are labelled on (roi.label_tiles coarsens it for salt-like masks)


def _share(prog, what, k, n, lo, hi):
    """Progress of region / span (`what`) k's sub-call (its own values in [lo, hi]) mapped into k's share of (lo, hi), never onto lo or hi themselves,
    so the caller still sees each of 5 / 10 / 20 / 50 / 90 once and non-decreasing values."""
    if prog is None:
        return None

    def cb(v, s):
        f = min(max((v - lo) / (hi - lo), 0.0), 1.0)
        prog(min(max(lo + int((hi - lo) * (k + f) / n), lo + 1), hi - 1), f"{what} {k + 1}/{n}: {s}" if s else f"{what} {k + 1}/{n}")
    return cb


# ---- masks: what the planners and the model see -----------------------------------------------------------------------------------------------
class MaskCleanReport(NamedTuple):
    """What clean_masks changed, per frame (int64 [T] each), and the cuts its temporal steps respected."""
    removed: np.ndarray     # components cleared by the despeckle
    cleared: np.ndarray     # pixels of the dilated mask cleared with them
    bridged: np.ndarray     # pixels set by the bridge
    grown: np.ndarray       # pixels set by the grow
    cuts: tuple


def clean_masks(m, dil_t, ccfg, cuts=None):
    """The mask clean-up (maskclean.py) on the device: m = the raw masks [T,H,W,ch] u8, dil_t = their dilation [T,H,W] u8, ccfg = a
    MaskCleanConfig, cuts = frame indices, None (one segment) or a callable that finds them on the despeckled masks (the detector must not see the
    speckles).  Despeckle, then bridge and grow inside every segment of spans.segments.  Returns (the masks that replace dil_t, MaskCleanReport).
    Depends on nothing but its arguments: every rank gets the same masks.  A step that is switched off launches nothing."""
    T, H, W = dil_t.shape
    counts = np.zeros((T, 4), np.int64)
    area = ccfg.area_for(H, W)
    if area > 1:
        dil_t, c = mask_hip.despeckle(dil_t, m, area)
        counts[:, :2] = c.cpu().numpy()
    cuts = tuple(int(c) for c in ((cuts(dil_t) if callable(cuts) else cuts) or ()))
    if ccfg.bridge or ccfg.grow:
        out = torch.empty_like(dil_t)
        c = torch.empty((T, 2), dtype=torch.int64, device=dil_t.device)
        for s, e in span_planner.segments(T, cuts):
            mask_hip.time_bridge_grow(dil_t[s:e], ccfg.bridge, ccfg.grow, out=out[s:e], counts=c[s:e])
        dil_t = out
        counts[:, 2:] = c.cpu().numpy()
    return dil_t, MaskCleanReport(*(counts[:, k].copy() for k in range(4)), cuts)


# ---- overlays: the screen-fixed graphics nobody painted a mask for ------------------------------------------------------------------------------
class OverlayMaskReport(NamedTuple):
    """What overlay_mask found: the verdict ("none": no strong pixel or nothing kept; "static": the scene itself stands still, nothing added;
    "found"), rule 2's two counts, the kept components as boxes [K,5] int32 = (x0, y0, x1, y1, area) in label order (at most 256 of `found`,
    the true count; x1, y1 exclusive), the pixels added to the mask per frame (int64 [T]) and the overlay O [H,W] u8 {0, 255} on the host."""
    verdict: str
    strong: int
    edges: int
    boxes: np.ndarray
    found: int
    added: np.ndarray
    overlay: np.ndarray


def overlay_mask(frames_rgb, dil_t, ocfg):
    """The overlay masking (overlaymask.py; rules: include/overlaymask.h): frames_rgb = the T host frames [H,W,3] u8, dil_t = the
    masks [T,H,W] u8 on the device, ocfg = an OverlayMaskConfig.  One call on the whole clip: the frames cross to the device in batches of at
    most max_bytes (at least a frame) and add into one set of sums; the closing and the fringe are hip.mask_collapse_dilate, the components
    mask_hip.label_components.  Returns (dil', OverlayMaskReport): dil' is dil_t itself for the verdicts "none" and "static", and neither the
    frames nor dil_t is ever written.  Depends on nothing but its arguments: every rank gets the same masks."""
    T, H, W = dil_t.shape
    if T > overlaymask.MAX_T:
        raise ValueError(f"overlay_mask: a clip call of at most {overlaymask.MAX_T} frames is supported, not {T}")
    dev = dil_t.device
    B = overlaymask_bind
    acc = B.new_acc(H, W, dev)
    step = ocfg.batch_frames(H, W)
    for s in range(0, T, step):
        f = torch.from_numpy(np.stack(frames_rgb[s:s + step])).to(dev)
        B.accumulate(f, dil_t[s:s + step], acc)
    edge, counts = B.classify(acc, ocfg.min_samples, ocfg.mag, ocfg.coh)
    strong, edges = (int(c) for c in counts.cpu().numpy())

    def nothing(verdict):
        return dil_t, OverlayMaskReport(verdict, strong, edges, np.zeros((0, 5), np.int32), 0, np.zeros(T, np.int64), np.zeros((H, W), np.uint8))

    if strong == 0:
        return nothing("none")
    if 100 * edges > ocfg.max_share * strong:
        return nothing("static")
    closed = hip.mask_collapse_dilate(edge[None, ..., None], ocfg.close) if ocfg.close else edge[None]                 # rule 4, [1,H,W]
    lab = mask_hip.label_components((closed == 0).to(torch.uint8))[0]                                                 # rule 5: the components of ~C
    holes, _, _ = B.select(lab, B.component_stats(lab), 0, ocfg.max_hole, True)
    filled, _ = B.merge(closed, holes)
    lab = mask_hip.label_components(filled)[0]                                                                        # rule 6
    kept, boxes, nboxes = B.select(lab, B.component_stats(lab), ocfg.min_area, ocfg.max_area_px(H, W), not ocfg.border)
    found = int(nboxes.item())
    if found == 0:
        return nothing("none")
    o = hip.mask_collapse_dilate(kept[None, ..., None], ocfg.grow)[0] if ocfg.grow else kept                          # rule 7
    dil, added = B.merge(dil_t, o)
    b = boxes[:min(found, overlaymask.MAX_BOXES)].cpu().numpy()
    b = b[np.argsort(b[:, 0], kind="stable")]
    return dil, OverlayMaskReport("found", strong, edges, np.ascontiguousarray(b[:, [2, 3, 4, 5, 1]]), found, added.cpu().numpy(), o.cpu().numpy())


# ---- shadows: what the object casts beside the mask --------------------------------------------------------------------------------------------
class ShadowMaskReport(NamedTuple):
    """What shadow_mask changed: per frame (int64 [T] each) the candidate pixels of rule 4 inside the segment's crop and the pixels added to the
    mask; per segment of `segments` the pixels of its crop that have a plate and whether it was skipped (its crop exceeded max_bytes or 65535
    frames: nothing added); the cuts the segments come from."""
    candidates: np.ndarray
    added: np.ndarray
    plate: tuple
    skipped: tuple
    segments: tuple
    cuts: tuple


def _shadow_device(f, d, hcfg):
    """The stage itself on resident frames f [T,h,w,3] and their masks d [T,h,w] (include/vvshadow.h): the sample frames from
    time_bridge_grow(., 0, guard), the plate, the candidates, the growth from the frame's mask, the despeckle of what was added, its penumbra
    (mask_collapse_dilate), the union -> (d' on the device, counts [T,2] = (candidates, added) on the host, plate pixels).  A step that is
    switched off launches nothing; nothing is read back before the end."""
    notsample = d if hcfg.guard == 0 else mask_hip.time_bridge_grow(d, 0, hcfg.guard)[0]
    ok, n2, t1 = shadow_hip.plate(f, notsample, hcfg.min_samples, hcfg.tol)
    cand, counts = shadow_hip.candidates(f, d, ok, n2, t1, hcfg.lo, hcfg.hi, hcfg.drop, hcfg.chroma, hcfg.floor)
    s = shadow_hip.grow(d, cand, hcfg.reach)
    if hcfg.min_area > 1:
        s = mask_hip.despeckle(s, s, hcfg.min_area)[0]
    if hcfg.grow:
        s = hip.mask_collapse_dilate(s[..., None], hcfg.grow)
    d2 = shadow_hip.merge(d, s, counts)
    return d2, counts.cpu().numpy(), int(ok.sum().item())


def shadow_mask(frames_rgb, dil_t, hcfg, cuts=None):
    """The shadow masking (shadowmask.py; rules: include/vvshadow.h): frames_rgb = the T host frames [H,W,3] u8, dil_t = the masks
    [T,H,W] u8 on the device, hcfg = a ShadowMaskConfig, cuts = frame indices or None (one segment).  Per segment of spans.segments: the crop of
    the union box of its masks (platefill.crop_box) widened by reach + grow (shadowmask.widen_box) crosses to the device, and the masks of that
    crop are replaced (_shadow_device).  A segment without a mask pixel uploads nothing; one whose crop exceeds max_bytes, or that is longer
    than 65535 frames, is left as it is and flagged.  Returns (dil', ShadowMaskReport): dil' is dil_t itself when nothing was added at all,
    and neither the frames nor dil_t is ever written.  Depends on nothing but its arguments: every rank gets the same masks."""
    T, H, W = dil_t.shape
    cuts = tuple(int(c) for c in (cuts or ()))
    segs = tuple(span_planner.segments(T, cuts))
    boxes = hip.mask_bbox(dil_t).cpu().numpy()
    dil = dil_t
    cand, added = np.zeros(T, np.int64), np.zeros(T, np.int64)
    plate, skipped = [], []
    for s, e in segs:
        plate.append(0)
        skipped.append(False)
        box = platefill.crop_box(boxes[s:e], H, W)
        if box is None:
            continue
        box = shadowmask.widen_box(box, H, W, hcfg.widen)
        if e - s > shadowmask.MAX_T or platefill.crop_bytes(e - s, box) > hcfg.max_bytes:
            skipped[-1] = True
            continue
        y0, x0, y1, x1 = box
        f = torch.from_numpy(np.stack([fr[y0:y1, x0:x1] for fr in frames_rgb[s:e]])).to(dil_t.device)
        d2, c, plate[-1] = _shadow_device(f, dil_t[s:e, y0:y1, x0:x1].contiguous(), hcfg)
        cand[s:e], added[s:e] = c[:, 0], c[:, 1]
        if c[:, 1].any():
            if dil is dil_t:
                dil = dil_t.clone()
            dil[s:e, y0:y1, x0:x1] = d2
    return dil, ShadowMaskReport(cand, added, tuple(plate), tuple(skipped), segs, cuts)


# ---- clean plate: what the clip itself shows behind the mask -------------------------------------------------------------------------------
class PlateFillReport(NamedTuple):
    """What plate_fill changed: per frame (int64 [T] each) the pixels filled from another frame and the masked pixels left to the model; per
    segment of `segments` the steady pixels of its crop and whether it was skipped (its crop exceeded max_bytes or 65535 frames: nothing filled);
    the cuts the segments come from."""
    filled: np.ndarray
    left: np.ndarray
    steady: tuple
    skipped: tuple
    segments: tuple
    cuts: tuple


class PlateGrainReport(NamedTuple):
    """What plate_fill(gcfg=) rotated: per frame (int64 [T] each) the filled pixels whose bytes come from another frame than the nearest usable
    one, and the pixels filled (PlateFillReport.filled); the segments."""
    rotated: np.ndarray
    filled: np.ndarray
    segments: tuple


class PlateToneReport(NamedTuple):
    """What plate_fill(tcfg=) matched: per frame the fitted gain and offset per channel (float64 [T,3]: the exact rationals of the fit, rounded
    for reading only; 1 and 0 where nothing was fitted) and the identity flag (bool [T]: the frame's tables are the identity, it is left
    alone); per segment of `segments` the support n (0 where none was counted) and the path: "matched" (the fill ran on the normalised crop),
    "identity" (every frame's tables are the identity: the fill as without the option), "unfit" (fewer than min_pixels of support: the
    same), "canvas" (filled on plate_align's canvas: not matched) or "skipped" (no mask pixel, the fill itself was skipped or found no tracked frame to
    fill, or the widened crop exceeds max_bytes or 2^24 pixels: that segment is filled unmatched)."""
    gain: np.ndarray
    offset: np.ndarray
    identity: np.ndarray
    n: tuple
    path: tuple
    segments: tuple


class PlateAlignReport(NamedTuple):
    """What the tracker of plate_fill(acfg=) found, per segment of `segments` (a tuple each): off [T,2] int32 = the frame's (x, y) on the canvas,
    key [T] = the key frame it was tracked against, tracked [T] bool, residual [T] = the mean absolute luma difference of its level-0 best
    (0 for frame 0 and a lost frame), the canvas box (y0, x0, y1, x1 in canvas coordinates, or None) and the path that ran: "canvas", "static"
    (every frame tracked at offset zero: the unaligned stage as it is), "fallback" (the canvas exceeds max_bytes: the unaligned stage),
    "none" (no tracked frame has a mask pixel: nothing filled), "empty" (no mask pixel at all: nothing tracked) or "untracked" (the segment
    is beyond the tracker's limits: the unaligned stage)."""
    off: tuple
    key: tuple
    tracked: tuple
    residual: tuple
    box: tuple
    path: tuple
    segments: tuple


class PlateWarpReport(NamedTuple):
    """What plate_fill(wcfg=) fitted, per segment of `segments` (a tuple each): maps [T,6] float64 = every frame's map to the canvas (ax, bx, cx,
    ay, by, cy: x' = ax + bx x + cx y; the exact rationals, rounded for reading only; NaN for an untracked frame), usable / used / kept [T] int64
    = the blocks vvw_search could match, those it matched within plate_align's max_residual, and those the trimmed fit kept; rms [T] = the root
    mean square distance of the kept blocks' vectors from the fit, in pixels; failed [T] bool = the frames whose fit failed (they keep
    plate_align's translation); the canvas box or None; and the path that ran: "warp" (filled on the warped canvas), "translation" (every map is
    plate_align's integer translation: its canvas path as it is), "fallback" (the warped canvas exceeds max_bytes: plate_align's path),
    "none", "empty", "untracked", "static" (plate_align's paths of those names: nothing was searched)."""
    maps: tuple
    usable: tuple
    used: tuple
    kept: tuple
    rms: tuple
    failed: tuple
    box: tuple
    path: tuple
    segments: tuple


def _track_segment(frames_rgb, d_seg, acfg, max_bytes, keep=None):
    """Pyramid in frame batches of at most max_bytes of image (only the luma planes stay resident), vva_track, and the ONE synchronisation:
    -> (track on the device, track on the host).  keep = a list that receives the packed pyramid (plate_warp searches its level 0)."""
    T, H, W = d_seg.shape
    L = platealign.coarsest_level(H, W, acfg.levels)
    pyr = torch.empty((T, align_hip.frame_bytes(H, W, L)), dtype=torch.uint8, device=d_seg.device)
    B = max(1, max_bytes // (H * W * 3))
    for b in range(0, T, B):
        f = torch.from_numpy(np.stack(frames_rgb[b:b + B])).to(d_seg.device)
        align_hip.pyramid(f, d_seg[b:b + B], L, out=pyr[b:b + B])
    track_t = align_hip.track(pyr, H, W, L, acfg.radius, acfg.min_overlap, acfg.max_residual)
    if keep is not None:
        keep.append(pyr)
    return track_t, track_t.cpu().numpy()


def _plan_alignment(frames_rgb, d_seg, boxes, pcfg, acfg, keep=None):
    """Steps 1 - 4 and 6 of DESIGN.md §17 for one segment -> (track on the device or None, track [T,8] on the host, the canvas box or None,
    the path: see PlateAlignReport).  keep: _track_segment's."""
    T, H, W = d_seg.shape
    track = np.zeros((T, 8), np.int32)
    track[:, 3] = 1
    if not any(b[2] > b[0] and b[3] > b[1] for b in boxes):
        return None, track, None, "empty"
    if not platealign.trackable(T, H, W):
        return None, track, None, "untracked"
    track_t, track = _track_segment(frames_rgb, d_seg, acfg, pcfg.max_bytes) if keep is None else _track_segment(frames_rgb, d_seg, acfg, pcfg.max_bytes, keep)
    ok = track[:, 3] == 1
    if ok.all() and not track[:, :2].any():
        return track_t, track, None, "static"
    cbox = platealign.canvas_box(boxes, track[:, :2], ok)
    if cbox is None:
        return track_t, track, None, "none"
    return track_t, track, cbox, "fallback" if platealign.canvas_bytes(T, cbox) > pcfg.max_bytes else "canvas"


def _not_sample(d, pcfg):
    """Rule 1 of include/vvplate.h, complemented: the masks d [T,h,w] grown `guard` frames in time (d itself for guard = 0)."""
    return d if pcfg.guard == 0 else mask_hip.time_bridge_grow(d, 0, pcfg.guard)[0]


def _fill_device(f, d, invalid, pcfg, gcfg=None, notsample=None):
    """The fill itself on resident frames f [T,h,w,3] (written in place) and their masks d [T,h,w]: the tile occupancy, the sample frames from
    time_bridge_grow(., 0, guard) (and not where `invalid` is set: the canvas places no tracked frame covers), stats, sources, the margin
    (mask_collapse_dilate of the unfilled remainder), fill -> (d' on the device, counts [T,3] = (filled, left, rotated) on the host, steady
    pixels).  gcfg = a plategrain.PlateGrainConfig with depth > 1: vvl_sources in place of vvp_sources, and the fill gathers from its live
    sources (include/vvplategrain.h); rotated = the filled pixels whose live source is not the nearest one, 0 otherwise.  notsample = the
    sample frames of d where the caller has them already (_not_sample)."""
    occ = hip.mask_tile_union(d, plate_hip.TILE)
    if notsample is None:
        notsample = _not_sample(d, pcfg)
    if invalid is not None:
        notsample = torch.bitwise_or(notsample, invalid)
    st, n, s1 = plate_hip.stats(f, notsample, occ, pcfg.min_samples, pcfg.tol)
    rotate = gcfg is not None and gcfg.depth > 1
    if rotate:
        near, src, r0 = plategrain_hip.sources(f, d, notsample, occ, st, n, s1, pcfg.tol, pcfg.outlier, pcfg.max_gap, gcfg.depth, gcfg.reach)
    else:
        src, r0 = plate_hip.sources(f, d, notsample, occ, st, n, s1, pcfg.tol, pcfg.outlier, pcfg.max_gap)
    keep = r0 if pcfg.margin == 0 else hip.mask_collapse_dilate(r0[..., None], pcfg.margin)
    d2, c = plate_hip.fill(f, d, keep, occ, src)
    rotated = ((d != 0) & (d2 == 0) & (src != near)).flatten(1).sum(1, keepdim=True) if rotate else torch.zeros_like(c[:, :1])
    return d2, torch.cat([c, rotated.to(c.dtype)], 1).cpu().numpy(), int(st.sum().item())


def _fill_on_crop(frames_rgb, d, box, pcfg, gcfg=None):
    """One segment filled on the crop `box` of its frames (d = the masks' crop, contiguous): the crop crosses to the device, the crops of the
    frames that got a fill come back into copies of those frames -> what _fill_on_canvas returns, dil' being the crop's."""
    y0, x0, y1, x1 = box
    f = torch.from_numpy(np.stack([fr[y0:y1, x0:x1] for fr in frames_rgb])).to(d.device)
    d2, c, steady = _fill_device(f, d, None, pcfg, gcfg)
    idx = np.nonzero(c[:, 0])[0]
    new = {}
    if not len(idx):
        return new, None, c, steady
    got = f[torch.from_numpy(idx).to(f.device)].cpu().numpy()
    for j, i in enumerate(idx):
        new[int(i)] = np.array(frames_rgb[i], copy=True)
        new[int(i)][y0:y1, x0:x1] = got[j]
    return new, d2, c, steady


def _tables(raw, T, dev):
    """T * 3 * 256 bytes -> [T,3,256] u8 on the device."""
    return torch.from_numpy(np.frombuffer(raw, np.uint8).reshape(T, 3, 256).copy()).to(dev)


def _fill_matched(frames_rgb, d, box, pcfg, gcfg, tcfg):
    """One segment under plate_tone (rules: include/platetone.h) on the widened crop `box` (d = the masks' crop, contiguous): the
    crop crosses to the device, mean_plane and, with enough support, moments; the integer fit and the tables on the host.  An unfit segment
    and one whose frames are all identity end here: -> (path, fit, None) and the caller runs the fill as without the option.  Otherwise apply,
    the unchanged fill on the normalised crop (_fill_device, handed the sample frames found here), restore into a fresh buffer next to the
    original crop -> ("matched", fit, what _fill_on_crop returns)."""
    y0, x0, y1, x1 = box
    T = len(frames_rgb)
    f = torch.from_numpy(np.stack([fr[y0:y1, x0:x1] for fr in frames_rgb])).to(d.device)
    notsample = _not_sample(d, pcfg)
    mean, support, n = platetone_bind.mean_plane(f, notsample, tcfg.floor)
    n = int(n.item())
    if n < tcfg.min_pixels:
        return "unfit", platetone.fit_segment(n, [()] * T, tcfg), None
    fit = platetone.fit_segment(n, platetone_bind.moments(f, mean, support).cpu().numpy(), tcfg)
    if fit.all_identity:
        return "identity", fit, None
    ident = torch.from_numpy(np.frombuffer(fit.identity, np.uint8).copy()).to(d.device)
    f1 = platetone_bind.apply(f, _tables(fit.fwd, T, d.device), ident)
    d2, c, steady = _fill_device(f1, d, None, pcfg, gcfg, notsample)
    idx = np.nonzero(c[:, 0])[0]
    new = {}
    if not len(idx):
        return "matched", fit, (new, None, c, steady)
    out = platetone_bind.restore(f, f1, d, d2, _tables(fit.back, T, d.device))
    got = out[torch.from_numpy(idx).to(f.device)].cpu().numpy()
    for j, i in enumerate(idx):
        new[int(i)] = np.array(frames_rgb[i], copy=True)
        new[int(i)][y0:y1, x0:x1] = got[j]
    return "matched", fit, (new, d2, c, steady)


def _fill_on_canvas(frames_rgb, d_seg, track_t, track, box, pcfg, gcfg=None):
    """Steps 5 and 7 - 9 of DESIGN.md §17 for one segment: the canvas from per-frame slices, the unchanged vvp_ kernels on it, the filled pixels
    back into copies of their frames -> ({frame index: new frame}, dil' [T,H,W] or None when nothing was filled, counts [T,3] as _fill_device's, steady)."""
    T, H, W = d_seg.shape
    y0, x0, y1, x1 = box
    canvas = np.zeros((T, y1 - y0, x1 - x0, 3), np.uint8)
    where = [platealign.frame_slices(box, track[t, :2], H, W) if track[t, 3] == 1 else None for t in range(T)]
    for t, sl in enumerate(where):
        if sl is not None:
            canvas[t][sl[0]] = frames_rgb[t][sl[1]]
    f = torch.from_numpy(canvas).to(d_seg.device)
    d, invalid = align_hip.place_masks(d_seg, track_t, box)
    d2, c, steady = _fill_device(f, d, invalid, pcfg, gcfg)
    idx = np.nonzero(c[:, 0])[0]
    new = {}
    if not len(idx):
        return new, None, c, steady
    sel = torch.from_numpy(idx).to(f.device)
    got, went = f[sel].cpu().numpy(), ((d[sel] != 0) & (d2[sel] == 0)).cpu().numpy()
    for j, i in enumerate(idx):
        cs, fs = where[i]
        fr = np.array(frames_rgb[i], copy=True)
        m = went[j][cs]
        fr[fs][m] = got[j][cs][m]                                          # only the filled pixels; fr[fs] is a view
        new[int(i)] = fr
    return new, align_hip.unplace_mask(d2, d_seg, track_t, box), c, steady


def _plan_warp(pyr, d_seg, track_t, track, boxes, pcfg, acfg, wcfg):
    """Steps 1 and 2 of DESIGN.md §28 for one tracked segment: vvw_search on the resident pyramid, the read-back of its records, the exact fit
    and the tables on the host -> (the platewarp.Plan, the search's stats [T,4], the canvas box or None, the path "warp" / "translation" /
    "fallback")."""
    T, H, W = d_seg.shape
    rec, stats = platewarp_bind.search(pyr, track_t, H, W, wcfg, acfg.max_residual)
    plan = platewarp.plan_segment(track, rec.cpu().numpy(), wcfg, H, W, boxes)
    stats = stats.cpu().numpy()
    if plan.translation:
        return plan, stats, None, "translation"
    cbox = platewarp.canvas_box(boxes, plan.fwd, plan.tracked)
    return plan, stats, cbox, "fallback" if cbox is None or platewarp.canvas_bytes(T, cbox) > pcfg.max_bytes else "warp"


def _fill_on_warp(frames_rgb, d_seg, plan, cbox, pbox, pcfg, gcfg=None):
    """Step 3 of DESIGN.md §28 for one segment: the frames cross in batches of at most max_bytes and vvw_place builds the canvas through the
    inverse maps, the unchanged vvp_ kernels run on it, vvw_unplace brings the filled bytes back as a patch over pbox (the union box of the
    frames' masks), and only the filled pixels go into copies of their frames -> ({frame index: new frame}, dil' [T,H,W] or None when nothing
    was filled, counts [T,3] = (frame pixels filled, frame pixels left, rotated) on the host, steady)."""
    T, H, W = d_seg.shape
    dev = d_seg.device
    y0, x0, y1, x1 = cbox
    inv_t, fwd_t, flags = platewarp_bind.tables(plan.inv, dev), platewarp_bind.tables(plan.fwd, dev), platewarp_bind.flags(plan.tracked, dev)
    f = torch.empty((T, y1 - y0, x1 - x0, 3), dtype=torch.uint8, device=dev)
    d, invalid = torch.empty((T, y1 - y0, x1 - x0), dtype=torch.uint8, device=dev), torch.empty((T, y1 - y0, x1 - x0), dtype=torch.uint8, device=dev)
    B = max(1, pcfg.max_bytes // (H * W * 3))
    for b in range(0, T, B):
        up = torch.from_numpy(np.stack(frames_rgb[b:b + B])).to(dev)
        platewarp_bind.place(up, d_seg[b:b + B], inv_t[b:b + B], flags[b:b + B], cbox, out=(f[b:b + B], d[b:b + B], invalid[b:b + B]))
    d2, c, steady = _fill_device(f, d, invalid, pcfg, gcfg)
    patch, dil2 = platewarp_bind.unplace(f, d, d2, d_seg, fwd_t, flags, cbox, pbox)
    went = (d_seg != 0) & (dil2 == 0)
    counts = torch.stack([went.flatten(1).sum(1), (dil2 != 0).flatten(1).sum(1)], 1).cpu().numpy()
    c = np.concatenate([counts, c[:, 2:3]], 1)
    idx = np.nonzero(c[:, 0])[0]
    new = {}
    if not len(idx):
        return new, None, c, steady
    sel = torch.from_numpy(idx).to(dev)
    py0, px0, py1, px1 = pbox
    got, m = patch[sel].cpu().numpy(), went[sel][:, py0:py1, px0:px1].cpu().numpy()
    for j, i in enumerate(idx):
        fr = np.array(frames_rgb[i], copy=True)
        fr[py0:py1, px0:px1][m[j]] = got[j][m[j]]                           # only the filled pixels; the slice is a view
        new[int(i)] = fr
    return new, dil2, c, steady


def plate_fill(frames_rgb, dil_t, pcfg, cuts=None, acfg=None, align_out=None, wcfg=None, warp_out=None, gcfg=None, grain_out=None, tcfg=None, tone_out=None):
    """The clean-plate fill (platefill.py; rules: include/vvplate.h): frames_rgb = the T host frames [H,W,3] u8, dil_t = the masks
    [T,H,W] u8 on the device, pcfg = a PlateFillConfig, cuts = frame indices or None (one segment).  Per segment of spans.segments: the crop of
    the union box of its masks (platefill.crop_box) crosses to the device and is filled in place (_fill_device); only the crops of frames
    that got a fill come back, into copies of those frames.  A segment without a mask pixel uploads nothing; one whose crop exceeds max_bytes
    is left as it is and flagged.  Returns (frames', dil', PlateFillReport): a frame with nothing filled is the caller's array itself, dil' is
    dil_t itself when nothing was filled at all, and neither the caller's frames nor dil_t is ever written.  Depends on nothing but its
    arguments: every rank gets the same frames and masks.
    acfg = a platealign.PlateAlignConfig (rules: include/vvalign.h), opt-in: every segment with a mask pixel is tracked first
    (one integer translation per frame against a held key); a segment whose frames all sit at offset zero takes the path above as it is, any
    other is filled on the canvas in which its background stands still (the same vvp_ kernels; the places no tracked frame covers are no
    samples), unless the canvas exceeds max_bytes: then the path above runs and the segment is flagged "fallback".  An untracked frame gives
    no sample, gets no fill and keeps its mask.  align_out = a list that receives the call's PlateAlignReport.
    gcfg = a plategrain.PlateGrainConfig (rule: include/vvplategrain.h), opt-in: wherever a segment is filled, on the crop or on
    the canvas, every masked frame takes its bytes from up to `depth` usable frames in turn, not from the nearest alone, so that the grain inside
    the fill moves; the pixels filled, dil' and the PlateFillReport are those without it, and depth = 1 is the call without it.  grain_out = a
    list that receives the call's PlateGrainReport.
    tcfg = a platetone.PlateToneConfig (rules: include/platetone.h), opt-in: a segment filled on the crop takes that crop widened
    by `ring` (shadowmask.widen_box), fits every frame's exposure to the segment's mean image over the pixels no frame masks, runs the fill
    on the normalised crop and maps every filled pixel back to its frame's exposure (_fill_matched); an unfilled pixel keeps its bytes.  A
    segment without enough support, or whose frames all fit the identity, takes the path above as it is; a segment on the canvas is not
    matched; one whose widened crop exceeds max_bytes or 2^24 pixels is flagged "skipped" and filled as without the option.  tone_out = a list
    that receives the call's PlateToneReport.
    wcfg = a platewarp.PlateWarpConfig (rules: include/platewarp.h), opt-in, needs acfg: a segment the tracker would fill on its
    canvas is first searched block by block against the held keys (vvw_search on the pyramid the tracker built), one affine map per frame is
    fitted exactly on the host (platewarp.plan_segment), and the canvas is built and read back through these maps with nearest-neighbour
    gathers (_fill_on_warp), so that the fill follows zoom and roll; a frame whose fit fails keeps its translation.  When every map is the
    tracker's translation the segment takes the tracker's canvas path unchanged ("translation"); a warped canvas over max_bytes does too
    ("fallback").  warp_out = a list that receives the call's PlateWarpReport."""
    if wcfg is not None and acfg is None:
        raise ValueError("plate_fill: wcfg (plate_warp) needs acfg (plate_align)")
    T, H, W = dil_t.shape
    cuts = tuple(int(c) for c in (cuts or ()))
    segs = tuple(span_planner.segments(T, cuts))
    boxes = hip.mask_bbox(dil_t).cpu().numpy()
    frames, dil = list(frames_rgb), dil_t
    filled, left, rotated = np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T, np.int64)
    steady, skipped = [], []
    arep = [[] for _ in range(6)]
    wrep = [[] for _ in range(8)]
    tgain, toff, tident, tn, tpath = np.ones((T, 3)), np.zeros((T, 3)), np.ones(T, bool), [], []
    for s, e in segs:
        # the segment's plan: "crop" / "canvas" fill; "empty" (no mask pixel), "skipped" (the crop is too large), "none" (no tracked frame has a mask pixel) do not
        plan, d, at = "crop", dil_t[s:e], ()
        if acfg is not None:
            pyr = [] if wcfg is not None else None
            track_t, track, cbox, path = _plan_alignment(frames_rgb[s:e], d, boxes[s:e], pcfg, acfg) if pyr is None else \
                _plan_alignment(frames_rgb[s:e], d, boxes[s:e], pcfg, acfg, pyr)
            for k, v in enumerate((track[:, :2].copy(), track[:, 2].copy(), track[:, 3] == 1, _residual(track), cbox, path)):
                arep[k].append(v)
            if path in ("none", "canvas"):
                plan = path
            if wcfg is not None:
                n, wpath, wbox, wplan = e - s, path, None, None
                nan, zero = np.full((n, 6), np.nan), np.zeros(n, np.int64)
                w = [nan, zero, zero, zero, np.zeros(n), np.zeros(n, bool)]
                if path == "canvas" and platewarp.searchable(n, H, W):
                    wplan, stats, wbox, wpath = _plan_warp(pyr[0], d, track_t, track, boxes[s:e], pcfg, acfg, wcfg)
                    fits = wplan.fits
                    w = [np.array([[float(v) for row in m for v in row] if m is not None else [np.nan] * 6 for m in wplan.maps]).reshape(n, 6),
                         stats[:, 0].copy(), stats[:, 1].copy(), np.array([len(f.kept) if f is not None else 0 for f in fits], np.int64),
                         np.array([float(f.mse) ** 0.5 if f is not None else 0.0 for f in fits]), np.array([f is not None and not f.ok for f in fits], bool)]
                    if wpath == "warp":
                        plan = "warp"
                pyr = None
                for k, v in enumerate(w + [wbox, wpath]):
                    wrep[k].append(v)
        if plan == "crop":
            box = platefill.crop_box(boxes[s:e], H, W)
            if box is None:
                plan = "empty"
            else:
                if e - s > platefill.MAX_T or platefill.crop_bytes(e - s, box) > pcfg.max_bytes:
                    plan = "skipped"
                at = (slice(box[0], box[2]), slice(box[1], box[3]))
                d = d[(slice(None),) + at].contiguous()
        steady.append(0)
        skipped.append(plan == "skipped")
        tn.append(0)
        tpath.append("canvas" if plan in ("canvas", "warp") else "skipped")
        if plan in ("none", "skipped", "canvas"):       # the masked pixels as they are; the canvas fill replaces those of its tracked frames
            left[s:e] = (d != 0).flatten(1).sum(1).cpu().numpy()
        if plan not in ("crop", "canvas", "warp"):
            continue
        if plan == "warp":
            new, d2, c, steady[-1] = _fill_on_warp(frames_rgb[s:e], d, wplan, wbox, platefill.crop_box(boxes[s:e], H, W), pcfg, gcfg)
            left[s:e] = c[:, 1]
        elif plan == "canvas":
            new, d2, c, steady[-1] = _fill_on_canvas(frames_rgb[s:e], d, track_t, track, cbox, pcfg, gcfg)
            left[s:e] = np.where(track[:, 3] == 1, c[:, 1], left[s:e])
        else:
            res = None
            if tcfg is not None:
                wbox = shadowmask.widen_box(box, H, W, tcfg.ring)
                wide = (slice(wbox[0], wbox[2]), slice(wbox[1], wbox[3]))
                if platefill.crop_bytes(e - s, wbox) <= pcfg.max_bytes and (wbox[2] - wbox[0]) * (wbox[3] - wbox[1]) <= platetone.MAX_PIXELS:
                    tpath[-1], fit, res = _fill_matched(frames_rgb[s:e], dil_t[(slice(s, e),) + wide].contiguous(), wbox, pcfg, gcfg, tcfg)
                    tn[-1] = fit.n
                    tgain[s:e] = [[f.an / f.ad for f in fs] for fs in fit.fits]
                    toff[s:e] = [[f.bn / f.bd for f in fs] for fs in fit.fits]
                    tident[s:e] = np.frombuffer(fit.identity, np.uint8) != 0
            if res is None:
                res = _fill_on_crop(frames_rgb[s:e], d, box, pcfg, gcfg)
            else:
                at = wide
            new, d2, c, steady[-1] = res
            left[s:e] = c[:, 1]
        filled[s:e], rotated[s:e] = c[:, 0], c[:, 2]
        for i, fr in new.items():
            frames[s + i] = fr
        if d2 is not None:
            if dil is dil_t:
                dil = dil_t.clone()
            dil[(slice(s, e),) + at] = d2
    if acfg is not None and align_out is not None:
        align_out.append(PlateAlignReport(*(tuple(v) for v in arep), segs))
    if wcfg is not None and warp_out is not None:
        warp_out.append(PlateWarpReport(*(tuple(v) for v in wrep), segs))
    if gcfg is not None and grain_out is not None:
        grain_out.append(PlateGrainReport(rotated, filled.copy(), segs))
    if tcfg is not None and tone_out is not None:
        tone_out.append(PlateToneReport(tgain, toff, tident, tuple(tn), tuple(tpath), segs))
    return frames, dil, PlateFillReport(filled, left, tuple(steady), tuple(skipped), segs, cuts)


def _residual(track):
    """Mean absolute luma difference of every frame's level-0 best from the records' (sad_lo, sad_hi, n); 0 where n == 0."""
    sad = track[:, 4].astype(np.int64) % (1 << 32) + (track[:, 5].astype(np.int64) << 32)
    return sad / np.maximum(track[:, 6], 1)


# ---- spans: the clip in time --------------------------------------------------------------------------------------------------------------
def clip_cuts(frames_rgb, dil_t, scfg):
    """The cuts a span setting asks for: its explicit frame indices, with cuts="auto" those spans.find_cuts reads from the device's pair
    statistics (every frame crosses to the device once for that), else None."""
    if isinstance(scfg.cuts, tuple):
        return list(scfg.cuts)
    if scfg.cuts != "auto":
        return None
    if len(frames_rgb) < 2:
        return []
    H0, W0 = frames_rgb[0].shape[:2]
    sad, n, hist = spans_hip.frame_pair_stats(frames_rgb, dil_t)
    return span_planner.find_cuts(sad, n, hist, scfg, npix=H0 * W0)


def span_plan(frames_rgb, dil_t, scfg):
    """spans.plan_spans for the dilated masks: the per-frame masked flags from mask_bbox (an empty box = unmasked) and the cuts of clip_cuts."""
    bb = hip.mask_bbox(dil_t).cpu().numpy()
    masked = (bb[:, 2] > bb[:, 0]) & (bb[:, 3] > bb[:, 1])
    return span_planner.plan_spans(masked, clip_cuts(frames_rgb, dil_t, scfg), scfg)


def _span_progress(prog, n):
    """(span, seen): span(k) is the progress callback of span k's sub-call, seen the milestones passed on so far.  10 (weights: loaded once, before
    the first span) is dropped, 20 and 50 are passed on the first time they are seen, values in (20, 50) and (50, 90] go through _share into span
    k's share with a "span k/n:" prefix.  A later span's prior runs after an earlier span's model, so a value below the largest one shown so far
    is raised to it: the caller sees each of 5 / 10 / 20 / 50 / 90 once and non-decreasing values."""
    seen, last = set(), [10]

    def show(v, s):
        if v < last[0]:
            v = last[0]
            if v in (10, 20, 50):       # nothing but a milestone shown so far: it is not shown twice
                return
        last[0] = v
        prog(v, s)

    def span(k):
        if prog is None:
            return None
        stages = {20: _share(show, "span", k, n, 20, 50), 50: _share(show, "span", k, n, 50, 90)}

        def cb(v, s=""):
            if v in stages:
                if v not in seen:
                    seen.add(v)
                    show(v, s or "running")
            elif 20 < v < 50:
                stages[20](v, s)
            elif 50 < v <= 90:              # the sub-call's own 90 closes span k's share; the call's 90 comes after the last span
                stages[50](v, s)
        return cb
    return span, seen


def run_spans(frames_rgb, dil, propainer_frames, plan, body, prog, load=None, frame0=False):
    """The temporal plan carried out: body(frames[a:b], dil[a:b], prior[a:b] | None, progress) per span (a, b), in order; every other frame is the
    original array.  One span that is the whole clip: body on the clip as it is, with the caller's progress.  No span: the original frames, no
    model (load is not called), the milestones 5 / 10 / 20 / 50 / 90 still delivered.  body is the per-clip computation (run_infill_on_frames
    passes run_clip); load loads the weights once, before the first span.  frame0=True: body also gets frame0=a, the index of its clip's first
    frame in the call (grain matching keys its noise on it: a frame gets the same field however the clip was split)."""
    T = len(frames_rgb)
    at = (lambda a: {"frame0": a}) if frame0 else (lambda a: {})
    if list(plan) == [(0, T)]:
        return body(frames_rgb, dil, propainer_frames, prog, **at(0))
    out = list(frames_rgb)
    if not plan:
        if prog is not None:
            for v, s in ((10, "no masked frame: no weights to load"), (20, "no masked frame: no prior"), (50, "no masked frame: no inference"),
                         (90, "returning the original frames")):
                prog(v, s)
        return out
    if prog is not None: prog(10, "loading weights")
    if load is not None:
        load()
    span, seen = _span_progress(prog, len(plan))
    for k, (a, b) in enumerate(plan):
        out[a:b] = body(frames_rgb[a:b], dil[a:b], None if propainer_frames is None else propainer_frames[a:b], span(k), **at(a))
    if prog is not None:
        if 50 not in seen: prog(50, "running DiffuEraser")
        prog(90, "resizing and merging finished frames")
    return out


# ---- windows: one clip in space -----------------------------------------------------------------------------------------------------------
def region_plans(dil_t, H0, W0, feather_px, cfg):
    """roi.plan_regions for the dilated masks: tile occupancy on the device, its components on the host, then one box per (frame, component)
    from the occupied tiles only (T * K * 16 bytes come back)."""
    occ = hip.mask_tile_union(dil_t, REGION_TILE).cpu().numpy()
    labels, K, tile = roi_plan.label_tiles(occ, tile=REGION_TILE)
    if K == 0:
        return None
    ty, tx = np.nonzero(labels >= 0)
    tiles = torch.from_numpy(np.stack([ty, tx, labels[ty, tx]], axis=1).astype(np.int32)).to(dil_t.device)
    return roi_plan.plan_regions(hip.mask_bbox_tiles(dil_t, tile, tiles, K).cpu().numpy(), H0, W0, feather_px, cfg)


def run_clip(frames_rgb, dil_t, propainer_frames, rcfg, stages, prog, dev, feather_px=3, keep_unmasked_original=True,
             compat_reference_early_return=False, **seam):
    """One clip after the dilation: the windows rcfg asks for (none without it, or where the planner falls back to the full frame), run_windows,
    finish.  The whole call without spans=, and each span's call with it.  seam = finish's stage keywords, handed on as they come: a call
    without them reaches finish with none."""
    H0, W0 = frames_rgb[0].shape[:2]
    if rcfg is None:
        plans = []
    elif rcfg.max_regions > 1:
        plans = region_plans(dil_t, H0, W0, feather_px, rcfg) or []
    else:
        plan = roi_plan.plan_roi(hip.mask_bbox(dil_t).cpu().numpy(), H0, W0, feather_px, rcfg)
        plans = [] if plan is None else [plan]
    outs = run_windows(frames_rgb, list(dil_t.cpu().numpy()), propainer_frames, plans, stages, prog)
    return finish(outs, frames_rgb, dil_t, plans, feather_px, keep_unmasked_original, dev, compat_reference_early_return, **seam)


def run_windows(frames_rgb, dil, propainer_frames, plans, stages, prog):
    """Weights, then every window's prior (unless one is supplied), then every window's model, each an ordinary clip call on that window's crop of
    the frames, the masks and a supplied prior; one list of output frames per window.  No plan: one "window" that is the full frame, the lists
    as they are.  Up to one window the stages get the caller's progress as it is; several windows each get their share of (20, 50) and (50, 90)
    with a "region k/n:" prefix."""
    n = len(plans)
    crops = [p.crop for p in plans] or [lambda x: x]
    share = (lambda k, lo, hi: _share(prog, "region", k, n, lo, hi)) if n > 1 else (lambda k, lo, hi: prog)
    clips = [(crop(frames_rgb), crop(dil)) for crop in crops]      # the model, and the prior when it is computed here, see only the windows
    priors = [None if propainer_frames is None else crop(propainer_frames) for crop in crops]
    if prog is not None: prog(10, "loading weights")
    stages.load_model()
    if propainer_frames is None:                                                # reference :47-57
        stages.load_prior()
        if prog is not None: prog(20, "running propainter prior")
        priors = [stages.run_prior(f, m, share(k, 20, 50)) for k, (f, m) in enumerate(clips)]
    if prog is not None: prog(50, "running DiffuEraser")
    outs = [stages.run_model(f, m, priors[k], share(k, 50, 90)) for k, (f, m) in enumerate(clips)]
    if prog is not None: prog(90, "resizing and merging finished frames")
    return outs


def _on_device(res, n, dev, fn):
    """res[i] = fn(idx, up)[j] for idx = the frames among res[:n] that this rank holds (multi-GPU "rank0" gather: the other ranks' frames are None
    and stay None); up(frames) = frames[idx] stacked on the device; fn returns a [len(idx),H,W,3] device tensor, downloaded once.  Returns res."""
    idx = [i for i in range(n) if res[i] is not None]
    if idx:
        out = fn(idx, lambda frames: torch.from_numpy(np.stack([frames[i] for i in idx])).to(dev)).cpu().numpy()
        for j, i in enumerate(idx):
            res[i] = out[j]
    return res


def _zeros(*tail, dtype=np.float64):
    """An "empty" field of a per-window, per-frame report: (K, T) -> zeros [K,T,*tail]."""
    return lambda K, T: np.zeros((K, T) + tail, dtype)


def _merged(report, empty, parts, spans, T, K):
    """The report of a call over T frames from its clips' reports: parts[i] (what finish appended) covers the frames spans[i] = (a, b); at least
    K windows; empty = one constructor (K, T) -> array per field, for the frames and windows no part covers."""
    K = max([len(p.n) for p in parts] + [K])
    rep = report(*(field(K, T) for field in empty))
    for part, (a, b) in zip(parts, spans):
        for whole, piece in zip(rep, part):
            whole[:len(piece), a:b] = piece
    return rep


class ToneMatchReport(NamedTuple):
    """What seam tone matching applied, per window k and frame t (K = 1 for the full frame): the pixels of the frame's own ring, the gain and offset
    per channel, and the RMS of original - model and of original - (gain model + offset) over that ring (tonematch.ToneFit, stacked).  Frames
    outside every span, frames this rank does not hold and windows a span does not have are identity rows with n = 0."""
    n: np.ndarray               # [K,T] int64
    gain: np.ndarray            # [K,T,3] float64
    offset: np.ndarray          # [K,T,3] float64
    rms_before: np.ndarray      # [K,T,3] float64
    rms_after: np.ndarray       # [K,T,3] float64


def tone_report(parts, spans, T, K=1):
    """The report of a call over T frames from its clips' reports: parts[i] (finish's tone_out) covers the frames spans[i] = (a, b); at least K
    windows."""
    return _merged(ToneMatchReport, (_zeros(dtype=np.int64), lambda K, T: np.ones((K, T, 3)), _zeros(3), _zeros(3), _zeros(3)), parts, spans, T, K)


class GrainMatchReport(NamedTuple):
    """What seam grain matching measured and added, per window k, frame t, channel and brightness band (K = 1 for the full frame): the counted
    pixels of the frame's own ring, the grain (sigma, 8-bit levels) of the original and of the model's rendering over the pooled ring, and the
    sigma of the noise added (grainmatch.GrainFit, stacked).  Frames outside every span, frames this rank does not hold and windows a span does
    not have are zero rows."""
    n: np.ndarray               # [K,T,3,4] int64
    sigma_orig: np.ndarray      # [K,T,3,4] float64
    sigma_model: np.ndarray     # [K,T,3,4] float64
    sigma_added: np.ndarray     # [K,T,3,4] float64


def grain_report(parts, spans, T, K=1):
    """The report of a call over T frames from its clips' reports: parts[i] (finish's grain_out) covers the frames spans[i] = (a, b); at least K
    windows."""
    return _merged(GrainMatchReport, (_zeros(3, grainmatch.BANDS, dtype=np.int64),) + (_zeros(3, grainmatch.BANDS),) * 3, parts, spans, T, K)


class SeamBlendReport(NamedTuple):
    """What seam membrane blending measured and added, per window k and frame t (K = 1 for the full frame): the ring pixels that gave data, the
    RMS of original - model on them per channel (after tone matching's table), the pixels of the hole, and the largest and the mean |membrane|
    inside the hole per channel, in 8-bit levels before `strength` (seamblend.SeamBlendFit, stacked: closed forms of exact integer sums).
    Frames outside every span, frames this rank does not hold and windows a span does not have are zero rows."""
    n: np.ndarray               # [K,T] int64
    rms_diff: np.ndarray        # [K,T,3] float64
    n_hole: np.ndarray          # [K,T] int64
    max_shift: np.ndarray       # [K,T,3] float64
    mean_shift: np.ndarray      # [K,T,3] float64


def seam_blend_report(parts, spans, T, K=1):
    """The report of a call over T frames from its clips' reports: parts[i] (finish's blend_out) covers the frames spans[i] = (a, b); at least K
    windows."""
    return _merged(SeamBlendReport, (_zeros(dtype=np.int64), _zeros(3), _zeros(dtype=np.int64), _zeros(3), _zeros(3)), parts, spans, T, K)


class DeflickerReport(NamedTuple):
    """What the inpaint deflicker did, per window k and frame t (K = 1 for the full frame), over the whole window and over its masked pixels
    (`_mask`): the pixels counted, the pixels with any byte changed, the mean number of accepted samples and the mean |out - in| per channel in
    8-bit levels (deflicker.DeflickerFit, stacked: closed forms of exact integer sums).  Frames outside every span, frames this rank does not
    hold and windows a span does not have are zero rows."""
    n: np.ndarray               # [K,T] int64
    changed: np.ndarray         # [K,T] int64
    samples: np.ndarray         # [K,T] float64
    shift: np.ndarray           # [K,T,3] float64
    n_mask: np.ndarray          # [K,T] int64
    changed_mask: np.ndarray    # [K,T] int64
    samples_mask: np.ndarray    # [K,T] float64
    shift_mask: np.ndarray      # [K,T,3] float64


def deflicker_report(parts, spans, T, K=1):
    """The report of a call over T frames from its clips' reports: parts[i] (finish's flicker_out) covers the frames spans[i] = (a, b); at least K
    windows."""
    return _merged(DeflickerReport, (_zeros(dtype=np.int64), _zeros(dtype=np.int64), _zeros(), _zeros(3)) * 2, parts, spans, T, K)


class DeflickerAlignReport(NamedTuple):
    """What the tracker of finish(flicker_align=) found, per clip call of `segments` (a tuple each; the spans of the call, (0, T) without spans):
    off [n,2] int32 = the frame's (x, y) on the canvas in which the background stands still, key [n] = the key frame it was tracked against,
    tracked [n] bool (a lost frame is left unfiltered), residual [n] = the mean absolute luma difference of its level-0 best (0 for frame 0 and
    a lost frame), and the path that ran: "tracked" (flickalign_hip.hold), "static" (one frame, or every frame tracked at offset zero: the
    unaligned filter as it is), "untracked" (the clip is beyond the tracker's limits: the unaligned filter) or "none" (this rank holds no
    frame of the clip call: nothing tracked, nothing filtered)."""
    off: tuple
    key: tuple
    tracked: tuple
    residual: tuple
    path: tuple
    segments: tuple


def deflicker_align_report(parts, spans):
    """The report of a call from its clips' records: parts[i] (finish's flicker_align_out) = (track [n,8] on the host, path) of the clip call
    over the frames spans[i] = (a, b)."""
    cols = [(tr[:, :2].copy(), tr[:, 2].copy(), tr[:, 3] == 1, _residual(tr), path) for tr, path in parts]
    return DeflickerAlignReport(*(tuple(c) for c in ([list(v) for v in zip(*cols)] or [[] for _ in range(5)])), tuple(tuple(s) for s in spans))


class DeflickerLocalReport(NamedTuple):
    """What the block matching of finish(flicker_local=) found, per window k and frame t (K = 1 for the full frame), over the frame's temporal
    neighbours: the block and neighbour pairs that got a vector, how many of those vectors are not zero, the mean |dy| + |dx| and the largest
    max(|dy|, |dx|) over the matched ones, and the winners' summed cost against the zero candidate's where that one was valid
    (deflickerlocal.DeflickerLocalFit, stacked: exact integer sums).  What the gate then accepted stands in the DeflickerReport.  Frames outside
    every span, frames this rank does not hold, windows a span does not have and calls with radius = 0 are zero rows."""
    blocks: np.ndarray          # [K,T] int64
    moved: np.ndarray           # [K,T] int64
    mean_vector: np.ndarray     # [K,T] float64
    max_vector: np.ndarray      # [K,T] int64
    cost: np.ndarray            # [K,T] int64
    cost_zero: np.ndarray       # [K,T] int64
    n = property(lambda self: self.blocks)      # what _merged sizes the windows by


def deflicker_local_report(parts, spans, T, K=1):
    """The report of a call over T frames from its clips' reports: parts[i] (finish's flicker_local_out) covers the frames spans[i] = (a, b); at
    least K windows."""
    i64 = _zeros(dtype=np.int64)
    return _merged(DeflickerLocalReport, (i64, i64, _zeros(), i64, i64, i64), parts, spans, T, K)


class DetailMatchReport(NamedTuple):
    """What seam detail matching measured and applied, per window k and frame t (K = 1 for the full frame): the counted pixels of the frame's own
    ring, the amount of the model's own high-pass added (negative: taken away; 0: the frame is left as it is), the mean of (H(original) -
    H(model))^2 over that ring before the stage, and whether the cap cut the fit or the dead zone took it for 0 (detailmatch.DetailFit,
    stacked).  Frames outside every span, frames this rank does not hold and windows a span does not have are zero rows."""
    n: np.ndarray               # [K,T] int64
    amount: np.ndarray          # [K,T] float64
    residual: np.ndarray        # [K,T] float64
    clamped: np.ndarray         # [K,T] bool
    dead: np.ndarray            # [K,T] bool


def detail_report(parts, spans, T, K=1):
    """The report of a call over T frames from its clips' reports: parts[i] (finish's detail_out) covers the frames spans[i] = (a, b); at least K
    windows."""
    return _merged(DetailMatchReport, (_zeros(dtype=np.int64), _zeros(), _zeros(), _zeros(dtype=bool), _zeros(dtype=bool)), parts, spans, T, K)


class GrainShapeReport(NamedTuple):
    """What grain shape fitted, per window k and frame t (K = 1 for the full frame).  Per channel and axis (0 = x, 1 = y): the counted pairs of
    the frame's own ring, rho = the lag-1 correlation of the grain's response to Immerkaer's operator over the pooled ring, the a of the
    shaping kernel [a, 1, a] that was applied (0: white), and whether the fit was cut at an end of [0, max_a] or fell into the dead zone.  Per
    channel: k, the factor by which the white estimate of the level was raised.  Per channel and band: the sigma of the shaped noise added, at
    pixel scale (grainshape.GrainShapeFit, stacked).  Frames outside every span, frames this rank does not hold and windows a span does not
    have are zero rows with k = 1."""
    pairs: np.ndarray           # [K,T,3,2] int64
    rho: np.ndarray             # [K,T,3,2] float64
    a: np.ndarray               # [K,T,3,2] float64
    k: np.ndarray               # [K,T,3] float64
    sigma_pixel: np.ndarray     # [K,T,3,4] float64
    clamped: np.ndarray         # [K,T,3,2] bool
    dead: np.ndarray            # [K,T,3,2] bool
    n = property(lambda self: self.pairs)       # what _merged sizes the windows by


def grain_shape_report(parts, spans, T, K=1):
    """The report of a call over T frames from its clips' reports: parts[i] (finish's grain_shape_out) covers the frames spans[i] = (a, b); at
    least K windows."""
    return _merged(GrainShapeReport, (_zeros(3, 2, dtype=np.int64), _zeros(3, 2), _zeros(3, 2), lambda K, T: np.ones((K, T, 3)),
                                      _zeros(3, grainmatch.BANDS), _zeros(3, 2, dtype=bool), _zeros(3, 2, dtype=bool)), parts, spans, T, K)


def finish(outs, frames_rgb, dil_t, plans, feather_px, keep_unmasked_original, dev, compat_reference_early_return=False, tone=None, tone_out=None,
           grain=None, grain_out=None, grain_shape=None, grain_shape_out=None, frame0=0, blend=None, blend_out=None, flicker=None, flicker_out=None, flicker_local=None, flicker_local_out=None,
           flicker_align=None, flicker_align_out=None, detail=None, detail_out=None):
    """The model's frames into frames of the original size.  No plan and no stage (full_frame; reference :69-112): resize when the model ran
    at another size, feathered composite with the originals when keep_unmasked_original, in place in outs[0].  The reference returns from
    inside its loop (:114) so only frame 0 is post-processed; the evident intent (all frames) is the default here,
    compat_reference_early_return=True reproduces the quirk.
    Otherwise ONE loop over the windows (pasted) -- with plans theirs, without the full frame as the window (0, 0, H0, W0) -- the output of
    window k the original of window k + 1: two buffers, one upload, one download.  Exact because the windows are disjoint: inside window k the
    mask holds only region k's pixels and no other window has touched the bytes.  Per window: its model frames to the device (model_px), the
    stages that are on, then the ONE fused call that resizes to the window, pastes and composites (keep_unmasked_original=False: the plain
    paste, and every pasted pixel goes through the stages).  A stage that is off calls nothing and resolves no symbol of its binding; each
    stage's per-clip report is appended to its *_out list.
      tone (a tonematch.ToneMatchConfig): ring_stats of the model's pixels against the running buffer (inside window k still
        the original bytes), the [T,16] sums to the host, tonematch.fit and tables, the [T,3,256] tables to the device.  Without tone the
        later stages get the identity table.
      grain (a grainmatch.GrainMatchConfig): ring_grain_stats of the looked-up pixels, the [T,36] sums to the host,
        grainmatch.fit and tables, the [T,3,256] amplitudes to the device; the noise is keyed on the frame's index in the call, frame0 + its
        index in this clip.
      blend (a seamblend.SeamBlendConfig): blend_hip.solve of the looked-up pixels against the running buffer gives the
        membrane, over groups of frames (seamblend.groups) that share one scratch buffer; it is added after the table and before the grain
        (zero amplitudes without grain, whose statistic stays on the tabled pixel without the membrane).  In front of it the tone stage fits
        the offset alone, gain 1, whatever tone.mode says: a shift that varies round the ring misleads a gain.
    The window ends in hip.roi_paste_composite (no stage), tone_hip.paste_lut_composite (tone alone), grain_hip.paste_grain_composite (grain,
    with or without tone) or, with blend, blend_hip.paste_blend_composite group by group.
    flicker (a deflicker.DeflickerConfig): per window, where its model frames are uploaded (model_px): the window's pixels
    materialised at the window's size (flicker_hip.window_pixels), filtered along time inside this clip call (flicker_hip.hold; rules:
    include/vvflicker.h); everything above then reads the filtered [n,h,w,3] patch at equal size with the same offsets, so tone, membrane and
    grain measure the filtered rendering.  Two more window-sized clip buffers live on the device meanwhile.  A rank holds every frame of the
    clip or none.  The clip's DeflickerReport is appended to flicker_out.  Without flicker model_px is the upload, nothing here changes and
    no vvf_ symbol is resolved.
    flicker_align (a platealign.PlateAlignConfig, with flicker; rules: include/vvflickalign.h): the first model_px of the clip
    call tracks one integer translation per frame on the call's own frames and dilated masks (_track_segment: the pyramid in batches of
    deflickeralign.TRACK_BYTES, one synchronisation); the track stays on the device and serves every window, whose neighbours are then read
    along it (flickalign_hip.hold in place of flicker_hip.hold).  A clip beyond the tracker's limits ("untracked"), a single frame and a clip
    whose frames all sit at offset zero ("static") take the unaligned filter exactly as above, fixed form included.  A frame the tracker
    loses (after a cut inside the clip call: every later frame) stays unfiltered.  (track, path) of the clip call is appended to
    flicker_align_out (deflicker_align_report).  Without flicker_align nothing here changes and no vvc_ symbol is resolved.
    flicker_local (a deflickerlocal.DeflickerLocalConfig, with flicker; rules: include/flicklocal.h): in model_px, after
    window_pixels and with flicker.radius > 0, flicklocal_bind.search finds one displacement per block and temporal neighbour on the window's
    own pixels and flicklocal_bind.hold filters along them, in place of flicker_hip.hold / flickalign_hip.hold; the track is flicker_align's
    when its path is "tracked", else none (the binding's zero track).  The vectors stay on the device; the [T,2 radius+1,6] statistics come to
    the host beside the filter's sums.  The clip's DeflickerLocalReport is appended to flicker_local_out.  With radius = 0 the path above
    runs as it is.  Without flicker_local nothing here changes and no vvk_ symbol is resolved.
    detail (a detailmatch.DetailMatchConfig; rules: include/detailmatch.h): a seam stage, so the full frame takes the loop as
    the window (0, 0, H0, W0).  Per window, directly after model_px (after the deflicker): ring_detail_stats of the model's pixels against the
    running buffer, the [T,12] sums to the host (one synchronisation), detailmatch.fit, the [T] amounts to the device, and
    detailmatch_bind.sharpen materialises the window's pixels at the window's size with that amount of their own high-pass added or taken
    away; everything above then reads the sharpened [n,h,w,3] patch at equal size, so tone, membrane and grain measure the sharpened
    rendering and the window ends in the same paste call.  One more window-sized clip buffer lives on the device meanwhile.  The clip's
    DetailMatchReport is appended to detail_out.  Without detail nothing here changes and no vvd_ symbol is resolved.
    grain_shape (a grainshape.GrainShapeConfig, with grain; rules: include/grainshape.h): per window,
    grainshape_bind.ring_shape_stats runs next to ring_grain_stats on the same looked-up pixels -- both are launched, then both [T,36] and
    [T,30] sums come to the host behind the one synchronisation --, grainshape.fit gives the taps and the amplitudes of the white noise in
    front of the shaping kernel, and the window ends in grainshape_bind.paste_shaped_composite, with or without blend's membrane.  The clip's
    GrainShapeReport is appended to grain_shape_out; grain_out gets grain matching's own fit, whose sigma_added is then the white estimate and
    not what was added.  Without grain_shape nothing here changes and no vvn_ symbol is resolved."""
    if grain_shape is not None and grain is None:
        raise ValueError("finish: grain_shape shapes the noise grain adds and needs it")
    if flicker_local is not None and flicker is None:
        raise ValueError("finish: flicker_local gives the deflicker its vectors and needs flicker")
    H0, W0 = frames_rgb[0].shape[:2]
    T = len(outs[0])
    fsums = []      # deflicker: the [T,12] sums of every window filtered so far
    lstats = []     # deflicker_local: the [T,2 radius+1,6] statistics of every window searched so far
    ftrack = []     # deflicker_align: (track on the device | None, track on the host, path) of this clip call, found by the first model_px

    def tracked():
        if not ftrack:
            if not platealign.trackable(T, H0, W0):
                ftrack.append((None, deflickeralign.identity_track(T), "untracked"))
            elif T == 1:
                ftrack.append((None, deflickeralign.identity_track(T), "static"))
            else:
                track_t, track = _track_segment(frames_rgb, dil_t, flicker_align, deflickeralign.TRACK_BYTES)
                ftrack.append((track_t, track, deflickeralign.path_of(track)))
        return ftrack[0]

    def model_px(o, idx, up, offsets=None, size=None, offs=None, mask=None):
        """Window frames o of the model on the device.  With flicker: as the window's h x w pixels (size; offsets [T,2] = the window's place per
        frame, None = the full frame), filtered along time; offs / mask = offsets[idx] and dil_t[idx] where the caller has them on the device."""
        if flicker is None:
            return up(o).contiguous()
        if len(idx) != T:
            raise RuntimeError(f"deflicker: a rank holds every frame of a clip call or none, not {len(idx)} of {T}")
        h, w = size or (H0, W0)
        place = np.zeros((T, 2), np.int32) if offsets is None else np.ascontiguousarray(offsets[idx], np.int32)
        win = flicker_hip.window_pixels(up(o).contiguous(), h, w)
        offs = torch.from_numpy(place).to(dev) if offs is None else offs
        mask = dil_t[idx].contiguous() if mask is None else mask
        if flicker_local is not None and flicker.radius > 0:
            track = tracked()[0] if flicker_align is not None and tracked()[2] == "tracked" else None
            mv, stats = flicklocal_bind.search(win, offs, track, flicker.radius, flicker_local)
            held, sums = flicklocal_bind.hold(win, offs, track, mv, mask, flicker.radius, flicker_local.block, flicker.tol)
        elif flicker_align is not None and tracked()[2] == "tracked":
            held, sums = flickalign_hip.hold(win, offs, tracked()[0], mask, flicker.radius, flicker.tol)
        else:
            held, sums = flicker_hip.hold(win, offs, mask, flicker.radius, flicker.tol, fixed=bool((place == place[0]).all()))
        fsums.append(sums.cpu().numpy())
        if flicker_local is not None:
            lstats.append(stats.cpu().numpy() if flicker.radius > 0 else np.zeros((T, 1, deflickerlocal.NSTAT), np.int64))
        return held

    def full_frame(idx, up):
        out = model_px(outs[0], idx, up)
        if tuple(out.shape[1:3]) != (H0, W0):
            out = hip.resize_u8(out.contiguous(), H0, W0, mode="bilinear")          # cv2.resize(f,(W0,H0)), :73
        if keep_unmasked_original:
            out = hip.feather_composite(out.contiguous(), up(frames_rgb).contiguous(), dil_t[idx].contiguous(), float(feather_px))   # :77-112
        return out

    seam = tone is not None or grain is not None or blend is not None or detail is not None
    feather = float(feather_px if keep_unmasked_original else -1.0)

    def pasted(idx, up):
        n = len(idx)
        wins = [(p.offsets, p.size) for p in plans] or [(np.zeros((T, 2), np.int32), (H0, W0))]
        bufs = [up(frames_rgb).contiguous()]
        bufs.append(torch.empty_like(bufs[0]))
        mask = dil_t[idx].contiguous()
        if grain is not None or blend is not None:
            ids = torch.from_numpy(np.asarray(idx, np.int32) + np.int32(frame0)).to(dev)
            ident = np.broadcast_to(np.arange(256, dtype=np.uint8), (n, 3, 256))
            seed, mode = (0, 0) if grain is None else (grain.seed, grainmatch.MODES.index(grain.mode))
            if grain is None:
                amp = torch.zeros((n, 3, 256), dtype=torch.uint8, device=dev)
        # a shift that varies round the ring is correlated with the picture there and misleads a fitted gain; what varies is the membrane's to
        # take, so in front of it the tone stage fits the offset alone
        tone_cfg = tone if tone is None or blend is None else dataclasses.replace(tone, mode="offset")
        tfits, gfits, bfits, dfits, nfits = [], [], [], [], []

        def whole(rows):        # [n,nsum] of this rank's frames -> [T,nsum], zero rows for the others
            sums = np.zeros((T, rows.shape[1]), np.int64)
            sums[idx] = rows
            return sums

        for k, ((offsets, (h, w)), o) in enumerate(zip(wins, outs)):
            src, dst = bufs[k % 2], bufs[(k + 1) % 2]
            offs = torch.from_numpy(np.ascontiguousarray(offsets[idx], np.int32)).to(dev)
            patch = model_px(o, idx, up, offsets, (h, w), offs, mask)
            if detail is not None:
                rows = detailmatch_bind.ring_detail_stats(patch, src, mask, offs, h, w, detail.ring, detail.edge).cpu().numpy()
                dfits.append(detailmatch.held_rows(detailmatch.fit(whole(rows), detail), idx))
                amounts = torch.from_numpy(detailmatch.q8(dfits[-1].amount[idx])).to(dev)
                patch = detailmatch_bind.sharpen(patch, amounts, h, w, detail.overshoot)
            if tone is not None:
                tfits.append(tonematch.fit(whole(tone_hip.ring_stats(patch, src, mask, offs, h, w, tone.ring).cpu().numpy()), tone_cfg))
                lut = torch.from_numpy(tonematch.tables(tfits[-1].gain[idx], tfits[-1].offset[idx])).to(dev)
            elif grain is not None or blend is not None:
                lut = torch.from_numpy(np.ascontiguousarray(ident)).to(dev)
            if grain is not None:
                rows = grain_hip.ring_grain_stats(patch, src, mask, offs, lut, h, w, grain.ring, grain.flat)
                if grain_shape is not None:                                               # launched before the download: one synchronisation for both
                    pairs = grainshape_bind.ring_shape_stats(patch, src, mask, offs, lut, h, w, grain.ring, grain.flat)
                rows = rows.cpu().numpy()
                gfits.append(grainmatch.fit(whole(rows), grain))
                if grain_shape is not None:
                    shaped = grainshape.fit(whole(pairs.cpu().numpy()), whole(rows), grain, grain_shape)
                    nfits.append(shaped[:7])
                    amp, taps = torch.from_numpy(shaped.amp[idx]).to(dev), torch.from_numpy(np.ascontiguousarray(shaped.taps[idx])).to(dev)
                else:
                    amp = torch.from_numpy(grainmatch.tables(gfits[-1].sigma_added[idx])).to(dev)
            if blend is not None:
                rows, scratch = [], None
                for a, b in seamblend.groups(n, h, w):
                    if scratch is None:
                        scratch = torch.empty((seamblend.scratch_bytes(b - a, h, w),), dtype=torch.uint8, device=dev)
                    field, _, part = blend_hip.solve(patch[a:b], src[a:b], mask[a:b], offs[a:b], lut[a:b], h, w, blend.ring, blend.presmooth,
                                                     blend.sweeps, blend.max_shift, scratch=scratch)
                    rows.append(part.cpu().numpy())
                    if grain_shape is not None:
                        grainshape_bind.paste_shaped_composite(patch[a:b], src[a:b], mask[a:b], offs[a:b], lut[a:b], field, blend.strength_q8, amp[a:b],
                                                               taps[a:b], ids[a:b], seed, mode, h, w, feather, out=dst[a:b])
                    else:
                        blend_hip.paste_blend_composite(patch[a:b], src[a:b], mask[a:b], offs[a:b], lut[a:b], field, blend.strength_q8, amp[a:b],
                                                        ids[a:b], seed, mode, h, w, feather, out=dst[a:b])
                bfits.append(seamblend.fit(whole(np.concatenate(rows))))
            elif grain_shape is not None:
                grainshape_bind.paste_shaped_composite(patch, src, mask, offs, lut, None, 0, amp, taps, ids, seed, mode, h, w, feather, out=dst)
            elif grain is not None:
                grain_hip.paste_grain_composite(patch, src, mask, offs, lut, amp, ids, seed, mode, h, w, feather, out=dst)
            elif tone is not None:
                tone_hip.paste_lut_composite(patch, src, mask, offs, lut, h, w, feather, out=dst)
            else:
                hip.roi_paste_composite(patch, src, mask, offs, h, w, feather, out=dst)
        for fits, out, report in ((tfits, tone_out, ToneMatchReport), (gfits, grain_out, GrainMatchReport), (bfits, blend_out, SeamBlendReport),
                                  (dfits, detail_out, DetailMatchReport), (nfits, grain_shape_out, GrainShapeReport)):
            if fits and out is not None:
                out.append(report(*(np.stack(f) for f in zip(*fits))))
        return bufs[len(wins) % 2]

    if seam or plans:
        asked = [(out, empty, len(out)) for cfg, out, empty in ((tone, tone_out, tone_report), (grain, grain_out, grain_report),
                                                                 (blend, blend_out, seam_blend_report), (detail, detail_out, detail_report),
                                                                 (grain_shape, grain_shape_out, grain_shape_report))
                 if cfg is not None and out is not None]
        res = _on_device(list(outs[0]) if plans else outs[0], T, dev, pasted)
        for out, empty, before in asked:
            if len(out) == before:                                                        # this rank holds no frame of the clip: identity / zero rows
                out.append(empty([], [], T, K=max(len(plans), 1)))
    else:
        res = _on_device(outs[0], 1 if compat_reference_early_return else T, dev, full_frame)
    if flicker is not None and flicker_out is not None:
        if fsums:
            flicker_out.append(DeflickerReport(*(np.stack(f) for f in zip(*(deflicker.fit(s) for s in fsums)))))
        else:                                                                             # this rank holds no frame of the clip: zero rows
            flicker_out.append(deflicker_report([], [], T, K=max(len(plans), 1)))
    if flicker_local is not None and flicker_local_out is not None:
        if lstats:
            flicker_local_out.append(DeflickerLocalReport(*(np.stack(f) for f in zip(*(deflickerlocal.fit(s) for s in lstats)))))
        else:                                                                             # this rank holds no frame of the clip: zero rows
            flicker_local_out.append(deflicker_local_report([], [], T, K=max(len(plans), 1)))
    if flicker_align is not None and flicker_align_out is not None:                       # no model_px on this rank: nothing tracked
        flicker_align_out.append(ftrack[0][1:] if ftrack else (deflickeralign.identity_track(T), "none"))
    return res

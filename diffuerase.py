"""Drop-in replacement for the reference module `diffuerase` (reference diffuerase.py:1-158): same module name, same
`run_infill_on_frames` signature and CLI, so `videovanish.py` (reference :46,1518,1593) keeps working unchanged --
with the hot path running on hand-written gfx950 HIP kernels (videovanish_amd/) instead of torch/cuDNN.

Extra keyword-only knobs (old callers are unaffected): num_inference_steps, scheduler, chunk, overlap, dtype, seed,
compat_reference_early_return, roi (mask-region inference: videovanish_amd/roi.py; also configure(roi=...) and $VV_ROI), spans / cuts (mask-span
inference: only the runs of masked frames are processed, and nothing crosses a hard cut: videovanish_amd/spans.py; also configure(spans=...) and
$VV_SPANS).  There is no CPU fallback: without the HIP extension / a GPU this raises.
"""
import argparse
import os

import numpy as np
import torch

from videovanish_amd import hip
from videovanish_amd import roi as roi_plan
from videovanish_amd import spans as span_plan
from videovanish_amd import spans_hip
from videovanish_amd.config import RunConfig
from videovanish_amd.diffueraser import DiffuEraser
from videovanish_amd.propainter import Propainter, get_device

# module-level singletons, as in the reference (diffuerase.py:15-18): not re-entrant, one worker thread at a time
device = None
last_ckpt = None
video_inpainting_sd = None
propainter = None
_run_config = None      # set through configure(); None = full SD-1.5 / sd-vae-ft-mse shapes
_dist = None
_gather = "all"
_prior_stages = {}      # configure(prior=...): optional learned stages of the ProPainter prior (flow_completion, generator)
_weights = None         # configure(weights=...) / $VV_WEIGHTS_DIR: a local model store (videovanish_amd/modelhub.py) or a CheckpointWeights
_loaded = None          # (CheckpointWeights, prior stages) resolved from _weights, cached until configure() is called again
_roi = None             # configure(roi=...): mask-region inference for calls that do not pass roi= themselves
_spans = None           # configure(spans=...): mask-span inference for calls that do not pass spans= themselves


def configure(run: RunConfig = None, dist=None, gather="all", prior=None, weights=None, reference_defaults=False, roi=None, spans=None):
    """Select architecture / chunking / dtype for subsequently constructed models (tests use small configs).
    dist = (rank, world) with torch.distributed initialised, one process per GPU (torchrun); gather = "all": every rank returns
    every frame; "rank0": only rank 0 does (the other ranks get None for frames they do not own and should not write a file).
    prior = {"flow_completion": bool, "generator": bool}: run the learned stages of the full ProPainter prior (videovanish_amd/propainter.py).
    weights = a directory holding the four checkpoints the reference names (reference :41-43,49; layout: videovanish_amd/modelhub.py), or a
    checkpoint.CheckpointWeights.  Without it (and without $VV_WEIGHTS_DIR) the models are seeded random-init of the same architecture.
    With it every tensor is checked against the architecture first, the empty prompt is CLIP-encoded once, the PCM "2-Step" LoRA is merged,
    and the learned ProPainter stages switch ON when their files are present (unless `prior` says otherwise).
    reference_defaults=True: ONE switch for the computation the reference app runs by default (reference diffuerase.py:20-21,37,47-57 + the third-party
    forward): the pipeline's own temporal scheme (22-frame windows shifted on odd steps, value / count averaging, key-frame pre-inference:
    RunConfig.windowing="reference", one GPU), the 2-step TCD schedule of the "2-Step" checkpoint (already the default of this module), and the
    COMPLETE ProPainter prior (recurrent flow completion + inpainting generator) when no prior is handed over -- instead of this build's defaults
    (independent 32 / 8 chunks that shard over GPUs; RAFT + propagation only).  `run` / `prior` given explicitly still win field by field.
    roi = None / "static" / "follow" / "static-regions" / "follow-regions" / a roi.RoiConfig: mask-region inference for calls that do not pass
    roi= (run_infill_on_frames).
    spans = None / "masked" / "cuts" / "masked-cuts" / a spans.SpanConfig: mask-span inference for calls that do not pass spans=."""
    global _run_config, _dist, _gather, last_ckpt, _prior_stages, propainter, _weights, _loaded, _roi, _spans
    span_plan.as_config(spans)
    roi_plan.as_config(roi)                 # validated now, kept as given: configure(roi="off") means the full frame whatever $VV_ROI says
    if reference_defaults:
        import dataclasses
        run = dataclasses.replace(run or RunConfig(), windowing="reference")
        prior = dict({"flow_completion": True, "generator": True}, **(prior or {}))
    _run_config, _dist, _gather, last_ckpt = run, dist, gather, None
    _prior_stages, propainter = dict(prior or {}), None
    _weights, _loaded = weights, None
    _roi = roi
    _spans = spans


def _resolve_weights(ckpt):
    """(weight source | None, prior stages) for the configured / environment-named model store."""
    global _loaded
    src = _weights if _weights is not None else os.environ.get("VV_WEIGHTS_DIR")
    if src is None:
        return None, dict(_prior_stages)
    if _loaded is None:
        if isinstance(src, (str, os.PathLike)):
            from videovanish_amd import modelhub
            run = _run_config or RunConfig()
            _loaded = modelhub.load(os.fspath(src), ckpt=ckpt, ucfg=run.unet, vcfg=run.vae)
        else:
            _loaded = (src, {"flow_completion": "fc" in src.components, "generator": "gen" in src.components and "fc" in src.components})
    w, stages = _loaded
    stages = dict(stages)
    stages.update(_prior_stages)            # an explicit configure(prior=...) wins
    return w, stages


def roi_config(roi=None):
    """The mask-region setting a call runs with: its own roi= argument, else configure(roi=...), else $VV_ROI (static | follow | static-regions |
    follow-regions | off).
    None = full frame.  roi="off" (or False) asks for the full frame whatever configure() or the environment say."""
    if roi is not None:
        return roi_plan.as_config(roi)
    if _roi is not None:
        return roi_plan.as_config(_roi)
    return roi_plan.as_config(os.environ.get("VV_ROI"))


def spans_config(spans=None, cuts=None):
    """The mask-span setting a call runs with: its own spans= argument, else configure(spans=...), else $VV_SPANS (masked | cuts | masked-cuts | off).
    None = the full clip.  spans="off" (or False) asks for the full clip whatever configure() or the environment say.  cuts (frame indices) replaces
    the setting's own cuts: explicit cuts always override the detector; given alone it means "every frame, split at these cuts"."""
    if spans is not None:
        cfg = span_plan.as_config(spans)
    elif _spans is not None:
        cfg = span_plan.as_config(_spans)
    else:
        cfg = span_plan.as_config(os.environ.get("VV_SPANS"))
    if cuts is not None and not (spans is not None and cfg is None):        # spans="off" wins over cuts=
        import dataclasses
        cfg = span_plan.SpanConfig("all", cuts=cuts) if cfg is None else dataclasses.replace(cfg, cuts=cuts)
    return cfg


def run_infill_on_frames(frames_rgb, mask_frames, mask_dilation_iter=8, ckpt="2-Step",
                         propainer_frames=None, max_img_size=960, keep_unmasked_original=True, feather_px=3, prog=None,
                         *, num_inference_steps=None, scheduler=None, compat_reference_early_return=False, roi=None, spans=None, cuts=None):
    """roi (mask-region inference, opt-in): "static" / "follow" / a videovanish_amd.roi.RoiConfig crops every frame to a window around the dilated
    masks, runs the prior and the model on that smaller clip and pastes the result back into the original frames: pixels outside the window are
    the original bytes.  Falls back to the full frame when no frame has a mask pixel or the window would be the whole frame.
    "static-regions" / "follow-regions" (RoiConfig.max_regions > 1): one window per separate masked region (roi.plan_regions), each region an
    ordinary clip call on its crop, the windows pasted one after another; with one region left this is the single-window path.
    spans (mask-span inference, opt-in): "masked" / "cuts" / "masked-cuts" / a videovanish_amd.spans.SpanConfig splits the clip in time
    (spans.plan_spans): at hard cuts (cuts=[...] frame indices, or found on the device: "cuts", "masked-cuts"), and in "masked" mode into spans
    around the runs of masked frames only.  Each span is this call on frames[a:b] (its own roi windows, chunks and lanes); frames outside every
    span are returned as the original arrays, also with keep_unmasked_original=False.  A clip without a mask pixel returns its input and loads
    no model; one span that is the whole clip is the plain call."""
    rcfg = roi_config(roi)
    scfg = spans_config(spans, cuts)
    if rcfg is not None and compat_reference_early_return:
        raise ValueError("roi= (mask-region inference) cannot be combined with compat_reference_early_return=True")
    if scfg is not None and compat_reference_early_return:
        raise ValueError("spans= (mask-span inference) cannot be combined with compat_reference_early_return=True")

    if prog is not None: prog(5, "dilating frames")
    dev = get_device()
    m = torch.from_numpy(np.stack([mm if mm.ndim == 3 else mm[..., None] for mm in mask_frames])).to(dev)
    dil_t = hip.mask_collapse_dilate(m.contiguous(), mask_dilation_iter)       # reference :27-31

    def body(frames, dil, prior, p):
        return _clip_body(frames, dil, prior, rcfg, ckpt, dev, max_img_size, keep_unmasked_original, feather_px, p, num_inference_steps, scheduler,
                          compat_reference_early_return)

    if scfg is None:
        return body(frames_rgb, dil_t, propainer_frames, prog)
    plan = _span_plan(frames_rgb, dil_t, scfg)
    return _run_spans(frames_rgb, dil_t, propainer_frames, plan, body, prog, load=lambda: _load_model(dev, ckpt))


def _span_plan(frames_rgb, dil_t, scfg):
    """spans.plan_spans for the dilated masks: the per-frame masked flags from mask_bbox (an empty box = unmasked) and, with cuts="auto", the cuts
    spans.find_cuts reads from the device's pair statistics (every frame crosses to the device once for that)."""
    bb = hip.mask_bbox(dil_t).cpu().numpy()
    masked = (bb[:, 2] > bb[:, 0]) & (bb[:, 3] > bb[:, 1])
    cuts = None
    if scfg.cuts == "auto":
        cuts = []
        if len(frames_rgb) >= 2:
            H0, W0 = frames_rgb[0].shape[:2]
            sad, n, hist = spans_hip.frame_pair_stats(frames_rgb, dil_t)
            cuts = span_plan.find_cuts(sad, n, hist, scfg, npix=H0 * W0)
    return span_plan.plan_spans(masked, cuts, scfg)


def _span_progress(prog, k, n, state):
    """Progress of span k's sub-call: 10 (weights: loaded once, before the first span) is dropped, 20 and 50 are passed on the first time
    they are seen, values in (20, 50) and (50, 90] go through _region_progress's mapping into span k's share with a "span k/n:" prefix.  A later
    span's prior runs after an earlier span's model, so a value below the largest one shown so far is raised to it: the caller sees each of
    5 / 10 / 20 / 50 / 90 once and non-decreasing values."""
    if prog is None:
        return None

    def show(v, s):
        if v < state["last"]:
            v = state["last"]
            if v in (10, 20, 50):       # nothing but a milestone shown so far: it is not shown twice
                return
        state["last"] = v
        prog(v, s)

    stages = {20: _region_progress(show, k, n, 20, 50, "span"), 50: _region_progress(show, k, n, 50, 90, "span")}

    def cb(v, s=""):
        if v in stages:
            if v not in state["seen"]:
                state["seen"].add(v)
                show(v, s or "running")
        elif 20 < v < 50:
            stages[20](v, s)
        elif 50 < v <= 90:              # the sub-call's own 90 closes span k's share; the call's 90 comes after the last span
            stages[50](v, s)
    return cb


def _run_spans(frames_rgb, dil, propainer_frames, plan, body, prog, load=None):
    """The temporal plan carried out: body(frames[a:b], dil[a:b], prior[a:b] | None, progress) per span (a, b), in order; every other frame is the
    original array.  One span that is the whole clip: body on the clip as it is, with the caller's progress.  No span: the original frames, no
    model (load is not called), the milestones 5 / 10 / 20 / 50 / 90 still delivered.  body is the per-clip computation (run_infill_on_frames
    passes _clip_body); load loads the weights once, before the first span."""
    T = len(frames_rgb)
    if list(plan) == [(0, T)]:
        return body(frames_rgb, dil, propainer_frames, prog)
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
    state = {"last": 10, "seen": set()}
    for k, (a, b) in enumerate(plan):
        out[a:b] = body(frames_rgb[a:b], dil[a:b], None if propainer_frames is None else propainer_frames[a:b], _span_progress(prog, k, len(plan), state))
    if prog is not None:
        if 50 not in state["seen"]: prog(50, "running DiffuEraser")
        prog(90, "resizing and merging finished frames")
    return out


def _clip_body(frames_rgb, dil_t, propainer_frames, rcfg, ckpt, dev, max_img_size, keep_unmasked_original, feather_px, prog, num_inference_steps,
               scheduler, compat_reference_early_return=False):
    """One clip after the dilation: roi planning (windows, regions), weights, prior, model, resize and composite.  The whole call without spans=, and
    each span's call with it."""
    H0, W0 = frames_rgb[0].shape[:2]
    if rcfg is not None and rcfg.max_regions > 1:
        plans = _region_plans(dil_t, H0, W0, feather_px, rcfg)
        if plans is not None and len(plans) > 1:
            return _run_regions(frames_rgb, dil_t, plans, propainer_frames, ckpt, dev, max_img_size, feather_px if keep_unmasked_original else -1.0,
                                prog, num_inference_steps, scheduler)
        plan = None if plans is None else plans[0]          # one region (or none): the single-window (or full-frame) path below
    else:
        plan = roi_plan.plan_roi(hip.mask_bbox(dil_t).cpu().numpy(), H0, W0, feather_px, rcfg) if rcfg is not None else None
    dilated_mask_frames = list(dil_t.cpu().numpy())
    full_frames = frames_rgb
    if plan is not None:      # the model, and the prior when it is computed here, see only the windows
        frames_rgb, dilated_mask_frames = plan.crop(frames_rgb), plan.crop(dilated_mask_frames)
        if propainer_frames is not None:
            propainer_frames = plan.crop(propainer_frames)

    if prog is not None: prog(10, "loading weights")
    _load_model(dev, ckpt)

    if propainer_frames is None:                                                # reference :47-57
        _load_prior()
        if prog is not None: prog(20, "running propainter prior")
        propainer_frames = _run_prior(frames_rgb, dilated_mask_frames, prog)

    if prog is not None: prog(50, "running DiffuEraser")
    inpainted_frames = _run_model(frames_rgb, dilated_mask_frames, propainer_frames, max_img_size, prog, num_inference_steps, scheduler)

    if prog is not None: prog(90, "resizing and merging finished frames")
    if plan is not None:
        return _paste_windows(inpainted_frames, full_frames, dil_t, plan, feather_px if keep_unmasked_original else -1.0, dev)
    # reference :69-112.  The reference returns from inside its loop (:114) so only frame 0 is post-processed; the
    # evident intent (all frames) is the default here, compat_reference_early_return=True reproduces the quirk.
    n_post = 1 if compat_reference_early_return else len(inpainted_frames)
    idx = [i for i in range(n_post) if inpainted_frames[i] is not None]        # multi-GPU "rank0" gather: other ranks hold only their own frames
    if not idx:
        return inpainted_frames
    Hm, Wm = inpainted_frames[idx[0]].shape[:2]
    out = torch.from_numpy(np.stack([inpainted_frames[i] for i in idx])).to(dev)
    if (Hm, Wm) != (H0, W0):
        out = hip.resize_u8(out.contiguous(), H0, W0, mode="bilinear")          # cv2.resize(f,(W0,H0)), :73
    if keep_unmasked_original:
        orig = torch.from_numpy(np.stack([frames_rgb[i] for i in idx])).to(dev)
        out = hip.feather_composite(out.contiguous(), orig.contiguous(), dil_t[idx].contiguous(), float(feather_px))   # :77-112
    out = out.cpu().numpy()
    for j, i in enumerate(idx):
        inpainted_frames[i] = out[j]
    return inpainted_frames


def _load_model(dev, ckpt):
    global device, last_ckpt, video_inpainting_sd
    if last_ckpt != ckpt or video_inpainting_sd is None:                        # reference :35-45 (ckpt forced to "2-Step")
        device = dev
        ckpt = "2-Step"
        last_ckpt = ckpt
        video_inpainting_sd = DiffuEraser(device, "stable-diffusion-v1-5/stable-diffusion-v1-5", "stabilityai/sd-vae-ft-mse",
                                          "lixiaowen/diffuEraser", ckpt=ckpt, run=_run_config, dist=_dist, gather=_gather,
                                          weights=_resolve_weights(ckpt)[0])


def _load_prior():
    global propainter
    if propainter is None:
        w, stages = _resolve_weights("2-Step")
        propainter = Propainter("ruffy369/propainter", device=device, weights=w if (w is not None and "raft" in w.components) else None, **stages)


def _run_prior(frames_rgb, dilated_mask_frames, prog):
    prev_tag, hip.PROFILE_TAG = hip.PROFILE_TAG, "prior:"                       # bench.py --prior raft prices the prior's kernels under this prefix
    try:
        return propainter.forward(frames_rgb, dilated_mask_frames, ref_stride=10, neighbor_length=10, subvideo_length=50, mask_dilation=0,
                                  progress=prog)
    finally:
        hip.PROFILE_TAG = prev_tag


def _run_model(frames_rgb, dilated_mask_frames, propainer_frames, max_img_size, prog, num_inference_steps, scheduler):
    guidance_scale = None
    return video_inpainting_sd.forward(frames_rgb, dilated_mask_frames, propainer_frames, max_img_size=max_img_size, mask_dilation_iter=0,
                                       guidance_scale=guidance_scale, progress=prog, num_inference_steps=num_inference_steps, scheduler=scheduler)


REGION_TILE = 16        # px: the occupancy grid the regions are labelled on (roi.label_tiles coarsens it for salt-like masks)


def _region_plans(dil_t, H0, W0, feather_px, cfg):
    """roi.plan_regions for the dilated masks: tile occupancy on the device, its components on the host, then one box per (frame, component)
    from the occupied tiles only (T * K * 16 bytes come back)."""
    occ = hip.mask_tile_union(dil_t, REGION_TILE).cpu().numpy()
    labels, K, tile = roi_plan.label_tiles(occ, tile=REGION_TILE)
    if K == 0:
        return None
    ty, tx = np.nonzero(labels >= 0)
    tiles = torch.from_numpy(np.stack([ty, tx, labels[ty, tx]], axis=1).astype(np.int32)).to(dil_t.device)
    return roi_plan.plan_regions(hip.mask_bbox_tiles(dil_t, tile, tiles, K).cpu().numpy(), H0, W0, feather_px, cfg)


def _region_progress(prog, k, n, lo, hi, what="region"):
    """Progress of region (or span: `what`) k's sub-call (its own values in [lo, hi]) mapped into region k's share of (lo, hi), never onto lo or hi themselves,
    so the caller still sees each of 5 / 10 / 20 / 50 / 90 once and non-decreasing values."""
    if prog is None:
        return None

    def cb(v, s):
        f = min(max((v - lo) / (hi - lo), 0.0), 1.0)
        prog(min(max(lo + int((hi - lo) * (k + f) / n), lo + 1), hi - 1), f"{what} {k + 1}/{n}: {s}" if s else f"{what} {k + 1}/{n}")
    return cb


def _run_regions(frames_rgb, dil_t, plans, propainer_frames, ckpt, dev, max_img_size, feather_px, prog, num_inference_steps, scheduler):
    """Several pairwise disjoint windows (roi.plan_regions): every region's prior, then every region's model, each an ordinary clip call on
    that region's crop, one region after another; then the windows are pasted into the originals one after another."""
    n = len(plans)
    dil = list(dil_t.cpu().numpy())
    crops = [(p.crop(frames_rgb), p.crop(dil)) for p in plans]
    priors = [None if propainer_frames is None else p.crop(propainer_frames) for p in plans]
    if prog is not None: prog(10, "loading weights")
    _load_model(dev, ckpt)
    if propainer_frames is None:
        _load_prior()
        if prog is not None: prog(20, "running propainter prior")
        priors = [_run_prior(f, m, _region_progress(prog, k, n, 20, 50)) for k, (f, m) in enumerate(crops)]
    if prog is not None: prog(50, "running DiffuEraser")
    outs = [_run_model(f, m, priors[k], max_img_size, _region_progress(prog, k, n, 50, 90), num_inference_steps, scheduler)
            for k, (f, m) in enumerate(crops)]
    if prog is not None: prog(90, "resizing and merging finished frames")
    return _paste_regions(outs, frames_rgb, dil_t, plans, feather_px, dev)


def _paste_regions(outs, frames_rgb, dil_t, plans, feather_px, dev):
    """Each region's window frames into the originals: roi_paste_composite once per region, the output of region k the original of region
    k + 1 (two buffers, one upload, one download).  Exact because the windows are disjoint: inside window k the mask holds only region k's
    pixels and no other region has touched the bytes."""
    idx = [i for i in range(len(outs[0])) if outs[0][i] is not None]          # multi-GPU "rank0" gather, as in _paste_windows
    if not idx:
        return outs[0]
    bufs = [torch.from_numpy(np.stack([frames_rgb[i] for i in idx])).to(dev).contiguous()]
    bufs.append(torch.empty_like(bufs[0]))
    mask = dil_t[idx].contiguous()
    for k, (plan, o) in enumerate(zip(plans, outs)):
        h, w = plan.size
        patch = torch.from_numpy(np.stack([o[i] for i in idx])).to(dev)
        offs = torch.from_numpy(np.ascontiguousarray(plan.offsets[idx])).to(dev)
        hip.roi_paste_composite(patch.contiguous(), bufs[k % 2], mask, offs, h, w, float(feather_px), out=bufs[(k + 1) % 2])
    out = bufs[len(plans) % 2].cpu().numpy()
    res = list(outs[0])
    for j, i in enumerate(idx):
        res[i] = out[j]
    return res


def _paste_windows(inpainted_frames, frames_rgb, dil_t, plan, feather_px, dev):
    """The model's window frames back into the full-size originals (resize to the window, paste, feathered composite: one kernel)."""
    idx = [i for i in range(len(inpainted_frames)) if inpainted_frames[i] is not None]       # multi-GPU "rank0" gather, as below
    if not idx:
        return inpainted_frames
    h, w = plan.size
    patch = torch.from_numpy(np.stack([inpainted_frames[i] for i in idx])).to(dev)
    orig = torch.from_numpy(np.stack([frames_rgb[i] for i in idx])).to(dev)
    offs = torch.from_numpy(np.ascontiguousarray(plan.offsets[idx])).to(dev)
    out = hip.roi_paste_composite(patch.contiguous(), orig.contiguous(), dil_t[idx].contiguous(), offs, h, w, float(feather_px)).cpu().numpy()
    res = list(inpainted_frames)
    for j, i in enumerate(idx):
        res[i] = out[j]
    return res


def _frame_io():
    """The reference's own frame I/O helper `tools` (cv2; reference tools.py:4-45) when the drop-in sits next to the GUI, else the
    cv2-free FFV1 / Matroska module with the same two functions.  The test is for the API, not for the import: a
    directory called tools/ next to this file imports as an (empty) namespace package."""
    try:
        import tools
        if callable(getattr(tools, "load_video_frames_from_path", None)) and callable(getattr(tools, "write_video_frames_to_path", None)):
            return tools
    except ImportError:
        pass
    from videovanish_amd import frameio
    return frameio


# =============================
# CLI entry point (reference diffuerase.py:121-155)
# =============================
def main():
    tools = _frame_io()
    ap = argparse.ArgumentParser(description="Remove masked objects from a video (DiffuEraser hot path on MI355X).")
    ap.add_argument("--color_video", required=True, type=str, help="Input color video path.")
    ap.add_argument("--mask_video", required=True, type=str, help="Input mask video path.")
    ap.add_argument("--prior_video", required=False, type=str, help="Input prior video path.")
    ap.add_argument("--start_frame", type=int, default=0, help="Index of first frame to process (default: 0).")
    ap.add_argument("--max_frames", type=int, default=-1, help="Max number of frames to process after start_frame.")
    ap.add_argument("--out", type=str, default=None, help="Output video path (default: <input>_vanished.mkv)")
    ap.add_argument("--roi", choices=roi_plan.SPELLINGS, default=None,
                    help="Mask-region inference: run the model only on a window around the masks (static: one window per clip; follow: "
                         "a window that follows the mask; static-regions / follow-regions: one such window per separate masked region).  "
                         "Pixels outside the windows stay the original ones.")
    ap.add_argument("--spans", choices=span_plan.SPELLINGS, default=None,
                    help="Mask-span inference: masked = process only the frame runs that have a mask (with some context), the other frames stay "
                         "the original ones; cuts = process every frame but split the clip at hard cuts found in the video; masked-cuts = both.")
    ap.add_argument("--cuts", type=span_plan.parse_cuts, default=None, metavar="120,431",
                    help="Frame indices (relative to --start_frame) where a new shot begins: used instead of the detector.")
    args = ap.parse_args()

    assert os.path.isfile(args.color_video), "input video missing"
    out_video = args.out or (args.color_video + "_vanished.mkv")
    frames, fps = tools.load_video_frames_from_path(args.color_video, args.start_frame, args.max_frames)
    H0, W0 = frames[0].shape[:2]
    mask_frames, mask_fps = tools.load_video_frames_from_path(args.mask_video, args.start_frame, args.max_frames)
    Hm, Wm = mask_frames[0].shape[:2]
    prior_frames = None
    if args.prior_video is not None:      # the reference's test is inverted (:142); a supplied prior is used here
        prior_frames, prior_fps = tools.load_video_frames_from_path(args.prior_video, args.start_frame, args.max_frames)
        Hp, Wp = prior_frames[0].shape[:2]
        assert (H0 == Hp and W0 == Wp), "prior and color video are diffrent sizes"
    assert (H0 == Hm and W0 == Wm), "mask and color video are diffrent sizes"
    kw = {"roi": args.roi} if args.roi is not None else {}      # pass roi= / spans= / cuts= only when asked for: a default call stays the reference's call
    if args.spans is not None: kw["spans"] = args.spans
    if args.cuts is not None: kw["cuts"] = args.cuts
    out_frames = run_infill_on_frames(frames, mask_frames, propainer_frames=prior_frames, **kw)
    tools.write_video_frames_to_path(out_video, out_frames, fps, H0, W0)


if __name__ == '__main__':
    main()

"""Drop-in replacement for the reference module `diffuerase` (reference diffuerase.py:1-158): same module name, same
`run_infill_on_frames` signature and CLI, so `videovanish.py` (reference :46,1518,1593) keeps working unchanged --
with the hot path running on hand-written gfx950 HIP kernels (videovanish_amd/) instead of torch/cuDNN.

Extra keyword-only knobs (old callers are unaffected): num_inference_steps, scheduler, chunk, overlap, dtype, seed,
compat_reference_early_return, roi (mask-region inference: videovanish_amd/roi.py; also configure(roi=...) and $VV_ROI), spans / cuts (mask-span
inference: only the runs of masked frames are processed, and nothing crosses a hard cut: videovanish_amd/spans.py; also configure(spans=...) and
$VV_SPANS), mask_clean (mask clean-up between the dilation and the planners: speckles dropped, dropouts bridged, the mask grown in time:
videovanish_amd/maskclean.py; also configure(mask_clean=...) and $VV_MASK_CLEAN), tone_match (seam tone matching: the model's pixels are fitted to
the ring of unmasked pixels round the mask before the composite: videovanish_amd/tonematch.py; also configure(tone_match=...) and $VV_TONE_MATCH), grain_match (seam grain matching: the pasted pixels get the grain
the original pixels of that ring have and the model's lack: videovanish_amd/grainmatch.py; also configure(grain_match=...) and $VV_GRAIN_MATCH),
grain_shape (grain shape: with grain_match, the size of that grain is fitted on the ring as well and the added noise is shaped by it:
videovanish_amd/grainshape.py; also configure(grain_shape=...) and $VV_GRAIN_SHAPE), seam_blend (seam membrane blending: the
difference original - model on that ring, interpolated harmonically into the hole and added to the pasted pixels: videovanish_amd/seamblend.py;
also configure(seam_blend=...) and $VV_SEAM_BLEND), detail_match (seam detail matching: the pasted pixels get, or lose, as much of their own
high-pass as makes the model's rendering of that ring as sharp as the original there: videovanish_amd/detailmatch.py; also
configure(detail_match=...) and $VV_DETAIL_MATCH), plate_fill (clean-plate fill: masked pixels whose background other frames of the shot show are
filled from the nearest such frame and leave the mask before anything plans or runs the model: videovanish_amd/platefill.py; also
configure(plate_fill=...) and $VV_PLATE_FILL), plate_align (clean-plate alignment: with plate_fill, one integer translation per frame is
tracked first, so that the fill follows a panning camera: videovanish_amd/platealign.py; also configure(plate_align=...) and $VV_PLATE_ALIGN),
plate_warp (clean-plate warp: with plate_fill and plate_align, one affine map per frame is fitted to block-matched vectors, so that the fill
follows zoom and roll too: videovanish_amd/platewarp.py; also configure(plate_warp=...) and $VV_PLATE_WARP),
plate_grain (clean-plate grain: with plate_fill, a filled pixel takes its bytes from a few usable frames in turn, not from the nearest alone, so
that the grain inside the fill moves: videovanish_amd/plategrain.py; also configure(plate_grain=...) and $VV_PLATE_GRAIN),
plate_tone (clean-plate exposure matching: with plate_fill, every frame of a segment is mapped to the segment's common exposure before the fill
samples it and every filled pixel back to its own frame's, so that the fill survives exposure drift and flicker: videovanish_amd/platetone.py;
also configure(plate_tone=...) and $VV_PLATE_TONE),
shadow_mask (shadow masking: unmasked pixels that look like the shot's clean background uniformly darkened and hang on to the mask join it,
between the mask clean-up and the clean-plate fill: videovanish_amd/shadowmask.py; also configure(shadow_mask=...) and $VV_SHADOW_MASK),
overlay_mask (overlay masking: screen-fixed graphics -- a station logo, a channel bug -- are found from the edges that stand still while the
picture under them moves and join the mask of every frame, between the mask clean-up and the shadow masking: videovanish_amd/overlaymask.py;
also configure(overlay_mask=...), $VV_OVERLAY_MASK and find_overlays()),
deflicker (inpaint deflicker: the model's pixels are filtered along time before every other seam stage reads them, each the mean of its temporal
neighbours within a tolerance, so that the patch stops shimmering while moving edges stay as they are: videovanish_amd/deflicker.py; also
configure(deflicker=...) and $VV_DEFLICKER), deflicker_align (aligned inpaint deflicker: with deflicker, one integer translation per frame is
tracked first, so that the filter follows a panning camera: videovanish_amd/deflickeralign.py; also configure(deflicker_align=...) and
$VV_DEFLICKER_ALIGN), deflicker_local (block-matched inpaint deflicker: with deflicker, one integer displacement per small block and temporal
neighbour is found by block matching first, so that the filter follows parallax, a zoom and a second plane of motion:
videovanish_amd/deflickerlocal.py; also configure(deflicker_local=...) and $VV_DEFLICKER_LOCAL).
There is no CPU fallback: without the HIP extension / a GPU this raises.

This file is the boundary: the reference's names and module state, the settings, and the stages (weights, prior, model) that read that state.
What a call does with them -- spans, windows, crop -> prior -> model, resize / paste / composite -- is videovanish_amd/infill.py.
"""
import argparse
import os
from typing import NamedTuple

import numpy as np
import torch

from videovanish_amd import hip, infill
from videovanish_amd import deflicker as deflicker_settings
from videovanish_amd import deflickeralign, deflickerlocal, detailmatch, grainmatch, grainshape, maskclean, overlaymask, platealign, platefill, plategrain, platetone, platewarp, seamblend, shadowmask, tonematch
from videovanish_amd import roi as roi_plan
from videovanish_amd import spans as span_plan
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
last_mask_clean = None  # the infill.MaskCleanReport of the last run_infill_on_frames call; None when the stage did not run
last_tone_match = None  # the infill.ToneMatchReport of the last run_infill_on_frames call; None when the stage did not run
last_grain_match = None # the infill.GrainMatchReport of the last run_infill_on_frames call; None when the stage did not run
last_seam_blend = None  # the infill.SeamBlendReport of the last run_infill_on_frames call; None when the stage did not run
last_plate_fill = None  # the infill.PlateFillReport of the last run_infill_on_frames call; None when the stage did not run
last_plate_align = None # the infill.PlateAlignReport of the last run_infill_on_frames call; None when the tracker did not run
last_plate_grain = None # the infill.PlateGrainReport of the last run_infill_on_frames call; None when the rotation was not asked for
last_plate_tone = None  # the infill.PlateToneReport of the last run_infill_on_frames call; None when the matching was not asked for
last_shadow_mask = None # the infill.ShadowMaskReport of the last run_infill_on_frames call; None when the stage did not run
last_deflicker = None   # the infill.DeflickerReport of the last run_infill_on_frames call; None when the stage did not run
last_deflicker_align = None  # the infill.DeflickerAlignReport of the last run_infill_on_frames call; None when the tracker did not run
last_detail_match = None     # the infill.DetailMatchReport of the last run_infill_on_frames call; None when the stage did not run
last_grain_shape = None      # the infill.GrainShapeReport of the last run_infill_on_frames call; None when the shape was not asked for
last_deflicker_local = None  # the infill.DeflickerLocalReport of the last run_infill_on_frames call; None when the search was not asked for
last_overlay_mask = None     # the infill.OverlayMaskReport of the last run_infill_on_frames call; None when the stage did not run
last_plate_warp = None       # the infill.PlateWarpReport of the last run_infill_on_frames call; None when the warp was not asked for


class Option(NamedTuple):
    """One opt-in setting: the keyword of run_infill_on_frames and configure(), the module whose as_config reads its spellings, the environment
    variable behind both, the words for it in messages, and what --help shows for the command-line value (None: a choice of the module's
    SPELLINGS)."""
    name: str
    settings: object
    env: str
    phrase: str
    metavar: str = None


OPTIONS = (
    Option("roi", roi_plan, "VV_ROI", "mask-region inference"),
    Option("spans", span_plan, "VV_SPANS", "mask-span inference"),
    Option("mask_clean", maskclean, "VV_MASK_CLEAN", "mask clean-up", "on|area=64,bridge=2,grow=1"),
    Option("tone_match", tonematch, "VV_TONE_MATCH", "seam tone matching", "on|affine|offset|mode=offset,ring=8,smooth=0"),
    Option("grain_match", grainmatch, "VV_GRAIN_MATCH", "seam grain matching", "on|luma|rgb|mode=rgb,ring=8,strength=0.8,seed=3"),
    Option("seam_blend", seamblend, "VV_SEAM_BLEND", "seam membrane blending", "on|ring=12,presmooth=2,sweeps=8,max_shift=32,strength=1.0"),
    Option("plate_fill", platefill, "VV_PLATE_FILL", "clean-plate fill", "on|guard=1,min_samples=4,tol=6,outlier=3,max_gap=0,margin=2"),
    Option("plate_align", platealign, "VV_PLATE_ALIGN", "clean-plate alignment", "on|levels=4,radius=4,min_overlap=25,max_residual=12"),
    Option("deflicker", deflicker_settings, "VV_DEFLICKER", "inpaint deflicker", "on|radius=2,tol=12"),
    Option("deflicker_align", deflickeralign, "VV_DEFLICKER_ALIGN", "aligned inpaint deflicker", "on|levels=4,radius=4,min_overlap=25,max_residual=12"),
)
# OPTIONS holds the ten rows tests/test_cli_cpu.py names one by one; a row added since stands here, and everything below walks ALL_OPTIONS
MORE_OPTIONS = (
    Option("plate_grain", plategrain, "VV_PLATE_GRAIN", "clean-plate grain", "on|depth=4,reach=8"),
    Option("shadow_mask", shadowmask, "VV_SHADOW_MASK", "shadow masking", "on|guard=1,min_samples=4,tol=6,lo=30,hi=90,drop=12,chroma=20,floor=16,reach=32,min_area=16,grow=1"),
    Option("plate_tone", platetone, "VV_PLATE_TONE", "clean-plate exposure matching", "on|mode=affine,ring=32,floor=16,min_pixels=1024,max_gain=25,max_offset=32"),
    Option("detail_match", detailmatch, "VV_DETAIL_MATCH", "seam detail matching",
           "on|ring=8,edge=12,smooth=2,min_pixels=256,max_sharpen=2.0,max_soften=1.0,dead=0.06,overshoot=4,strength=1.0"),
    Option("grain_shape", grainshape, "VV_GRAIN_SHAPE", "grain shape", "on|max_a=0.5,dead=0.05,min_pairs=512,smooth=4,max_gain=6"),
    Option("deflicker_local", deflickerlocal, "VV_DEFLICKER_LOCAL", "block-matched inpaint deflicker", "on|block=8,search=4,lam=32"),
    Option("overlay_mask", overlaymask, "VV_OVERLAY_MASK", "overlay masking",
           "on|min_samples=12,mag=8,coh=80,max_share=25,close=2,max_hole=4096,min_area=64,max_area=10,border=0,grow=3"),
    Option("plate_warp", platewarp, "VV_PLATE_WARP", "clean-plate warp", "on|block=16,search=8,min_texture=2,min_blocks=12,trim=10,rounds=3,max_linear=50"),
)
ALL_OPTIONS = OPTIONS + MORE_OPTIONS
_OPTION = {o.name: o for o in ALL_OPTIONS}
_configured = {}        # configure(<option>=...): the value for calls that do not pass that keyword themselves, as given


def configure(run: RunConfig = None, dist=None, gather="all", prior=None, weights=None, reference_defaults=False, roi=None, spans=None,
              mask_clean=None, tone_match=None, grain_match=None, grain_shape=None, seam_blend=None, detail_match=None, deflicker=None, deflicker_align=None, deflicker_local=None, overlay_mask=None, shadow_mask=None, plate_tone=None, plate_warp=None, plate_grain=None, plate_align=None, plate_fill=None):
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
    spans = None / "masked" / "cuts" / "masked-cuts" / a spans.SpanConfig: mask-span inference for calls that do not pass spans=.
    mask_clean = None / "on" / "area=64,bridge=2,grow=1" (any subset) / a maskclean.MaskCleanConfig: mask clean-up for calls that do not pass
    mask_clean=.
    tone_match = None / "on" / "affine" / "offset" / "mode=offset,ring=8,smooth=0" (any subset) / a tonematch.ToneMatchConfig: seam tone matching
    for calls that do not pass tone_match=.
    grain_match = None / "on" / "luma" / "rgb" / "mode=rgb,ring=8,strength=0.8,seed=3" (any subset) / a grainmatch.GrainMatchConfig: seam grain
    matching for calls that do not pass grain_match=.
    grain_shape = None / "on" / "max_a=0.5,dead=0.05,min_pairs=512,smooth=4,max_gain=6" (any subset) / a grainshape.GrainShapeConfig: grain shape
    for calls that do not pass grain_shape=.
    seam_blend = None / "on" / "ring=12,presmooth=2,sweeps=8,max_shift=32,strength=1.0" (any subset) / a seamblend.SeamBlendConfig: seam membrane
    blending for calls that do not pass seam_blend=.
    detail_match = None / "on" / "ring=8,edge=12,smooth=2,min_pixels=256,max_sharpen=2.0,max_soften=1.0,dead=0.06,overshoot=4,strength=1.0" (any
    subset) / a detailmatch.DetailMatchConfig: seam detail matching for calls that do not pass detail_match=.
    plate_fill = None / "on" / "guard=1,min_samples=4,tol=6,outlier=3,max_gap=0,margin=2,max_bytes=N" (any subset) / a platefill.PlateFillConfig:
    clean-plate fill for calls that do not pass plate_fill=.
    plate_align = None / "on" / "levels=4,radius=4,min_overlap=25,max_residual=12" (any subset) / a platealign.PlateAlignConfig: clean-plate
    alignment for calls that do not pass plate_align=.
    plate_grain = None / "on" / "depth=4,reach=8" (any subset) / a plategrain.PlateGrainConfig: clean-plate grain for calls that do not pass
    plate_grain=.
    plate_tone = None / "on" / "mode=affine,ring=32,floor=16,min_pixels=1024,max_gain=25,max_offset=32" (any subset) / a platetone.PlateToneConfig:
    clean-plate exposure matching for calls that do not pass plate_tone=.
    shadow_mask = None / "on" / "guard=1,min_samples=4,tol=6,lo=30,hi=90,drop=12,chroma=20,floor=16,reach=32,min_area=16,grow=1,max_bytes=N" (any
    subset) / a shadowmask.ShadowMaskConfig: shadow masking for calls that do not pass shadow_mask=.
    overlay_mask = None / "on" / "min_samples=12,mag=8,coh=80,max_share=25,close=2,max_hole=4096,min_area=64,max_area=10,border=0,grow=3,
    max_bytes=N" (any subset) / an overlaymask.OverlayMaskConfig: overlay masking for calls that do not pass overlay_mask=.
    deflicker = None / "on" / "radius=2,tol=12" (any subset) / a deflicker.DeflickerConfig: inpaint deflicker for calls that do not pass
    deflicker=.
    deflicker_align = None / "on" / "levels=4,radius=4,min_overlap=25,max_residual=12" (any subset) / a platealign.PlateAlignConfig: aligned
    inpaint deflicker for calls that do not pass deflicker_align=.
    deflicker_local = None / "on" / "block=8,search=4,lam=32" (any subset) / a deflickerlocal.DeflickerLocalConfig: block-matched inpaint
    deflicker for calls that do not pass deflicker_local=.
    plate_warp = None / "on" / "block=16,search=8,min_texture=2,min_blocks=12,trim=10,rounds=3,max_linear=50" (any subset) / a
    platewarp.PlateWarpConfig: clean-plate warp for calls that do not pass plate_warp=."""
    global _run_config, _dist, _gather, last_ckpt, _prior_stages, propainter, _weights, _loaded
    given = locals()
    for o in reversed(ALL_OPTIONS):         # validated now, kept as given: configure(roi="off") means the full frame whatever $VV_ROI says
        o.settings.as_config(given[o.name])
    if reference_defaults:
        import dataclasses
        run = dataclasses.replace(run or RunConfig(), windowing="reference")
        prior = dict({"flow_completion": True, "generator": True}, **(prior or {}))
    _run_config, _dist, _gather, last_ckpt = run, dist, gather, None
    _prior_stages, propainter = dict(prior or {}), None
    _weights, _loaded = weights, None
    _configured.update({o.name: given[o.name] for o in ALL_OPTIONS})


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


def _setting(name, value, *more):
    """The setting `name` a call runs with: its own argument, else configure()'s, else the environment's; "off" (or False) at any level ends
    the search with None.  more = what the option's as_config takes besides the value."""
    o = _OPTION[name]
    for v in (value, _configured.get(name)):
        if v is not None:
            return o.settings.as_config(v, *more)
    return o.settings.as_config(os.environ.get(o.env), *more)


def roi_config(roi=None):
    """The mask-region setting a call runs with: its own roi= argument, else configure(roi=...), else $VV_ROI (static | follow | static-regions |
    follow-regions | off).
    None = full frame.  roi="off" (or False) asks for the full frame whatever configure() or the environment say."""
    return _setting("roi", roi)


def spans_config(spans=None, cuts=None):
    """The mask-span setting a call runs with: its own spans= argument, else configure(spans=...), else $VV_SPANS (masked | cuts | masked-cuts | off).
    None = the full clip.  spans="off" (or False) asks for the full clip whatever configure() or the environment say.  cuts (frame indices) replaces
    the setting's own cuts: explicit cuts always override the detector; given alone it means "every frame, split at these cuts"."""
    cfg = _setting("spans", spans)
    if cuts is not None and not (spans is not None and cfg is None):        # spans="off" wins over cuts=
        import dataclasses
        cfg = span_plan.SpanConfig("all", cuts=cuts) if cfg is None else dataclasses.replace(cfg, cuts=cuts)
    return cfg


def mask_clean_config(mask_clean=None):
    """The mask clean-up setting a call runs with: its own mask_clean= argument, else configure(mask_clean=...), else $VV_MASK_CLEAN (on | off |
    area=N,bridge=N,grow=N).  None = no clean-up.  mask_clean="off" (or False) asks for none whatever configure() or the environment say."""
    return _setting("mask_clean", mask_clean)


def tone_match_config(tone_match=None):
    """The seam tone matching setting a call runs with: its own tone_match= argument, else configure(tone_match=...), else $VV_TONE_MATCH (on |
    affine | offset | off | mode=..,ring=N,..).  None = no tone matching.  tone_match="off" (or False) asks for none whatever configure() or the
    environment say."""
    return _setting("tone_match", tone_match)


def grain_match_config(grain_match=None):
    """The seam grain matching setting a call runs with: its own grain_match= argument, else configure(grain_match=...), else $VV_GRAIN_MATCH (on |
    luma | rgb | off | mode=..,ring=N,..).  None = no grain matching.  grain_match="off" (or False) asks for none whatever configure() or the
    environment say."""
    return _setting("grain_match", grain_match)


def grain_shape_config(grain_shape=None):
    """The grain shape setting a call runs with: its own grain_shape= argument, else configure(grain_shape=...), else $VV_GRAIN_SHAPE (on | off |
    max_a=X,dead=X,min_pairs=N,smooth=N,max_gain=X).  None = grain matching adds white noise.  grain_shape="off" (or False) asks for that
    whatever configure() or the environment say."""
    return _setting("grain_shape", grain_shape)


def seam_blend_config(seam_blend=None, feather_px=None):
    """The seam membrane blending setting a call runs with: its own seam_blend= argument, else configure(seam_blend=...), else $VV_SEAM_BLEND (on |
    off | ring=N,presmooth=N,sweeps=N,max_shift=N,strength=X).  None = no blending.  seam_blend="off" (or False) asks for none whatever
    configure() or the environment say.  feather_px: the call's feather, which the ring has to be wider than."""
    return _setting("seam_blend", seam_blend, feather_px)


def detail_match_config(detail_match=None):
    """The seam detail matching setting a call runs with: its own detail_match= argument, else configure(detail_match=...), else $VV_DETAIL_MATCH
    (on | off | ring=N,edge=N,smooth=N,min_pixels=N,max_sharpen=X,max_soften=X,dead=X,overshoot=N,strength=X).  None = no detail matching.
    detail_match="off" (or False) asks for none whatever configure() or the environment say."""
    return _setting("detail_match", detail_match)


def plate_fill_config(plate_fill=None):
    """The clean-plate fill setting a call runs with: its own plate_fill= argument, else configure(plate_fill=...), else $VV_PLATE_FILL (on | off |
    guard=N,min_samples=N,tol=N,outlier=N,max_gap=N,margin=N,max_bytes=N).  None = no fill.  plate_fill="off" (or False) asks for none whatever
    configure() or the environment say."""
    return _setting("plate_fill", plate_fill)


def plate_align_config(plate_align=None):
    """The clean-plate alignment setting a call runs with: its own plate_align= argument, else configure(plate_align=...), else $VV_PLATE_ALIGN
    (on | off | levels=N,radius=N,min_overlap=N,max_residual=N).  None = no alignment.  plate_align="off" (or False) asks for none whatever
    configure() or the environment say."""
    return _setting("plate_align", plate_align)


def plate_warp_config(plate_warp=None):
    """The clean-plate warp setting a call runs with: its own plate_warp= argument, else configure(plate_warp=...), else $VV_PLATE_WARP (on | off |
    block=N,search=N,min_texture=N,min_blocks=N,trim=N,rounds=N,max_linear=N).  None = translations only.  plate_warp="off" (or False) asks
    for that whatever configure() or the environment say."""
    return _setting("plate_warp", plate_warp)


def plate_grain_config(plate_grain=None):
    """The clean-plate grain setting a call runs with: its own plate_grain= argument, else configure(plate_grain=...), else $VV_PLATE_GRAIN
    (on | off | depth=N,reach=N).  None = every filled pixel takes the nearest usable frame.  plate_grain="off" (or False) asks for that whatever
    configure() or the environment say."""
    return _setting("plate_grain", plate_grain)


def plate_tone_config(plate_tone=None):
    """The clean-plate exposure matching setting a call runs with: its own plate_tone= argument, else configure(plate_tone=...), else
    $VV_PLATE_TONE (on | off | mode=affine|gain|offset,ring=N,floor=N,min_pixels=N,max_gain=N,max_offset=N).  None = the fill samples the frames
    as they are.  plate_tone="off" (or False) asks for that whatever configure() or the environment say."""
    return _setting("plate_tone", plate_tone)


def shadow_mask_config(shadow_mask=None):
    """The shadow masking setting a call runs with: its own shadow_mask= argument, else configure(shadow_mask=...), else $VV_SHADOW_MASK (on | off |
    guard=N,min_samples=N,tol=N,lo=N,hi=N,drop=N,chroma=N,floor=N,reach=N,min_area=N,grow=N,max_bytes=N).  None = the masks as they are.
    shadow_mask="off" (or False) asks for that whatever configure() or the environment say."""
    return _setting("shadow_mask", shadow_mask)


def overlay_mask_config(overlay_mask=None):
    """The overlay masking setting a call runs with: its own overlay_mask= argument, else configure(overlay_mask=...), else $VV_OVERLAY_MASK (on |
    off | min_samples=N,mag=N,coh=N,max_share=N,close=N,max_hole=N,min_area=N,max_area=N,border=N,grow=N,max_bytes=N).  None = the masks as
    they are.  overlay_mask="off" (or False) asks for that whatever configure() or the environment say."""
    return _setting("overlay_mask", overlay_mask)


def deflicker_config(deflicker=None):
    """The inpaint deflicker setting a call runs with: its own deflicker= argument, else configure(deflicker=...), else $VV_DEFLICKER (on | off |
    radius=N,tol=N).  None = no deflicker.  deflicker="off" (or False) asks for none whatever configure() or the environment say."""
    return _setting("deflicker", deflicker)


def deflicker_align_config(deflicker_align=None):
    """The aligned-deflicker setting a call runs with: its own deflicker_align= argument, else configure(deflicker_align=...), else
    $VV_DEFLICKER_ALIGN (on | off | levels=N,radius=N,min_overlap=N,max_residual=N).  None = the filter stays at a fixed frame place.
    deflicker_align="off" (or False) asks for none whatever configure() or the environment say."""
    return _setting("deflicker_align", deflicker_align)


def deflicker_local_config(deflicker_local=None):
    """The block-matched deflicker setting a call runs with: its own deflicker_local= argument, else configure(deflicker_local=...), else
    $VV_DEFLICKER_LOCAL (on | off | block=N,search=N,lam=N).  None = the filter reads its neighbours at one place per frame.
    deflicker_local="off" (or False) asks for that whatever configure() or the environment say."""
    return _setting("deflicker_local", deflicker_local)


def run_infill_on_frames(frames_rgb, mask_frames, mask_dilation_iter=8, ckpt="2-Step",
                         propainer_frames=None, max_img_size=960, keep_unmasked_original=True, feather_px=3, prog=None,
                         *, num_inference_steps=None, scheduler=None, compat_reference_early_return=False, roi=None, spans=None, cuts=None,
                         mask_clean=None, tone_match=None, grain_match=None, grain_shape=None, seam_blend=None, detail_match=None, deflicker=None, deflicker_align=None, deflicker_local=None, overlay_mask=None, shadow_mask=None, plate_tone=None, plate_warp=None, plate_grain=None, plate_align=None, plate_fill=None):
    """roi (mask-region inference, opt-in): "static" / "follow" / a videovanish_amd.roi.RoiConfig crops every frame to a window around the dilated
    masks, runs the prior and the model on that smaller clip and pastes the result back into the original frames: pixels outside the window are
    the original bytes.  Falls back to the full frame when no frame has a mask pixel or the window would be the whole frame.
    "static-regions" / "follow-regions" (RoiConfig.max_regions > 1): one window per separate masked region (roi.plan_regions), each region an
    ordinary clip call on its crop, the windows pasted one after another; one region left is one window, as with "static" / "follow" (infill.run_clip: one path for 0, 1 and k windows).
    spans (mask-span inference, opt-in): "masked" / "cuts" / "masked-cuts" / a videovanish_amd.spans.SpanConfig splits the clip in time
    (spans.plan_spans): at hard cuts (cuts=[...] frame indices, or found on the device: "cuts", "masked-cuts"), and in "masked" mode into spans
    around the runs of masked frames only.  Each span is this call on frames[a:b] (its own roi windows, chunks and lanes); frames outside every
    span are returned as the original arrays, also with keep_unmasked_original=False.  A clip without a mask pixel returns its input and loads
    no model; one span that is the whole clip is the plain call.
    mask_clean (mask clean-up, opt-in): "on" / "area=64,bridge=2,grow=1" / a videovanish_amd.maskclean.MaskCleanConfig cleans the dilated masks
    on the device before anything reads them (infill.clean_masks): components holding fewer than min_area raw mask pixels are cleared, dropouts
    of at most `bridge` frames are filled per pixel, the mask is held `grow` frames longer at both ends; the temporal steps stay inside the
    segments between the cuts of spans= / cuts= (found on the despeckled masks when they are "auto").  The result replaces the dilated masks
    for the span and window planners, the prior, the model and the composite; what it changed is kept in last_mask_clean.  Masks that need
    nothing give the bytes of the call without it.
    tone_match (seam tone matching, opt-in): "on" / "affine" / "offset" / "mode=offset,ring=8,smooth=0" / a videovanish_amd.tonematch.ToneMatchConfig
    fits, per frame and channel, the model's pixels to the original ones over the ring of unmasked pixels round the mask (a gain and an offset,
    pooled over neighbouring frames, clamped) and sends every pasted pixel through the resulting table before the feathered composite
    (infill.finish), for the full frame and for every roi window, inside each span.  What it applied is kept in last_tone_match.  A model frame
    that equals the original on the ring gives the bytes of the call without it.
    grain_match (seam grain matching, opt-in): "on" / "luma" / "rgb" / "mode=rgb,ring=8,strength=0.8,seed=3" / a
    videovanish_amd.grainmatch.GrainMatchConfig measures, per frame, channel and brightness band, the grain the original pixels have and the
    model's pixels lack over the flat part of that ring (after tone matching's table, when both are on; pooled over neighbouring frames,
    capped) and adds stateless white noise of that level to every pasted pixel before the feathered composite (infill.finish), for the full
    frame and for every roi window, inside each span; the noise of a pixel depends on the seed, the frame's index in this call and the
    pixel's position in the frame only.  What it measured and added is kept in last_grain_match.  A model frame that equals the original on
    the ring gives the bytes of the call without it.
    grain_shape (grain shape, opt-in, needs grain_match): "on" / "max_a=0.5,dead=0.05,min_pairs=512,smooth=4,max_gain=6" / a
    videovanish_amd.grainshape.GrainShapeConfig fits, per frame (and per channel in "rgb" mode) and axis, the SIZE of that grain from the lag-1
    correlation of the noise operator's responses over the same ring (rules: include/grainshape.h), corrects the level the operator
    under-reads on grain that is not white, and sends the added noise through the separable kernel [a, 1, a] per axis, 0 <= a <= 0.5: from
    white to the binomial blur, for footage whose grain has been resized, debayered, denoised or compressed.  What it fitted is kept in
    last_grain_shape.  Grain that is white gives a = 0 and the bytes of grain_match alone.  Without an effective grain_match it is a
    ValueError.
    seam_blend (seam membrane blending, opt-in): "on" / "ring=12,presmooth=2,sweeps=8,max_shift=32,strength=1.0" / a
    videovanish_amd.seamblend.SeamBlendConfig interpolates, per frame and channel, the difference original - model from that ring harmonically
    into the hole (after tone matching's table, when both are on) and adds this membrane to every pasted pixel before the grain and the
    feathered composite (infill.finish), for the full frame and for every roi window, inside each span: a correction that varies across the
    hole, which one gain and offset cannot give; in front of it tone matching fits its offset alone (gain 1), whatever its mode.  The ring must be wider than ceil(feather_px).  What it measured and added is kept in
    last_seam_blend.  A model frame that equals the original on the ring gives the bytes of the call without it.
    detail_match (seam detail matching, opt-in): "on" / "ring=8,edge=12,smooth=2,min_pixels=256,max_sharpen=2.0,max_soften=1.0,dead=0.06,
    overshoot=4,strength=1.0" / a videovanish_amd.detailmatch.DetailMatchConfig fits, per frame, how much of its own 3 x 3 high-pass the model's
    rendering lacks, or has too much of, against the original over the structured part of that ring (an exact integer least-squares fit, pooled
    over neighbouring frames, capped, with a dead zone; rules: include/detailmatch.h) and applies that amount to every pixel of the window as an
    unsharp mask clamped to the range of the pixel's neighbourhood, after the deflicker and before tone matching, membrane blending and grain
    matching measure the rendering (infill.finish), for the full frame and for every roi window, inside each span.  What it measured and
    applied is kept in last_detail_match.  A model frame that equals the original on the ring gives the bytes of the call without it, and so
    does strength=0.
    plate_fill (clean-plate fill, opt-in): "on" / "guard=1,min_samples=4,tol=6,outlier=3,max_gap=0,margin=2,max_bytes=N" / a
    videovanish_amd.platefill.PlateFillConfig fills, after the dilation and the mask clean-up and before anything plans or runs, every masked
    pixel whose background the same shot shows steadily in other frames at the same place with the bytes of the nearest such frame
    (infill.plate_fill; rules: include/vvplate.h) and takes it out of the mask; the segments are those between the cuts of spans= / cuts=.  The
    filled frames and the smaller masks replace the originals for the span and window planners, the prior, the model and the composite: windows
    shrink, and with spans="masked" frames that are filled completely drop out of inference.  A supplied propainer_frames is passed on
    untouched.  What it filled is kept in last_plate_fill.  A clip in which nothing can be filled gives the bytes of the call without it.
    plate_align (clean-plate alignment, opt-in, needs plate_fill): "on" / "levels=4,radius=4,min_overlap=25,max_residual=12" / a
    videovanish_amd.platealign.PlateAlignConfig tracks, per segment, one integer translation per frame against a held key frame (rules:
    include/vvalign.h) and runs the fill on the canvas in which the background stands still, so that a slow pan or tilt, or a static overlay
    over a panning shot, is filled from the frames that show its background at another place.  A frame the tracker loses gives no sample
    and keeps its mask; a locked-off clip gives the bytes of the call without it.  What it found is kept in last_plate_align.  Without an
    effective plate_fill it is a ValueError.
    plate_warp (clean-plate warp, opt-in, needs plate_fill and plate_align): "on" / "block=16,search=8,min_texture=2,min_blocks=12,trim=10,
    rounds=3,max_linear=50" / a videovanish_amd.platewarp.PlateWarpConfig refines the tracked translations to one affine map per frame (whole
    blocks matched against the held key, an exact trimmed least-squares fit on the host; rules: include/platewarp.h) and builds and reads the
    canvas through these maps with nearest-neighbour gathers, so that the fill follows zoom and roll; every filled byte is still a byte of
    the clip.  A frame whose fit fails keeps its translation; a locked-off clip and a pure pan give the bytes of the call without it.  What
    it fitted is kept in last_plate_warp.  Without an effective plate_fill and plate_align it is a ValueError.
    plate_grain (clean-plate grain, opt-in, needs plate_fill): "on" / "depth=4,reach=8" / a videovanish_amd.plategrain.PlateGrainConfig makes
    every filled pixel take its bytes from up to `depth` usable frames in turn (the nearest one and the next ones on its side, none more than
    `reach` frames from it; rule: include/vvplategrain.h), so that the grain inside the fill moves as it does around it.  Every filled byte is
    still a byte of the clip at that place; the pixels filled, the masks and last_plate_fill are those of plate_fill alone, on the crop and
    on plate_align's canvas alike, and depth=1 gives its bytes.  What it rotated is kept in last_plate_grain.  Without an effective
    plate_fill it is a ValueError.
    plate_tone (clean-plate exposure matching, opt-in, needs plate_fill): "on" / "mode=affine,ring=32,floor=16,min_pixels=1024,max_gain=25,
    max_offset=32" / a videovanish_amd.platetone.PlateToneConfig fits, per segment, frame and channel, how the frame's exposure differs from the
    segment's mean image over the pixels that are never masked (a gain and an offset, clamped; rules: include/platetone.h), maps the fill's
    crop, widened by `ring`, to the common exposure, runs the unchanged fill on it and maps every filled pixel back to the exposure of the
    frame it lands in, so that a clip whose brightness drifts or flickers by more than the fill's tol is still filled.  Pixels that are not
    filled keep their bytes; a clip without drift gives the bytes of the call without it, and a segment filled on plate_align's canvas is not
    matched.  What it fitted is kept in last_plate_tone.  Without an effective plate_fill it is a ValueError.
    shadow_mask (shadow masking, opt-in): "on" / "guard=1,min_samples=4,tol=6,lo=30,hi=90,drop=12,chroma=20,floor=16,reach=32,min_area=16,grow=1,
    max_bytes=N" / a videovanish_amd.shadowmask.ShadowMaskConfig extends, after the mask clean-up and before the clean-plate fill, every frame's
    mask over the cast shadow of what it covers (infill.shadow_mask; rules: include/vvshadow.h): per segment between the cuts of spans= / cuts=
    and per pixel a clean background is taken from the unmasked frames that are not themselves darkened, the unmasked pixels that look like it
    uniformly darkened are marked, and those that hang on to the frame's mask within `reach` steps join it, grown by `grow`.  Masks change,
    never a frame byte; the larger masks replace the dilated ones for the clean-plate fill, the planners, the prior, the model and the
    composite.  It needs neither plate_fill nor a locked-off camera: where the shot shows no steady background (a pan) nothing is added, and
    the call's bytes are those of the call without it.  What it added is kept in last_shadow_mask.
    overlay_mask (overlay masking, opt-in): "on" / "min_samples=12,mag=8,coh=80,max_share=25,close=2,max_hole=4096,min_area=64,max_area=10,
    border=0,grow=3,max_bytes=N" / a videovanish_amd.overlaymask.OverlayMaskConfig finds, after the mask clean-up and before the shadow
    masking, the screen-fixed graphics of the clip -- a station logo, a channel bug, the frame of a timestamp -- and adds them to the mask of
    every frame (infill.overlay_mask; rules: include/overlaymask.h): over the whole call and per pixel the luma gradients of the unmasked
    frames are summed with their signs and by magnitude, a pixel whose gradient kept its direction is a persistent edge, the edges are
    closed, the holes they enclose filled, and the parts of a plausible size away from the frame's border join the mask, grown by `grow`.
    mask_frames may be all zero: the stage is a mask where none was painted.  Masks change, never a frame byte; the larger masks replace
    the dilated ones for every later stage.  The rule needs the background to travel: a clip in which more than `max_share` percent of the
    strong gradients are persistent is called static, nothing is added and the call's bytes are those of the call without it.  What it
    found, every box included, is kept in last_overlay_mask; find_overlays() gives the same answer without loading a model.
    deflicker (inpaint deflicker, opt-in): "on" / "radius=2,tol=12" / a videovanish_amd.deflicker.DeflickerConfig filters the model's pixels
    along time where they reach the device, for the full frame and for every roi window, inside each span (infill.finish; rules:
    include/vvflicker.h): every pixel becomes the rounded mean of those of its neighbours at most `radius` frames away that lie within `tol`
    levels of it in all three channels.  Flicker is averaged, a moving edge or a real change fails the gate and stays as it is; no byte moves
    more than `tol` levels.  Tone matching, membrane blending and grain matching then measure the filtered rendering, and grain matching puts
    back as moving grain the texture the averaging took out.  Nothing crosses the ends of a span.  What it changed is kept in
    last_deflicker.  radius=0 gives the bytes of the call without it.
    deflicker_align (aligned inpaint deflicker, opt-in, needs deflicker): "on" / "levels=4,radius=4,min_overlap=25,max_residual=12" / a
    videovanish_amd.platealign.PlateAlignConfig tracks, per clip call (per span), one integer translation per frame on the frames and dilated
    masks that call works on (the tracker of plate_align; rules: include/vvalign.h) and reads every temporal neighbour of the filter at the
    place where the same piece of background sits in that neighbour frame (rules: include/vvflickalign.h), so that the patch stops shimmering
    under a pan or tilt too.  A frame the tracker loses takes no sample and gives none; after a cut inside a clip call every later frame is
    lost and stays unfiltered: spans="cuts" (or "masked-cuts") splits the call there.  A locked-off clip gives the bytes of deflicker alone.
    What it found is kept in last_deflicker_align.  Without an effective deflicker it is a ValueError.
    deflicker_local (block-matched inpaint deflicker, opt-in, needs deflicker): "on" / "block=8,search=4,lam=32" / a
    videovanish_amd.deflickerlocal.DeflickerLocalConfig cuts every window into blocks of `block` x `block` pixels and finds, per block and
    temporal neighbour, the integer displacement of at most `search` px whose summed byte difference plus `lam` per px of displacement is
    smallest (block matching on the model's own pixels; rules: include/flicklocal.h); the filter then reads every neighbour along its block's
    vector, so that the patch stops shimmering under parallax, a zoom and in front of a second plane of motion too.  With deflicker_align
    the search starts from the tracked translation.  The gate is unchanged: no byte moves more than the deflicker's `tol`.  search=0 and a
    deflicker of radius 0 give the bytes of the call without it.  What the search found is kept in last_deflicker_local, what the gate then
    accepted in last_deflicker.  Without an effective deflicker it is a ValueError."""
    global last_mask_clean, last_tone_match, last_grain_match, last_seam_blend, last_plate_fill, last_plate_align, last_plate_grain, last_plate_tone, last_shadow_mask, last_deflicker, last_deflicker_align, last_deflicker_local, last_detail_match, last_grain_shape, last_overlay_mask, last_plate_warp
    rcfg = roi_config(roi)
    scfg = spans_config(spans, cuts)
    ccfg = mask_clean_config(mask_clean)
    tcfg = tone_match_config(tone_match)
    gcfg = grain_match_config(grain_match)
    fcfg = deflicker_config(deflicker)
    last_mask_clean = last_tone_match = last_grain_match = last_seam_blend = last_plate_fill = last_plate_align = last_plate_grain = last_plate_tone = last_shadow_mask = last_deflicker = last_deflicker_align = last_deflicker_local = last_detail_match = last_grain_shape = last_overlay_mask = last_plate_warp = None
    dcfg = detail_match_config(detail_match)
    ncfg = grain_shape_config(grain_shape)
    if ncfg is not None and gcfg is None:
        raise ValueError("grain_shape= (grain shape) needs grain_match= (seam grain matching)")
    pcfg = plate_fill_config(plate_fill)
    acfg = plate_align_config(plate_align)
    if acfg is not None and pcfg is None:
        raise ValueError("plate_align= (clean-plate alignment) needs plate_fill= (clean-plate fill)")
    wcfg = plate_warp_config(plate_warp)
    if wcfg is not None and (pcfg is None or acfg is None):
        raise ValueError("plate_warp= (clean-plate warp) needs plate_fill= (clean-plate fill) and plate_align= (clean-plate alignment)")
    lcfg = plate_grain_config(plate_grain)
    if lcfg is not None and pcfg is None:
        raise ValueError("plate_grain= (clean-plate grain) needs plate_fill= (clean-plate fill)")
    ecfg = plate_tone_config(plate_tone)
    if ecfg is not None and pcfg is None:
        raise ValueError("plate_tone= (clean-plate exposure matching) needs plate_fill= (clean-plate fill)")
    hcfg = shadow_mask_config(shadow_mask)
    ocfg = overlay_mask_config(overlay_mask)
    facfg = deflicker_align_config(deflicker_align)
    if facfg is not None and fcfg is None:
        raise ValueError("deflicker_align= (aligned inpaint deflicker) needs deflicker= (inpaint deflicker)")
    flcfg = deflicker_local_config(deflicker_local)
    if flcfg is not None and fcfg is None:
        raise ValueError("deflicker_local= (block-matched inpaint deflicker) needs deflicker= (inpaint deflicker)")
    bcfg = seam_blend_config(seam_blend, feather_px if keep_unmasked_original else None)
    if compat_reference_early_return:
        on = dict(roi=rcfg, spans=scfg, mask_clean=ccfg, tone_match=tcfg, grain_match=gcfg, seam_blend=bcfg, plate_fill=pcfg, plate_align=acfg,
                  plate_grain=lcfg, plate_tone=ecfg, shadow_mask=hcfg, deflicker=fcfg, deflicker_align=facfg, deflicker_local=flcfg, detail_match=dcfg, grain_shape=ncfg, overlay_mask=ocfg, plate_warp=wcfg)
        for o in ALL_OPTIONS:
            if on[o.name] is not None:
                raise ValueError(f"{o.name}= ({o.phrase}) cannot be combined with compat_reference_early_return=True")

    if prog is not None: prog(5, "dilating frames")
    dev = get_device()
    m = torch.from_numpy(np.stack([mm if mm.ndim == 3 else mm[..., None] for mm in mask_frames])).to(dev)
    dil_t = hip.mask_collapse_dilate(m.contiguous(), mask_dilation_iter)       # reference :27-31
    if ccfg is not None:
        find = None if scfg is None else (lambda despeckled: infill.clip_cuts(frames_rgb, despeckled, scfg))
        dil_t, last_mask_clean = infill.clean_masks(m.contiguous(), dil_t, ccfg, find)
        if scfg is not None and scfg.cuts == "auto":        # the detector has run, on the despeckled masks: the span plan takes its cuts
            import dataclasses
            scfg = dataclasses.replace(scfg, cuts=last_mask_clean.cuts)
    if ocfg is not None:        # before the cut detector and both plate stages: none of them samples the graphic as background
        dil_t, last_overlay_mask = infill.overlay_mask(frames_rgb, dil_t, ocfg)
    if hcfg is not None or pcfg is not None:
        found = None if scfg is None else infill.clip_cuts(frames_rgb, dil_t, scfg)
        if scfg is not None and scfg.cuts == "auto":        # the detector has run, once for both stages: the span plan takes its cuts
            import dataclasses
            scfg = dataclasses.replace(scfg, cuts=tuple(found))
    if hcfg is not None:
        dil_t, last_shadow_mask = infill.shadow_mask(frames_rgb, dil_t, hcfg, found)
    if pcfg is not None:
        more, found_align, found_grain, found_tone, found_warp = {}, [], [], [], []
        if acfg is not None:
            more.update(acfg=acfg, align_out=found_align)
        if wcfg is not None:
            more.update(wcfg=wcfg, warp_out=found_warp)
        if lcfg is not None:
            more.update(gcfg=lcfg, grain_out=found_grain)
        if ecfg is not None:
            more.update(tcfg=ecfg, tone_out=found_tone)
        frames_rgb, dil_t, last_plate_fill = infill.plate_fill(frames_rgb, dil_t, pcfg, found, **more)      # downstream these are the originals
        if acfg is not None:
            last_plate_align = found_align[0]
        if wcfg is not None:
            last_plate_warp = found_warp[0]
        if lcfg is not None:
            last_plate_grain = found_grain[0]
        if ecfg is not None:
            last_plate_tone = found_tone[0]

    stages = infill.Stages(lambda: _load_model(dev, ckpt), _load_prior, _run_prior,
                           lambda f, d, prior, p: _run_model(f, d, prior, max_img_size, p, num_inference_steps, scheduler))

    seam = {}               # finish's keywords of the stages that are on; each *_out list gets one report per clip call, in the order of the spans
    for key, cfg in (("tone", tcfg), ("grain", gcfg), ("blend", bcfg), ("flicker", fcfg), ("flicker_align", facfg), ("detail", dcfg),
                     ("grain_shape", ncfg), ("flicker_local", flcfg)):
        if cfg is not None:
            seam.update({key: cfg, key + "_out": []})

    def body(frames, dil, prior, p, **at):          # at: frame0, which run_spans passes when grain matching is on
        return infill.run_clip(frames, dil, prior, rcfg, stages, p, dev, feather_px, keep_unmasked_original, compat_reference_early_return, **seam, **at)

    T = len(frames_rgb)
    if scfg is None:
        plan = [(0, T)]
        out = body(frames_rgb, dil_t, propainer_frames, prog)
    else:
        plan = infill.span_plan(frames_rgb, dil_t, scfg)
        more = {} if gcfg is None else dict(frame0=True)        # each span's clip call learns where it starts
        out = infill.run_spans(frames_rgb, dil_t, propainer_frames, plan, body, prog, load=stages.load_model, **more)
    if tcfg is not None:
        last_tone_match = infill.tone_report(seam["tone_out"], plan, T)
    if gcfg is not None:
        last_grain_match = infill.grain_report(seam["grain_out"], plan, T)
    if bcfg is not None:
        last_seam_blend = infill.seam_blend_report(seam["blend_out"], plan, T)
    if fcfg is not None:
        last_deflicker = infill.deflicker_report(seam["flicker_out"], plan, T)
    if facfg is not None:
        last_deflicker_align = infill.deflicker_align_report(seam["flicker_align_out"], plan)
    if flcfg is not None:
        last_deflicker_local = infill.deflicker_local_report(seam["flicker_local_out"], plan, T)
    if dcfg is not None:
        last_detail_match = infill.detail_report(seam["detail_out"], plan, T)
    if ncfg is not None:
        last_grain_shape = infill.grain_shape_report(seam["grain_shape_out"], plan, T)
    return out


def find_overlays(frames_rgb, mask_frames=None, overlay_mask="on"):
    """The overlay masking alone, for a preview in a GUI or a script: frames_rgb = the clip's frames [H,W,3] u8, mask_frames = masks of their
    size ([H,W] or [H,W,ch], non-zero = masked: those pixels give no sample in their frame; they are taken as they are, not dilated) or None
    (no mask), overlay_mask = "on" / a settings string / a videovanish_amd.overlaymask.OverlayMaskConfig.  -> (overlay [H,W] u8 {0, 255}: the
    pixels run_infill_on_frames(..., overlay_mask=...) would add to every frame's mask; the infill.OverlayMaskReport with the verdict and
    every box).  Loads no model and changes no module state; "off" is a ValueError."""
    ocfg = overlaymask.as_config(overlay_mask)
    if ocfg is None:
        raise ValueError("find_overlays: overlay_mask= must name a setting ('on', 'mag=8,...' or an OverlayMaskConfig), not switch the stage off")
    H, W = frames_rgb[0].shape[:2]
    if mask_frames is None:
        dil = np.zeros((len(frames_rgb), H, W), np.uint8)
    else:
        dil = np.stack([((mm != 0).any(axis=2) if mm.ndim == 3 else mm != 0) for mm in mask_frames]).astype(np.uint8) * 255
    _, report = infill.overlay_mask(frames_rgb, torch.from_numpy(dil).to(get_device()), ocfg)
    return report.overlay, report


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


def _setting_arg(name):
    """The argparse type of an option's command-line value: checked while the arguments are parsed and passed on as written ("off" is refused,
    as for --roi / --spans)."""
    def check(text):
        try:
            if _OPTION[name].settings.as_config(text) is None:
                raise ValueError("not a setting")
        except ValueError as e:
            raise argparse.ArgumentTypeError(str(e))
        return text
    return check


# =============================
# CLI entry point (reference diffuerase.py:121-155)
# =============================
def main():
    tools = _frame_io()
    ap = argparse.ArgumentParser(description="Remove masked objects from a video (DiffuEraser hot path on MI355X).")
    ap.add_argument("--color_video", required=True, type=str, help="Input color video path.")
    ap.add_argument("--mask_video", required=False, type=str, help="Input mask video path (required unless --overlay-mask is given: then no "
                                                                   "mask video means all-zero masks).")
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
    ap.add_argument("--mask-clean", type=_setting_arg("mask_clean"), default=None, metavar=_OPTION["mask_clean"].metavar,
                    help="Mask clean-up before anything reads the masks: drop components of the dilated mask that hold fewer than `area` mask pixels "
                         "(on: four cells of a 256 x 256 grid at the clip's size), fill dropouts of at most `bridge` frames (on: 2), hold the mask "
                         "`grow` frames longer at both ends (on: 0).  Prints one line with what it changed.")
    ap.add_argument("--tone-match", type=_setting_arg("tone_match"), default=None, metavar=_OPTION["tone_match"].metavar,
                    help="Seam tone matching before the composite: per frame and channel, fit the model's pixels to the original ones over the ring of "
                         "unmasked pixels within `ring` px of the mask (on: a gain and an offset, ring 12, pooled over 2 frames either side; offset: "
                         "an offset only) and correct every pasted pixel with it.  Prints one line with what it applied.")
    ap.add_argument("--grain-match", type=_setting_arg("grain_match"), default=None, metavar=_OPTION["grain_match"].metavar,
                    help="Seam grain matching before the composite: measure, over the flat part of the ring of unmasked pixels within `ring` px of the "
                         "mask, the grain the original pixels have and the model's lack, and add white noise of that level to every pasted pixel (on / "
                         "luma: one noise value per pixel; rgb: one per channel).  Prints one line with what it added.")
    ap.add_argument("--grain-shape", type=_setting_arg("grain_shape"), default=None, metavar=_OPTION["grain_shape"].metavar,
                    help="With --grain-match: fit the SIZE of the grain on the same ring as well (per axis the a of a kernel [a, 1, a], 0 = white, "
                         "0.5 = the binomial blur), correct the level that the white estimate under-reads on soft grain, and add noise shaped by "
                         "that kernel.  For footage that was resized, debayered, denoised or compressed.  Prints one line with what it fitted.")
    ap.add_argument("--seam-blend", type=_setting_arg("seam_blend"), default=None, metavar=_OPTION["seam_blend"].metavar,
                    help="Seam membrane blending before the composite: interpolate the difference original - model from the ring of unmasked pixels "
                         "within `ring` px of the mask harmonically into the hole and add it to every pasted pixel, so that the patch meets the "
                         "original along the whole outline (a correction that varies across the hole).  Prints one line with what it added.")
    ap.add_argument("--detail-match", type=_setting_arg("detail_match"), default=None, metavar=_OPTION["detail_match"].metavar,
                    help="Seam detail matching before the other seam stages: fit, over the structured part of the ring of unmasked pixels within "
                         "`ring` px of the mask, how much of its own 3 x 3 high-pass the model's rendering lacks (or has too much of) against the "
                         "original, and sharpen (or soften) every pasted pixel by that amount, clamped to its neighbourhood's range plus `overshoot`.  "
                         "Prints one line with what it applied.")
    ap.add_argument("--plate-fill", type=_setting_arg("plate_fill"), default=None, metavar=_OPTION["plate_fill"].metavar,
                    help="Clean-plate fill before anything plans or runs the model: a masked pixel whose background the same shot shows steadily (a "
                         "standard deviation of at most `tol` over at least `min_samples` unmasked frames, `guard` frames away from the mask) is filled "
                         "from the nearest such frame and leaves the mask; what is never revealed stays with the model.  For locked-off shots.  "
                         "Prints one line with what it filled.")
    ap.add_argument("--plate-align", type=_setting_arg("plate_align"), default=None, metavar=_OPTION["plate_align"].metavar,
                    help="With --plate-fill: track one integer translation per frame first (a coarse-to-fine search over `levels` pyramid levels, "
                         "+-`radius` at the coarsest; a frame whose best match differs by more than `max_residual` levels on average is left out) "
                         "and fill on the canvas in which the background stands still.  For slow pans and tilts.  Prints one line with what it tracked.")
    ap.add_argument("--plate-warp", type=_setting_arg("plate_warp"), default=None, metavar=_OPTION["plate_warp"].metavar,
                    help="With --plate-fill and --plate-align: match `block`-pixel blocks of every tracked frame against its key frame +-`search` px round "
                         "the tracked translation, fit one affine map per frame to the blocks' vectors (exact least squares, blocks further than "
                         "`trim` tenths of a pixel from the fit dropped, at least `min_blocks` kept, linear coefficients up to `max_linear` thousandths) "
                         "and fill on the canvas built through these maps.  For handheld and gimbal shots: zoom and roll.  Prints one line with what it fitted.")
    ap.add_argument("--plate-grain", type=_setting_arg("plate_grain"), default=None, metavar=_OPTION["plate_grain"].metavar,
                    help="With --plate-fill: a filled pixel takes its bytes from up to `depth` usable frames in turn (the nearest and the next ones on "
                         "its side, at most `reach` frames from it), not from the nearest alone, so that the grain inside the fill moves as it does "
                         "around it.  Prints one line with what it rotated.")
    ap.add_argument("--plate-tone", type=_setting_arg("plate_tone"), default=None, metavar=_OPTION["plate_tone"].metavar,
                    help="With --plate-fill: fit, per segment, frame and channel, a gain and an offset (mode=gain, mode=offset: one of them) between the "
                         "frame and the segment's mean image over the pixels that are never masked, run the fill at that common exposure and map "
                         "every filled pixel back to its own frame's, so that exposure drift and flicker beyond the fill's tol still fill.  "
                         "Prints one line with what it matched.")
    ap.add_argument("--shadow-mask", type=_setting_arg("shadow_mask"), default=None, metavar=_OPTION["shadow_mask"].metavar,
                    help="Shadow masking before the clean-plate fill: extend every frame's mask over the cast shadow of what it covers.  Unmasked "
                         "pixels at `lo` .. `hi` percent of the shot's clean background (at least `drop` levels darker, the three channels within "
                         "`chroma` points of each other) that hang on to the mask within `reach` steps join it, grown by `grow`; parts under "
                         "`min_area` pixels are dropped.  Changes masks only.  Prints one line with what it added.")
    ap.add_argument("--overlay-mask", type=_setting_arg("overlay_mask"), default=None, metavar=_OPTION["overlay_mask"].metavar,
                    help="Overlay masking before the shadow masking: find the screen-fixed graphics of the clip (a station logo, a channel bug) from "
                         "the edges that stand still while the picture under them moves (mean gradient at least `mag`, `coh` percent of it in one "
                         "direction), close them, fill what they enclose and add the parts of `min_area` pixels to `max_area` percent of the frame, "
                         "grown by `grow`, to every frame's mask.  Needs a moving background; --mask_video becomes optional.  Changes masks only.  "
                         "Prints one line with what it found.")
    ap.add_argument("--deflicker", type=_setting_arg("deflicker"), default=None, metavar=_OPTION["deflicker"].metavar,
                    help="Inpaint deflicker before the seam stages: every pixel of the model's output becomes the mean of those of its neighbours at "
                         "most `radius` frames away (on: 2) that lie within `tol` levels of it (on: 12), so the patch stops shimmering; what changes by "
                         "more (a moving edge) stays as it is.  Prints one line with what it changed.")
    ap.add_argument("--deflicker-align", type=_setting_arg("deflicker_align"), default=None, metavar=_OPTION["deflicker_align"].metavar,
                    help="With --deflicker: track one integer translation per frame first (the tracker of --plate-align, per span) and read the "
                         "filter's temporal neighbours along it, so the patch stops shimmering under a pan or tilt too.  A frame the tracker "
                         "loses stays unfiltered; split at cuts with --spans cuts.  Prints one line with what it tracked.")
    ap.add_argument("--deflicker-local", type=_setting_arg("deflicker_local"), default=None, metavar=_OPTION["deflicker_local"].metavar,
                    help="With --deflicker: find one integer displacement per `block` x `block` pixels and temporal neighbour first (block matching "
                         "within +-`search` px, `lam` per px of displacement against flat blocks' wandering) and read the filter's temporal "
                         "neighbours along it, so the patch stops shimmering under parallax, a zoom and in front of moving background too.  "
                         "Composes with --deflicker-align.  Prints one line with what it found.")
    ap.add_argument("--cuts", type=span_plan.parse_cuts, default=None, metavar="120,431",
                    help="Frame indices (relative to --start_frame) where a new shot begins: used instead of the detector.")
    args = ap.parse_args()
    if args.mask_video is None and args.overlay_mask is None:
        ap.error("the following arguments are required: --mask_video (or --overlay-mask, which finds a mask where none was painted)")

    assert os.path.isfile(args.color_video), "input video missing"
    out_video = args.out or (args.color_video + "_vanished.mkv")
    frames, fps = tools.load_video_frames_from_path(args.color_video, args.start_frame, args.max_frames)
    H0, W0 = frames[0].shape[:2]
    if args.mask_video is None:
        mask_frames = [np.zeros((H0, W0), np.uint8) for _ in frames]
    else:
        mask_frames, mask_fps = tools.load_video_frames_from_path(args.mask_video, args.start_frame, args.max_frames)
    Hm, Wm = mask_frames[0].shape[:2]
    prior_frames = None
    if args.prior_video is not None:      # the reference's test is inverted (:142); a supplied prior is used here
        prior_frames, prior_fps = tools.load_video_frames_from_path(args.prior_video, args.start_frame, args.max_frames)
        Hp, Wp = prior_frames[0].shape[:2]
        assert (H0 == Hp and W0 == Wp), "prior and color video are diffrent sizes"
    assert (H0 == Hm and W0 == Wm), "mask and color video are diffrent sizes"
    # pass roi= / spans= / cuts= / a stage only when asked for: a default call stays the reference's call
    kw = {name: getattr(args, name) for name in [o.name for o in ALL_OPTIONS] + ["cuts"] if getattr(args, name) is not None}
    out_frames = run_infill_on_frames(frames, mask_frames, propainer_frames=prior_frames, **kw)
    if args.mask_clean is not None and last_mask_clean is not None:
        r = last_mask_clean
        print(f"mask clean-up: {int(r.removed.sum())} components ({int(r.cleared.sum())} px) cleared in {int((r.removed > 0).sum())} frames, "
              f"{int(r.bridged.sum())} px bridged in {int((r.bridged > 0).sum())} frames, {int(r.grown.sum())} px grown in {int((r.grown > 0).sum())} frames")
    if args.tone_match is not None and last_tone_match is not None:
        r = last_tone_match
        changed = (r.gain != 1.0).any(axis=(0, 2)) | (r.offset != 0.0).any(axis=(0, 2))
        print(f"tone match: {int(changed.sum())} of {changed.size} frames corrected, largest |gain - 1| {float(np.abs(r.gain - 1.0).max()):.4f}, "
              f"largest |offset| {float(np.abs(r.offset).max()):.2f}")
    if args.grain_match is not None and last_grain_match is not None:
        r = last_grain_match
        touched = (r.sigma_added > 0.0).any(axis=(0, 2, 3))
        print(f"grain match: grain added in {int(touched.sum())} of {touched.size} frames, largest sigma {float(r.sigma_added.max()):.2f}")
    if args.grain_shape is not None and last_grain_shape is not None:
        r = last_grain_shape
        shaped = (r.a > 0.0).any(axis=(0, 2, 3))
        print(f"grain shape: grain shaped in {int(shaped.sum())} of {shaped.size} frames, largest a {float(r.a.max(initial=0.0)):.3f}, "
              f"largest level gain {float(r.k.max(initial=1.0)):.2f}, largest sigma {float(r.sigma_pixel.max(initial=0.0)):.2f}")
    if args.seam_blend is not None and last_seam_blend is not None:
        r = last_seam_blend
        touched = (r.max_shift > 0.0).any(axis=(0, 2))
        print(f"seam blend: membrane added in {int(touched.sum())} of {touched.size} frames, largest |shift| {float(r.max_shift.max()):.2f}, "
              f"largest ring RMS {float(r.rms_diff.max()):.2f}")
    if args.detail_match is not None and last_detail_match is not None:
        r = last_detail_match
        matched, unfit = (r.amount != 0.0).any(axis=0), ((r.amount == 0.0) & ~r.dead).all(axis=0)
        print(f"detail match: {int(matched.sum())} of {matched.size} frames matched, largest sharpen {float(max(r.amount.max(initial=0.0), 0.0)):.3f}, "
              f"largest soften {float(max(-r.amount.min(initial=0.0), 0.0)):.3f}, {int(unfit.sum())} frames unfit")
    if args.plate_fill is not None and last_plate_fill is not None:
        r = last_plate_fill
        print(f"plate fill: {int(r.filled.sum())} px filled in {int((r.filled > 0).sum())} frames, {int(r.left.sum())} px left to the model in "
              f"{int((r.left > 0).sum())} of {r.left.size} frames, {sum(r.skipped)} of {len(r.segments)} segments skipped")
    if args.plate_align is not None and last_plate_align is not None:
        r = last_plate_align
        ok = np.concatenate(r.tracked)
        span = [int(o[k][:, a].max() - o[k][:, a].min()) if k.any() else 0 for a in (0, 1) for o, k in zip(r.off, r.tracked)]
        n = len(r.segments)
        print(f"plate align: {int(ok.sum())} of {ok.size} frames tracked, pan extent {max(span[:n])} x {max(span[n:])} px, "
              f"{sum(p == 'canvas' for p in r.path)} of {n} segments filled on a canvas")
    if args.plate_warp is not None and last_plate_warp is not None:
        r = last_plate_warp
        failed, kept = np.concatenate(r.failed), np.concatenate(r.kept)
        lin = np.concatenate([np.abs(m[:, [1, 2, 4, 5]] - np.array([1.0, 0.0, 0.0, 1.0])).max(axis=1) for m in r.maps]) if len(r.maps) else np.zeros(0)
        print(f"plate warp: {int((kept > 0).sum())} of {kept.size} frames fitted, {int(failed.sum())} fits failed, largest linear coefficient "
              f"{float(np.nanmax(lin, initial=0.0)):.4f}, largest rms {float(np.concatenate(r.rms).max(initial=0.0)):.2f} px, "
              f"{sum(p == 'warp' for p in r.path)} of {len(r.segments)} segments filled on a warped canvas")
    if args.plate_grain is not None and last_plate_grain is not None:
        r = last_plate_grain
        filled, rotated = int(r.filled.sum()), int(r.rotated.sum())
        print(f"plate grain: {filled} px filled, {100.0 * rotated / max(filled, 1):.1f} % of them from another frame than the nearest")
    if args.plate_tone is not None and last_plate_tone is not None:
        r = last_plate_tone
        print(f"plate tone: {int((~r.identity).sum())} of {r.identity.size} frames matched, largest |gain - 1| {float(np.abs(r.gain - 1.0).max(initial=0.0)):.4f}, "
              f"largest |offset| {float(np.abs(r.offset).max(initial=0.0)):.2f}, {sum(p == 'unfit' for p in r.path)} segments unfit, "
              f"{sum(p == 'canvas' for p in r.path)} on the canvas, of {len(r.segments)}")
    if args.shadow_mask is not None and last_shadow_mask is not None:
        r = last_shadow_mask
        print(f"shadow mask: {int(r.added.sum())} px added in {int((r.added > 0).sum())} of {r.added.size} frames from {int(r.candidates.sum())} candidate px, "
              f"{sum(r.skipped)} of {len(r.segments)} segments skipped")
    if args.overlay_mask is not None and last_overlay_mask is not None:
        r = last_overlay_mask
        boxes = ", ".join(f"{x1 - x0} x {y1 - y0} at ({x0}, {y0}), {area} px" for x0, y0, x1, y1, area in r.boxes.tolist()) or "no box"
        print(f"overlay mask: {r.verdict}, {r.found} overlays ({boxes}), {int(r.overlay.astype(bool).sum())} px in the overlay, "
              f"{int(r.added.min())} .. {int(r.added.max())} px added per frame, {r.edges} of {r.strong} strong px persistent")
    if args.deflicker is not None and last_deflicker is not None:
        r = last_deflicker
        touched = (r.changed > 0).any(axis=0)
        inside = int(r.n_mask.sum())
        mean_n = float((r.samples_mask * r.n_mask).sum() / inside) if inside else 0.0
        print(f"deflicker: {int(touched.sum())} of {touched.size} frames changed, mean accepted samples inside the mask {mean_n:.2f}, "
              f"largest mean |shift| {float(r.shift.max(initial=0.0)):.2f}")
    if args.deflicker_align is not None and last_deflicker_align is not None:
        r = last_deflicker_align
        paths = ", ".join(f"{sum(p == name for p in r.path)} {name}" for name in deflickeralign.PATHS if name in r.path) or "no clip call"
        lost = sum(int((~k).sum()) for k in r.tracked)
        far = max([int(np.abs(o[k]).max()) for o, k in zip(r.off, r.tracked) if k.any()] + [0])
        print(f"deflicker align: {len(r.path)} clip calls ({paths}), {lost} of {sum(len(k) for k in r.tracked)} frames lost, largest |offset| {far} px")
    if args.deflicker_local is not None and last_deflicker_local is not None:
        r = last_deflicker_local
        matched, inside = int(r.blocks.sum()), 0 if last_deflicker is None else int(last_deflicker.n_mask.sum())
        mean_n = float((last_deflicker.samples_mask * last_deflicker.n_mask).sum() / inside) if inside else 0.0
        print(f"deflicker local: {matched} blocks matched, {100.0 * int(r.moved.sum()) / max(matched, 1):.1f} % of them moved, largest |vector| "
              f"{int(r.max_vector.max(initial=0))} px, mean accepted samples inside the mask {mean_n:.2f}")
    tools.write_video_frames_to_path(out_video, out_frames, fps, H0, W0)


if __name__ == '__main__':
    main()

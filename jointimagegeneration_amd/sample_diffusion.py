"""LDM conditional CT sampling entry point: `python -m jointimagegeneration_amd.sample_diffusion -r <logdir|ckpt> -c 50`.

Re-creates the CLI, config and checkpoint surface of latentdiffusion/sample_diffusion.py:165-273,356-433,492-570:
`-r/--resume` (logdir or .ckpt), `-n/--n_samples`, `-e/--eta`, `-c/--custom_steps`, `-l/--logdir`, `--batch_size`, dot-list
overrides; config = logdir/configs/*.yaml merged (+ dot-list); model = instantiate_from_config(config.model) with the
checkpoint's "state_dict" loaded strict=False; sampling under model.ema_scope().  `sample_cond` keeps the reference's
slice loop exactly (Python indexing quirks included) on the reference-shaped API (get_learned_conditioning /
DDIMSampler.sample / decode_first_stage); `GuideGenPipeline.sample_ct` is the all-device fast path of the same loop.
With `--gt DIR --lpips-vgg PATH --lpips-lin PATH` each sampled volume is scored against the same-named volume of DIR with the
three-view LPIPS of compute_metrics (sample_diffusion.py:436-475; jointimagegeneration_amd/lpips.py) and metrics.json is written next to
the samples.  With `--png` each sampled volume is also rendered as `<stem>_<ix:04d>.png`: the organ overlay and slice grid of
sample_diffusion.py:241-261 (jointimagegeneration_amd/render.py).  With `-v --progress-png [--log-every-t K]` the last generated slice
is sampled by `progressive_denoising` (sample_diffusion.py:116-122) and its denoise row -- the decoded predictions of x_0 at the logged
timesteps, one row per sample (ddpm.py:539-549) -- is written as `<stem>_progress.png`.  FVD (no I3D network or scripts.fvd in the reference), the per-slice
`layers/*.png` and the private datasets are out of scope; the mask comes from `--inputs <dir>` (the
`pred_*.nii.gz` label volumes the stage-1 entry point ddpm_eval writes: the hand-off of README.md:21, one CT volume per mask),
from --mask (.npy label volume [D,H,W]) or is synthetic.
CT editing (this package's addition): with `--inputs DIR --known-ct DIR` and one of `--known-mask DIR` (the original label
volumes) and `--keep-mask DIR` (explicit keep volumes), all paired by stem, each volume runs through
`GuideGenPipeline.sample_ct_volumes(known_ct=, keep=, edit_margin=--edit-margin)`: kept voxels of the known CT come back bit for bit, the
rest is regenerated, and metrics.json gains an `edit` block.
"""
from __future__ import annotations

import argparse
import glob
import os
import sys
import time

import numpy as np
import torch

from .config import apply_dotlist, instantiate_from_config, load_yaml, merge
from . import ops
from .io import load_checkpoint, read_nifti, write_nifti, write_png
from .ldm import DDIMSampler, PLMSSampler
from .pipeline import DISCRETIZATIONS, check_sampler_options
from .render import volume_png
from .synth import randomize_parameters, synth_mask_volume


SAMPLERS = tuple(DISCRETIZATIONS)                     # ddim, plms, dpmpp_2m


def get_parser():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("-r", "--resume", type=str, nargs="?", help="load from logdir or checkpoint in logdir")
    p.add_argument("-n", "--n_samples", type=int, nargs="?", default=1, help="number of samples to draw")
    p.add_argument("-e", "--eta", type=float, nargs="?", default=0.0, help="eta for ddim sampling (0.0 yields deterministic sampling)")
    p.add_argument("-v", "--vanilla_sample", default=False, action="store_true", help="vanilla ancestral sampling (default: DDIM)")
    p.add_argument("--plms", default=False, action="store_true", help="PLMS sampler instead of DDIM")
    p.add_argument("--sampler", choices=SAMPLERS, default=None, help="latent sampler (default ddim; --plms is --sampler plms): dpmpp_2m is "
                   "DPM-Solver++ 2M, a second-order multistep solver meant for about 20 steps (-c 20), eta 0 only")
    p.add_argument("--discretize", choices=("uniform", "quad", "logsnr"), default=None, help="step grid: uniform (the default of ddim / plms), "
                   "quad, or logsnr (dpmpp_2m only, and its default: steps uniform in the log-SNR)")
    p.add_argument("-l", "--logdir", type=str, nargs="?", default="none", help="extra logdir")
    p.add_argument("-c", "--custom_steps", type=int, nargs="?", default=50, help="number of steps for ddim sampling")
    p.add_argument("--batch_size", type=int, nargs="?", default=1)
    p.add_argument("--config", type=str, default=None, help="model yaml when -r is not a log directory")
    p.add_argument("--inputs", type=str, default=None, help="directory of stage-1 label volumes (*.nii.gz / *.nii, as ddpm_eval writes them): "
                   "each is zoomed (order 0) to --slices x --size x --size, rotated and scaled as the reference recipe does, and gets its own CT volume")
    p.add_argument("--mask", type=str, default=None, help=".npy label volume [D,H,W] (labels 0..11); default synthetic ellipsoids")
    p.add_argument("--slices", type=int, default=64)
    p.add_argument("--size", type=int, default=512)
    p.add_argument("--seed", type=int, default=2048)
    p.add_argument("--gt", type=str, default=None, help="directory of ground-truth CT volumes named like the samples (<stem>_<ix:04d>.nii.gz): "
                   "with --lpips-vgg and --lpips-lin each sample is scored against it (three-view LPIPS) and metrics.json is written next to the samples")
    p.add_argument("--lpips-vgg", type=str, default=None, help="VGG16 feature state dict (torchvision's features.N.* names or net.sliceK.N.*)")
    p.add_argument("--lpips-lin", type=str, default=None, help="lpips checkpoint with linK.model.1.weight")
    p.add_argument("--png", default=False, action="store_true", help="render each sampled volume as <stem>_<ix:04d>.png beside its NIfTI file: "
                   "the mask blended over the CT at 20 %% with organ boundaries, slices tiled 8 per row.  The overlay is given the mask as "
                   "label / 11, the convention its colour table needs; the reference's own call passes label / 255, for which no organ is painted")
    p.add_argument("--progress-png", default=False, action="store_true", help="with -v: sample the last generated slice with "
                   "progressive_denoising and write its denoise row (decoded x_0 predictions at the logged timesteps) as <stem>_progress.png")
    p.add_argument("--log-every-t", type=int, default=None, help="with --progress-png: log every K-th timestep (default: the model's log_every_t)")
    p.add_argument("--known-ct", type=str, default=None, help="CT editing (with --inputs): directory of known CT volumes (NIfTI, fp32 in [0, 1], already "
                   "--slices x --size x --size; nothing is resampled), paired with the --inputs label volumes by stem.  Kept voxels come back bit for bit")
    p.add_argument("--known-mask", type=str, default=None, help="with --known-ct: directory of the ORIGINAL label volumes (same stems): a voxel is kept "
                   "where the edited and the original label condition the slice loop alike")
    p.add_argument("--keep-mask", type=str, default=None, help="with --known-ct: directory of explicit uint8 keep volumes (same stems, --slices x --size x "
                   "--size, non-zero = keep), instead of --known-mask")
    p.add_argument("--largest-component", default=None, help="with --inputs: 'all' or comma-separated classes; keep only the largest connected "
                   "component of these classes of every stage-1 mask before the slice loop (postprocess.clean; metrics.json gains a mask_cleanup block)")
    p.add_argument("--min-component", type=int, default=None, help="with --inputs: remove every component of a stage-1 mask below this many voxels")
    p.add_argument("--connectivity", type=int, default=None, help="with --inputs: 6 (faces, the default) or 26 (faces, edges, corners)")
    p.add_argument("--edit-margin", type=int, default=0, help="with --known-ct: latent cells within R cells of an un-kept pixel are regenerated too")
    return p


def sampler_from_options(opt):
    """(sampler name, grid or None) of --sampler / --plms / --discretize / -e, refused by name before a model is loaded."""
    name = opt.sampler or ("plms" if opt.plms else "ddim")
    if opt.plms and name != "plms":
        raise SystemExit(f"--plms contradicts --sampler {name}")
    try:
        check_sampler_options(name, opt.discretize, SAMPLERS)
    except ValueError as e:
        raise SystemExit(f"--sampler / --discretize: {e}") from None
    if name == "dpmpp_2m" and opt.eta != 0:
        raise SystemExit(f"--sampler dpmpp_2m: eta = {opt.eta} is not supported (the solver is deterministic; -e must be 0)")
    if name == "dpmpp_2m" and opt.vanilla_sample:
        raise SystemExit("--sampler dpmpp_2m contradicts -v / --vanilla_sample (ancestral sampling)")
    return name, opt.discretize


def make_sampler(model, name: str):
    if name == "dpmpp_2m":
        from .dpm_solver import DPMSolverSampler
        return DPMSolverSampler(model)
    return PLMSSampler(model) if name == "plms" else DDIMSampler(model)


def load_model_from_config(config, sd):
    model = instantiate_from_config(config)
    if sd is not None:
        model.load_state_dict(sd, strict=False)
    model.cuda()
    model.eval()
    return model


def load_model(config, ckpt):
    if ckpt and os.path.exists(ckpt):
        pl_sd = load_checkpoint(ckpt)
        global_step = pl_sd.get("global_step", 0)
        model = load_model_from_config(config["model"], pl_sd["state_dict"])
    else:
        print(f"checkpoint {ckpt!r} not found: random-init weights from the seed recipe (synthetic run)", file=sys.stderr)
        model = instantiate_from_config(config["model"])
        randomize_parameters(model, 1024, "ldm.")
        if getattr(model, "use_ema", False):
            model.model_ema.reset_from(model.model)        # the EMA shadow is what ema_scope() samples with
        model.cuda().eval()
        global_step = 0
    return model, global_step


def strip_ckpt_paths(cfg):
    """yaml ckpt_path entries point at the authors' cluster (/mnt/...); sub-model weights come from the main checkpoint."""
    if isinstance(cfg, dict):
        return {k: (None if k == "ckpt_path" and isinstance(v, str) and not os.path.exists(v) else strip_ckpt_paths(v)) for k, v in cfg.items()}
    return cfg


@torch.no_grad()
def stage1_mask_to_wholemask(labels, depth: int, hw: int) -> torch.Tensor:
    """The commented recipe of latentdiffusion/sample_diffusion.py:199-200 on the device: a stage-1 label volume [Dm, Hm, Wm] ->
    `rot90(scipy.ndimage.zoom(mask, (depth, hw, hw) / mask.shape, order=0), k=3, dims=(1, 2)) / 255` as fp32 [depth, hw, hw], through the
    glue kernel the all-device pipeline uses per slice (gg_mask_to_cond_slice: scipy's order-0 index rule in IEEE double)."""
    lab = torch.as_tensor(np.ascontiguousarray(labels)).to(device="cuda", dtype=torch.int32)[None].contiguous()
    vol = torch.empty((depth, hw, hw), dtype=torch.float32, device=lab.device)
    scratch = torch.empty((1, 1, hw, hw, 32), dtype=torch.bfloat16, device=lab.device)
    for d in range(depth):
        ops.mask_to_cond_slice(lab, d, depth, hw, hw, None, scratch, mask_out=vol[d])
    return vol


@torch.no_grad()
def sample_cond(model, instance, n_samples=1, ddim_steps=50, ddim_eta=0.0, noise_seed=None, vanilla=False, plms=False, x_T_tape=None,
                progress=None, sampler_name=None, discretize=None, record=None):
    """The reference slice loop (sample_diffusion.py:196-224) on the reference-shaped API. instance["wholemask"] is
    [1, D, H, W, 1] (label/255); returns pred [n, 2, D, H, W] = cat([samples, gen_mask]).  `x_T_tape` (parity runs): one
    [n, C, h, w] start latent per generated slice, in loop order, instead of the generator draw of ddim.py:124.  `progress` (a dict, with
    vanilla): the last slice is sampled by progressive_denoising(log_every_t=progress.get("log_every_t")) and its list of x_0 predictions
    is left in progress["intermediates"]; the other slices, and every call without it, run as before.  `sampler_name` ("ddim" | "plms" |
    "dpmpp_2m"; None: `plms` decides) and `discretize` (None: the sampler's default grid) choose the sampler; `record` (a dict) receives
    the sampler, the grid and the chain's own step count."""
    sampler = make_sampler(model, sampler_name or ("plms" if plms else "ddim"))
    grid = {} if discretize is None else {"ddim_discretize": discretize}
    with model.ema_scope():
        wholemask = instance["wholemask"].permute(0, 4, 1, 2, 3).cuda()
        nz = torch.where(wholemask.sum((0, 1, 3, 4)))[0]
        start_layer, end_layer = nz[0], nz[-1]
        shape = (model.channels, model.image_size, model.image_size) if not model.no_first_stage else (1,) + tuple(wholemask.shape[-2:])
        assert wholemask.shape[0] == 1, "batch size should be 1"
        samples = torch.zeros((n_samples,) + wholemask.shape[1:], dtype=torch.float32, device=wholemask.device)
        gen_mask = wholemask.repeat(n_samples, 1, 1, 1, 1)
        g = torch.Generator(device=wholemask.device).manual_seed(noise_seed) if noise_seed is not None else None
        layers = range(start_layer.item() - 1, end_layer.item() + 1)
        for it, m_ in enumerate(layers):
            concat_cond = torch.cat([samples[:, :, max(0, m_ - 1)], gen_mask[:, :, m_]], axis=1)
            c = model.get_learned_conditioning(concat_cond)
            if x_T_tape is not None:
                x_T = x_T_tape[it].to(wholemask.device).float()
            else:
                x_T = torch.randn((n_samples,) + shape, generator=g, device=wholemask.device) if g is not None else None
            if vanilla and progress is not None and it == len(layers) - 1:
                s, progress["intermediates"] = model.progressive_denoising(c, (n_samples,) + shape, x_T=x_T, verbose=False,
                                                                           log_every_t=progress.get("log_every_t"))
            elif vanilla:
                s = model.p_sample_loop(c, (n_samples,) + shape, x_T=x_T, verbose=False)
            else:
                s, _ = sampler.sample(S=ddim_steps, dims=len(shape) - 1, conditioning=c, batch_size=n_samples, shape=shape,
                                      verbose=False, eta=ddim_eta, x_T=x_T, **grid)
            ds = model.decode_first_stage(s)
            samples[:, :, m_] = (ds - ds.min()) / (ds.max() - ds.min())
        if record is not None and not vanilla:
            record.update(sampler=sampler_name or ("plms" if plms else "ddim"),
                          discretize=discretize or ("logsnr" if sampler_name == "dpmpp_2m" else "uniform"), steps_asked=int(ddim_steps),
                          steps=int(sampler.ddim_timesteps.shape[0]) if hasattr(sampler, "ddim_timesteps") else None)
        return torch.cat([samples, gen_mask], dim=1)


def check_edit_options(opt) -> bool:
    """The CT editing flags, checked by name before a model is loaded.  True when the run edits."""
    if opt.known_ct is None:
        if opt.known_mask is not None or opt.keep_mask is not None or opt.edit_margin != 0:
            raise SystemExit("--known-mask / --keep-mask / --edit-margin edit a known CT: give --known-ct DIR")
        return False
    if not opt.inputs:
        raise SystemExit("--known-ct pairs known CT volumes with the label volumes of --inputs DIR")
    if (opt.known_mask is None) == (opt.keep_mask is None):
        raise SystemExit("--known-ct needs exactly one of --known-mask DIR and --keep-mask DIR")
    for name in ("known_ct", "known_mask", "keep_mask"):
        d = getattr(opt, name)
        if d is not None and not os.path.isdir(d):
            raise SystemExit(f"--{name.replace('_', '-')} {d!r} is not a directory")
    if opt.edit_margin < 0:
        raise SystemExit(f"--edit-margin {opt.edit_margin}: must be >= 0")
    if opt.vanilla_sample:
        raise SystemExit("--known-ct: -v / --vanilla_sample is not supported (CT editing runs the DDIM sampler at eta 0)")
    if opt.plms:
        raise SystemExit("--known-ct: --plms is not supported (CT editing runs the DDIM sampler at eta 0)")
    if opt.eta > 0:
        raise SystemExit(f"--known-ct: eta = {opt.eta} is not supported (CT editing runs the DDIM sampler at eta 0)")
    if opt.n_samples > 1:
        raise SystemExit(f"--known-ct: n_samples = {opt.n_samples} is not supported (one edited CT per known volume)")
    return True


def _paired_volume(directory: str, stem: str, flag: str) -> np.ndarray:
    found = [f for f in (os.path.join(directory, stem + ext) for ext in (".nii.gz", ".nii")) if os.path.exists(f)]
    if not found:
        raise SystemExit(f"{flag} {directory!r}: no volume named {stem}.nii.gz / {stem}.nii (volumes pair with --inputs by stem)")
    return np.ascontiguousarray(read_nifti(found[0]))


@torch.no_grad()
def edit_volume(pipe, opt, stem: str, labels: np.ndarray, seed: int):
    """One edited volume of --known-ct: (ct fp32 [slices, size, size] on the device, its entry of metrics.json's edit block)."""
    shape = (opt.slices, opt.size, opt.size)
    known = _paired_volume(opt.known_ct, stem, "--known-ct")
    if tuple(known.shape) != shape:
        raise SystemExit(f"--known-ct: {stem} has shape {tuple(known.shape)}, --slices x --size x --size is {shape} (nothing is resampled)")
    known = torch.from_numpy(known.astype(np.float32))
    if not (float(known.min()) >= 0.0 and float(known.max()) <= 1.0):
        raise SystemExit(f"--known-ct: {stem} holds values {float(known.min()):g}..{float(known.max()):g} outside [0, 1]")
    lab = torch.as_tensor(np.ascontiguousarray(labels)).to(device="cuda", dtype=torch.int32)[None].contiguous()
    if opt.keep_mask is not None:
        keep = _paired_volume(opt.keep_mask, stem, "--keep-mask")
        if tuple(keep.shape) != shape:
            raise SystemExit(f"--keep-mask: {stem} has shape {tuple(keep.shape)}, --slices x --size x --size is {shape}")
        keep = (torch.from_numpy(keep) != 0).to(device="cuda", dtype=torch.uint8)[None]
    else:
        old = _paired_volume(opt.known_mask, stem, "--known-mask")
        if tuple(old.shape) != tuple(lab.shape[1:]):
            raise SystemExit(f"--known-mask: {stem} has shape {tuple(old.shape)}, the edited label volume {tuple(lab.shape[1:])}")
        keep = pipe.ct_keep_from_labels(torch.as_tensor(old).to(device="cuda", dtype=torch.int32)[None].contiguous(), lab, opt.slices, opt.size)
    known = known.cuda()[None]
    ct = pipe.sample_ct_volumes(lab, opt.slices, opt.size, [seed], known_ct=known, keep=keep, edit_margin=opt.edit_margin)[0]
    kb = keep[0] != 0
    diff = float((ct[kb] - known[0][kb]).abs().max()) if bool(kb.any()) else 0.0
    doc = dict(volume=stem, kept_fraction=float(kb.float().mean()), slices_visited=int(pipe.stats["slices_visited"]),
               slices_skipped_kept=int(pipe.stats["slices_skipped_kept"]), slices_mixed=int(pipe.stats["slices_mixed"]),
               unkept_outside_window=int(pipe.stats["unkept_outside_window"]), kept_max_abs_diff=diff)
    return ct, doc


def cleanup_from_options(opt):
    """The postprocess.clean options of --largest-component / --min-component / --connectivity, or None; refusals before any sampling.
    Stage-1 masks carry their class count in their labels: the options are checked against the 32 classes the kernels take."""
    from . import postprocess
    try:
        opts = postprocess.cleanup_options(opt, 32)
    except ValueError as e:
        raise SystemExit(str(e)) from None
    if opts is not None and not opt.inputs:
        raise SystemExit("--largest-component / --min-component clean the stage-1 masks of --inputs DIR")
    return opts


def clean_stage1_mask(labels: np.ndarray, opts: dict, stem: str):
    """One stage-1 label volume through postprocess.clean on the device: (cleaned labels, numpy, dtype kept; its entry of metrics.json's
    mask_cleanup block)."""
    from . import postprocess
    if labels.ndim != 3 or labels.dtype.kind not in "iu" or labels.min() < 0 or labels.max() > 31:
        raise SystemExit(f"--inputs volume {stem}: cleaning needs an integer [D, H, W] label volume with labels 0..31, got {labels.dtype} "
                         f"{labels.shape}")
    K = max(2, int(labels.max()) + 1)
    largest = opts["largest"] if opts["largest"] in (None, "all") else [c for c in opts["largest"] if c < K]
    dev_labels = torch.from_numpy(labels.astype(np.int32)).cuda()
    cleaned, kept, before, after = postprocess.clean(dev_labels, K, largest=largest, min_size=opts["min_size"], connectivity=opts["connectivity"])
    doc = dict(volume=stem, num_classes=K, removed_voxels=int((kept == 0).sum()), before=before, after=after)
    return cleaned.cpu().numpy().astype(labels.dtype), doc


def render_input(x: torch.Tensor) -> torch.Tensor:
    """One sampled volume [2, D, H, W] = (CT, label / 255) as render.combine_mask_and_im takes it: (CT, label / 11).  The reference
    renders `pred` as it is (sample_diffusion.py:257); label / 255 * 11 truncates to 0 for every label, so nothing would be painted."""
    return torch.cat([x[:1].float(), torch.round(x[1:2].float() * 255) / 11])


def main(argv=None):
    opt, unknown = get_parser().parse_known_args(argv)
    scoring = (opt.gt, opt.lpips_vgg, opt.lpips_lin)
    if any(scoring) and not all(scoring):
        raise SystemExit("--gt, --lpips-vgg and --lpips-lin go together")
    if opt.progress_png and not opt.vanilla_sample:
        raise SystemExit("--progress-png goes with -v / --vanilla_sample (the denoise row comes from progressive_denoising)")
    if opt.log_every_t is not None and not opt.progress_png:
        raise SystemExit("--log-every-t goes with --progress-png")
    sampler_name, discretize = sampler_from_options(opt)
    editing = check_edit_options(opt)
    if editing and (sampler_name != "ddim" or discretize is not None):
        raise SystemExit(f"--known-ct: --sampler {sampler_name} / --discretize is not supported (CT editing runs the DDIM sampler at eta 0 on its "
                         "uniform grid)")
    cleanup = cleanup_from_options(opt)
    cleanup_docs = []
    scorer = None
    if all(scoring):                         # weights and directory are checked before anything is sampled
        from .lpips import LPIPS
        if not os.path.isdir(opt.gt):
            raise SystemExit(f"--gt {opt.gt!r} is not a directory")
        scorer = LPIPS.load(opt.lpips_vgg, opt.lpips_lin)
    ckpt, logdir = None, opt.logdir
    if opt.resume:
        if os.path.isfile(opt.resume):
            logdir = "/".join(opt.resume.split("/")[:-2]) or "."
            ckpt = opt.resume
        else:
            logdir = opt.resume.rstrip("/")
            ckpt = os.path.join(logdir, "checkpoints", "last.ckpt")
    cfgs = sorted(glob.glob(os.path.join(logdir, "configs", "*.yaml"))) if logdir != "none" else []
    if opt.config:
        cfgs.append(opt.config)
    if not cfgs:
        raise SystemExit("no model config: give -r <logdir with configs/*.yaml> or --config <yaml>")
    config = {}
    for c in cfgs:
        config = merge(config, load_yaml(c))
    config = strip_ckpt_paths(apply_dotlist(config, unknown))
    model, global_step = load_model(config, ckpt)
    print(f"global step: {global_step}", file=sys.stderr)
    out_dir = os.path.join(logdir if logdir != "none" else ".", "samples", f"{global_step:08}")
    os.makedirs(out_dir, exist_ok=True)
    if opt.inputs:
        # stage-1 hand-off (README.md:21): one CT volume per label volume found in the directory, in name order; the start latents of
        # volume i come from the generator seeded with --seed + i
        files = sorted(f for f in glob.glob(os.path.join(opt.inputs, "*.nii*")) if f.endswith((".nii", ".nii.gz")))
        if not files:
            raise SystemExit(f"--inputs {opt.inputs!r}: no *.nii / *.nii.gz label volumes found")
        stage1 = {os.path.basename(f).split(".nii")[0]: read_nifti(f) for f in files}
        if cleanup is not None:                  # the slice loop (and an edit) is conditioned on the cleaned masks
            for stem in list(stage1):
                stage1[stem], cdoc = clean_stage1_mask(stage1[stem], cleanup, stem)
                cleanup_docs.append(cdoc)
        label_volumes = stage1 if editing else None
        jobs = [(os.path.basename(f).split(".nii")[0], stage1_mask_to_wholemask(stage1[os.path.basename(f).split(".nii")[0]], opt.slices, opt.size),
                 opt.seed + i) for i, f in enumerate(files)]
    else:
        lab = torch.from_numpy(np.load(opt.mask)).long() if opt.mask else synth_mask_volume(opt.slices, opt.size, opt.size)
        jobs = [("sample", lab.float() / 255.0, opt.seed)]
    written = []
    edit_docs = []
    sampler_doc = {}
    if editing:
        if getattr(model, "no_first_stage", False):
            raise SystemExit("--known-ct: a model without a first stage is not supported (the known slice is encoded by the first stage)")
        from .pipeline import GuideGenPipeline
        pipe = GuideGenPipeline(None, model, opt.custom_steps)
    for stem, wholemask, seed in jobs:
        instance = {"wholemask": wholemask[None, ..., None]}
        t0 = time.time()
        if editing:
            with model.ema_scope():
                ct, doc = edit_volume(pipe, opt, stem, label_volumes[stem], seed)
            torch.cuda.synchronize()
            edit_docs.append(doc)
            write_nifti(os.path.join(out_dir, f"{stem}_0000.nii.gz"), ct.float().cpu().numpy())
            written.append(os.path.join(out_dir, f"{stem}_0000.nii.gz"))
            if opt.png:
                volume_png(render_input(torch.stack([ct, wholemask.to(ct.device)])), os.path.join(out_dir, f"{stem}_0000.png"))
            print(f"edited {tuple(ct.shape)} in {time.time() - t0:.1f}s ({doc['slices_visited']} slices visited, {doc['slices_skipped_kept']} kept "
                  f"whole) -> {out_dir}/{stem}_0000.nii.gz", file=sys.stderr)
            continue
        progress = dict(log_every_t=opt.log_every_t) if opt.progress_png else None
        pred = sample_cond(model, instance, n_samples=opt.n_samples, ddim_steps=opt.custom_steps, ddim_eta=opt.eta, noise_seed=seed,
                           vanilla=opt.vanilla_sample, plms=opt.plms, progress=progress, sampler_name=sampler_name, discretize=discretize,
                           record=sampler_doc)
        torch.cuda.synchronize()
        if progress is not None:
            write_png(os.path.join(out_dir, f"{stem}_progress.png"), model.denoise_row(progress["intermediates"], value_range=(-1.0, 1.0)).cpu().numpy())
        for ix, x in enumerate(pred):
            write_nifti(os.path.join(out_dir, f"{stem}_{ix:04d}.nii.gz"), x[0].float().cpu().numpy())
            written.append(os.path.join(out_dir, f"{stem}_{ix:04d}.nii.gz"))
            if opt.png:
                volume_png(render_input(x), os.path.join(out_dir, f"{stem}_{ix:04d}.png"))
        print(f"sampled {tuple(pred.shape)} in {time.time() - t0:.1f}s -> {out_dir}/{stem}_*.nii.gz", file=sys.stderr)
        if sampler_doc:
            print(f"sampler {sampler_doc['sampler']} on the {sampler_doc['discretize']} grid: {sampler_doc['steps']} steps per slice "
                  f"({sampler_doc['steps_asked']} asked)", file=sys.stderr)
    chosen = opt.sampler is not None or opt.discretize is not None          # an explicit choice is recorded even when nothing is scored
    if scorer is not None or editing or cleanup is not None or (chosen and sampler_doc):
        import json
        doc = {}
        if scorer is not None:
            from .lpips import score_directory
            doc = score_directory(scorer.cuda(), written, opt.gt, torch.device("cuda"))
        if sampler_doc:
            doc["sampler"] = dict(sampler_doc)
        if editing:
            doc["edit"] = dict(edit_margin=opt.edit_margin, known_mask=opt.known_mask, keep_mask=opt.keep_mask, volumes=edit_docs)
        if cleanup is not None:
            doc["mask_cleanup"] = dict(largest=cleanup["largest"], min_size=cleanup["min_size"], connectivity=cleanup["connectivity"],
                                       volumes=cleanup_docs)
        with open(os.path.join(out_dir, "metrics.json"), "w") as f:
            json.dump(doc, f, indent=1)
    if scorer is not None:
        print(f"mean LPIPS {doc['mean_lpips']:.5f} over {len(written)} volume(s) -> {out_dir}/metrics.json", file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1:])

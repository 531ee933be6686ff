"""GuideGen volume pipeline on one GPU: CCDM mask (labels) -> stage glue -> autoregressive LDM slices -> CT volume.

Restates the orchestration of ccdm/ddpm/evaluator.py:127-170 (x_T ~ uniform categorical, condition = zeros) and
latentdiffusion/sample_diffusion.py:196-224 (slice loop: cond = [previous generated slice, mask slice] -> cond stage
-> DDIM -> decode -> min-max normalise -> feed back), keeping every tensor on the device in channels-last form.
Volumes are independent units: multi-GPU runs shard volumes over ranks with no collective.

CLI (one process per GPU, under torch.distributed.run or alone):
    python -m jointimagegeneration_amd.pipeline --volumes V --out DIR [--mask-size D H W] [--depth 256] [--hw 512] [--ccdm-steps 250] [--ddim-steps 50]
                                                [--volumes-per-gpu B] [--sampler ddim|dpmpp_2m] [--discretize uniform|quad|logsnr]
samples volumes `volume_id mod world_size == rank` and writes `mask_<id>.nii.gz` (uint8 labels) and `ct_<id>.nii.gz` (fp32 in [0, 1])
per volume; volume id v uses seed `--seed + 1000 v` for the mask chain and `+ 1` for the slice loop, whatever the world size.
With B > 1 a rank samples its volumes in groups of B independent volumes per batch (GuideGenPipeline.run_volumes; the last group may
be smaller): same seeds and file names per volume id as at B = 1.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .ccdm import DenoisingModel, DiffusionModel, uniform_x_T
from .ldm import DDIMSampler, LatentDiffusion
from .ops import CL
from .synth import randomize_parameters
from .unet import create_unet_openai

CCDM_PARAMS = dict(base_channels=64, channel_mult=[1, 2, 2, 4, 5], attention_resolutions=[32, 16, 8], num_heads=1,
                   num_head_channels=32, softmax_output=True)                      # ccdm/params_eval.yml:58-64


def ae_config(in_channels: int, ch: int) -> dict:
    """first/cond stage of configs/latent-diffusion/ruijin-ldm_from_controlnet_ae.yaml:41-94."""
    return dict(target="ldm.models.autoencoder.AutoencoderKL",
                params=dict(embed_dim=4, dims=2, lossconfig=dict(target="torch.nn.Identity"),
                            ddconfig=dict(double_z=True, z_channels=4, resolution=512, in_channels=in_channels, out_ch=in_channels,
                                          ch=ch, ch_mult=[1, 2, 4, 4], num_res_blocks=2, dropout=0.0, dims=2, attn_resolutions=[16, 8])))


LDM_UNET = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel",
                params=dict(dims=2, image_size=512, in_channels=8, out_channels=4, model_channels=160, attention_resolutions=[8, 4, 2],
                            num_res_blocks=2, channel_mult=[1, 2, 4, 4, 5], num_head_channels=32))   # …_ae.yaml:17-40


def build_ccdm(K: int = 14, T: int = 250, seed: int = 1024, device="cuda") -> DenoisingModel:
    unet = create_unet_openai(image_size=128, in_channels=K + 1, out_channels=K, num_res_blocks=2, cond_encoded_shape=None, dims=3,
                              **CCDM_PARAMS)
    randomize_parameters(unet, seed, "ccdm.")
    return DenoisingModel(DiffusionModel("cosine", T, K, dims=3), unet, "synthetic", "majority", dims=3).eval().to(device)


def build_ldm(seed: int = 1024, device="cuda", use_ema: bool = False) -> LatentDiffusion:
    m = LatentDiffusion(first_stage_config=ae_config(1, 128), cond_stage_config=ae_config(2, 96), unet_config=LDM_UNET,
                        linear_start=0.0015, linear_end=0.0195, num_timesteps_cond=1, timesteps=1000, first_stage_key="image",
                        cond_stage_key="mask", image_size=64, channels=4, dims=2, use_ema=use_ema)
    randomize_parameters(m, seed, "ldm.")
    return m.eval().to(device)


def slice_window(labels: torch.Tensor, depth: int, max_slices: Optional[int] = None) -> List[int]:
    """The slice loop of labels [Dm, Hm, Wm] or [N, Dm, Hm, Wm], as GuideGenPipeline.sample_ct visits it: slices whose order-0 upsampled
    mask is non-empty in ANY batch element (sample_diffusion.py:202; the reference's batch is N copies of one mask), from one before the
    first (python indexing: -1 is the last slice) to the last; an empty mask visits slice 0 only.  Independent volumes pass one volume
    at a time.  Returns the loop values m (slice m % depth, previous slice max(0, m - 1) % depth)."""
    lab = labels.reshape((-1,) + tuple(labels.shape[-3:]))
    Dm = lab.shape[1]
    nz = (lab != 0).flatten(2).any(-1).any(0).cpu()                                   # [Dm]
    idx = torch.nonzero(nz[ops.zoom0_index(Dm, depth)]).flatten()                   # same order-0 rule as the glue kernel
    start, end = (int(idx[0]), int(idx[-1])) if idx.numel() else (1, 0)
    todo = list(range(start - 1, end + 1))
    return todo[:max_slices] if max_slices is not None else todo


def volume_schedule(windows: Sequence[Sequence[int]], depth: int) -> Tuple[torch.Tensor, float]:
    """Static-batch schedule of independent volumes: int32 [iterations, B, 3] of (slice, previous slice, active), iterations = the longest
    window; volume i is active in its first len(windows[i]) iterations (finished volumes keep computing on row (0, 0, 0), their output is
    discarded).  Also returns the fraction of batch slots that do discarded work, 1 - sum(len_i) / (B * iterations)."""
    B = len(windows)
    iters = max(len(w) for w in windows)
    sched = torch.zeros((iters, B, 3), dtype=torch.int32)
    for i, w in enumerate(windows):
        for it, m in enumerate(w):
            sched[it, i, 0], sched[it, i, 1], sched[it, i, 2] = m % depth, max(0, m - 1) % depth, 1
    wasted = 1.0 - sum(len(w) for w in windows) / float(B * iters)
    return sched, wasted


def plan_ct_edit(labels: torch.Tensor, depth: int, max_slices: Optional[int], known_d: torch.Tensor, keep_d: torch.Tensor,
                 q_shape: Tuple[int, ...], x_T_tapes=None, q_noise_tapes=None):
    """What CT editing adds to the loop of independent volumes, on the host: known_d fp32 and keep_d bool are slice-major
    [depth, B, hw, hw], q_shape is the q-sample noise of one mixed slice, (S, 1, Cz, lat, lat).  Per volume: the slices of its window it
    visits (one all of whose pixels are kept is skipped) and which of them are mixed (some pixel kept); the four counters of
    self.stats; the refusals of tapes whose lengths or shapes do not fit the visits; the start volume (known where kept, else 0), which
    is the result when no volume visits anything.  Returns (windows, mixed, counters, start)."""
    B = labels.shape[0]
    kept_all = keep_d.flatten(2).all(-1).cpu()                                         # [depth, B]
    kept_any = keep_d.flatten(2).any(-1).cpu()
    unkept_px = (~keep_d).flatten(2).sum(-1).cpu()
    windows, mixed, skipped, outside = [], [], 0, 0
    for i in range(B):
        win = slice_window(labels[i], depth, max_slices)
        visit = [m for m in win if not bool(kept_all[m % depth, i])]
        skipped += len(win) - len(visit)
        inside = {m % depth for m in win}
        outside += int(sum(int(unkept_px[d, i]) for d in range(depth) if d not in inside))
        windows.append(visit)
        mixed.append([bool(kept_any[m % depth, i]) for m in visit])
    n_mixed = [sum(mx) for mx in mixed]
    for name, tapes, want in (("x_T_tapes", x_T_tapes, [len(w) for w in windows]), ("q_noise_tapes", q_noise_tapes, n_mixed)):
        if tapes is not None:
            for i in range(B):
                if len(tapes[i]) != want[i]:
                    raise ValueError(f"sample_ct_volumes: {name}[{i}] holds {len(tapes[i])} tensors, volume {i} "
                                     f"{'visits' if name == 'x_T_tapes' else 'has'} {want[i]} {'slices' if name == 'x_T_tapes' else 'mixed slices'}")
    if q_noise_tapes is not None:
        for i in range(B):
            for k, t in enumerate(q_noise_tapes[i]):
                if tuple(t.shape) != tuple(q_shape):
                    raise ValueError(f"sample_ct_volumes: q_noise_tapes[{i}][{k}] has shape {tuple(t.shape)}, a mixed slice takes {tuple(q_shape)}")
    counters = dict(slices_visited=sum(len(w) for w in windows), slices_skipped_kept=skipped, slices_mixed=sum(n_mixed),
                    unkept_outside_window=outside)
    return windows, mixed, counters, torch.where(keep_d, known_d, torch.zeros_like(known_d))


def _tape_or_randn(tape, k: int, shape: Tuple[int, ...], gen: torch.Generator) -> torch.Tensor:
    """Entry k of a parity tape, or the seeded draw of `shape` from `gen` on its device, in the reference's NCHW element order
    (ddim.py:124 `torch.randn(shape)`), so that a seeded generator gives sample_diffusion.sample_cond and these loops the same noise."""
    return tape[k].to(gen.device).float() if tape is not None else torch.randn(shape, generator=gen, device=gen.device)


def _load_x_T(st: Dict, x_T: torch.Tensor) -> None:
    """NCHW x_T [B, Cz, lat, lat] -> the chain state's fp32 x and the bf16 UNet input, both channels-last (plumbing copies)."""
    Cz = x_T.shape[1]
    x_T = x_T.permute(0, 2, 3, 1).reshape(st["x"].shape)
    st["x"].copy_(x_T)
    st["unet_in"][..., :Cz].copy_(x_T)


def _log(msg: str) -> None:
    print(f"[guidegen {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


SAMPLERS = ("ddim", "dpmpp_2m")                       # GuideGenPipeline(sampler=); the command lines add "plms" where they take it
DISCRETIZATIONS = {"ddim": ("uniform", "quad"), "plms": ("uniform", "quad"), "dpmpp_2m": ("uniform", "quad", "logsnr")}


def check_sampler_options(sampler: str, discretize: Optional[str], samplers: Sequence[str] = SAMPLERS) -> None:
    """Host-side refusal, by name, of a sampler / grid pair that does not exist."""
    if sampler not in samplers:
        raise ValueError(f"sampler = {sampler!r} is not one of {', '.join(samplers)}")
    if discretize is not None and discretize not in DISCRETIZATIONS[sampler]:
        raise ValueError(f"discretize = {discretize!r} is not a grid of the {sampler} sampler ({', '.join(DISCRETIZATIONS[sampler])})")


class GuideGenPipeline:
    progress_every_s = 30.0

    @property
    def steps(self) -> int:
        """The chain's own step count: the grid's, which may differ from the ddim_steps asked for."""
        return int(self.sampler.ddim_timesteps.shape[0])

    def __init__(self, ccdm: DenoisingModel, ldm: LatentDiffusion, ddim_steps: int = 50, sampler: str = "ddim", discretize: Optional[str] = None):
        """sampler: "ddim" (the default: DDIM at eta 0 on its uniform grid, or on `discretize` "quad") or "dpmpp_2m" (DPM-Solver++ 2M,
        dpm_solver.py, on its log-SNR grid unless `discretize` names "uniform" / "quad"); ddim_steps is the step count asked of the grid."""
        self.ccdm, self.ldm, self.ddim_steps = ccdm, ldm, ddim_steps
        check_sampler_options(sampler, discretize)
        self.sampler_name = sampler
        if sampler == "dpmpp_2m":
            from .dpm_solver import DPMSolverSampler
            self.discretize = discretize or "logsnr"
            self.sampler = DPMSolverSampler(ldm)
            self.sampler.make_schedule(ddim_steps, ddim_discretize=self.discretize, ddim_eta=0.0, verbose=False)
        else:
            self.discretize = discretize or "uniform"
            self.sampler = DDIMSampler(ldm)
            self.sampler.make_schedule(ddim_steps, ddim_discretize=self.discretize, ddim_eta=0.0, verbose=False)
        self.stats: Dict[str, float] = {}
        self.use_graph = True
        self._slice_graphs: Dict = {}
        self._volume_graphs: Dict = {}
        # spatial reduction of the first stage: f = 2^(levels-1) (8 for ch_mult [1,2,4,4], ..._ae.yaml:41-67)
        self.latent_factor = 2 ** (ldm.first_stage_model.decoder.num_resolutions - 1)

    # ---- stage 1 ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample_mask(self, N: int, size: Tuple[int, int, int], seed: int, init_t: Optional[int] = None, known: Optional[torch.Tensor] = None,
                    keep: Optional[torch.Tensor] = None, resample: int = 1) -> torch.Tensor:
        """x_T ~ uniform categorical one-hot (evaluator.py:135-136), condition = zeros; returns int32 labels [N,D,H,W].
        known / keep / resample: mask editing, as `DenoisingModel.sample_labels` takes them ([N, D, H, W])."""
        dev = self.ccdm.diffusion.betas.device
        K = self.ccdm.diffusion.num_classes
        g = torch.Generator(device=dev).manual_seed(seed)
        x_T = torch.randint(0, K, (N,) + tuple(size), generator=g, device=dev, dtype=torch.int32)
        self.ccdm.philox_seed = seed
        cond = torch.zeros((N, 1) + tuple(size), device=dev)
        labels, _ = self.ccdm.sample_labels(x_T, cond, init_t, known=known, keep=keep, resample=resample)
        return labels

    @torch.no_grad()
    def sample_masks(self, seeds: Sequence[int], size: Tuple[int, int, int], init_t: Optional[int] = None,
                     known: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None, resample: int = 1) -> torch.Tensor:
        """Independent volumes in one batch: volume i is sample_mask(1, size, seeds[i]) -- its own x_T generator and its own Philox key
        (per-sample key of the reverse step), so that it depends on nothing its neighbours hold.  Returns int32 labels [B, D, H, W].
        known / keep / resample: mask editing, as `DenoisingModel.sample_labels` takes them ([B, D, H, W])."""
        dev = self.ccdm.diffusion.betas.device
        x_T = uniform_x_T(self.ccdm.diffusion.num_classes, size, seeds, dev)
        cond = torch.zeros((len(seeds), 1) + tuple(size), device=dev)
        labels, _ = self.ccdm.sample_labels(x_T, cond, init_t, philox_seeds=[int(s) for s in seeds], known=known, keep=keep, resample=resample)
        return labels

    def _engine(self, cache: Dict, key, N: int, hw: int, dev, st, finish) -> Dict:
        """What the two slice engines share, cached in `cache` under `key` until the chain state or a network's weights change: the static
        buffers (cond-stage input, first-stage latent, decoded slices), the ladder's "warmed" flag, and the heads of the two per-slice
        networks -- cond-stage encode into the chain's c_concat channels (returns the moments), and z = x / scale_factor through the
        first-stage decode into "ds".  finish(engine, encode_head, decode_head) adds a new engine's own buffers and graph slots and sets
        its "encode" and "decode"."""
        ldm = self.ldm
        lat, Cz = hw // self.latent_factor, ldm.channels
        # decode_head divides by scale_factor: a Python float is folded into the captured launch, the scale_by_std buffer is read by it
        # in place -- so the float's value, or the buffer's identity (address and version), joins the token
        sf = ldm.scale_factor
        sf = (sf.data_ptr(), sf._version) if isinstance(sf, torch.Tensor) else float(sf)
        token = (id(st), ops.weights_token(ldm.cond_stage_model), ops.weights_token(ldm.first_stage_model), sf)
        eng = cache.get(key)
        if eng is not None and eng["token"] == token:
            return eng
        eng = dict(token=token, cond_in=torch.empty((N, 1, hw, hw, 32), dtype=torch.bfloat16, device=dev),
                   z=torch.zeros((N, 1, lat, lat, 32), dtype=torch.bfloat16, device=dev),
                   ds=torch.empty((N, hw, hw), dtype=torch.float32, device=dev), warmed=False)

        def encode_head():
            mom = ldm.cond_stage_model.encode_moments_cl(CL(eng["cond_in"], 2))         # fp32 CL [N,1,lat,lat,32]; mode() = mean
            st["unet_in"][..., Cz:2 * Cz].copy_(mom.t[..., :Cz])                       # c_concat = posterior mean (plumbing copy)
            return mom

        def decode_head():
            eng["z"][..., :Cz].copy_(st["x"] * (1.0 / ldm.scale_factor))
            dec = ldm.first_stage_model.decode_cl(CL(eng["z"], Cz))                     # fp32 CL [N,1,hw,hw,32]
            eng["ds"].copy_(dec.t[..., 0].reshape(N, hw, hw))

        finish(eng, encode_head, decode_head)
        cache[key] = eng
        return eng

    def _slice_engine(self, N: int, hw: int, dev, st) -> Dict:
        """Static buffers + hipGraphs of the two per-slice networks (cond-stage encode, first-stage decode) for one shape; the decoded
        batch is normalised as a whole, in place."""
        def finish(sg, encode_head, decode_head):
            sg.update(enc=None, dec=None, slice=None, mom=None)

            def encode():
                sg["mom"] = encode_head()

            def decode():
                decode_head()
                ops.minmax_normalise(sg["ds"], out=sg["ds"])

            sg["encode"], sg["decode"] = encode, decode

        return self._engine(self._slice_graphs, (N, hw, str(dev)), N, hw, dev, st, finish)

    @torch.no_grad()
    def time_slice_stages(self, N: int = 1, hw: int = 512) -> Dict[str, float]:
        """HIP-event times (ms) of the three per-slice stages on the engine's own buffers, as the slice loop runs them
        (captured graphs when enabled): cond-encode, one sampler step (average over the steps of a slice: DDIM divides by the
        ddim_steps asked for, as it always has; any other sampler by its chain's own count, `steps`), decode."""
        dev = self.ldm.device
        lat, Cz = hw // self.latent_factor, self.ldm.channels
        st = self.sampler.prepare_state(N, Cz, (lat, lat), dev, Cz)
        sg = self._slice_engine(N, hw, dev, st)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

        sg["cond_in"].zero_()
        st["x"].normal_()
        st["unet_in"][..., :Cz].copy_(st["x"])
        if self.use_graph:                                    # per-stage graphs for the timing only (the slice loop replays ONE graph)
            if not sg["warmed"]:
                sg["encode"](); sg["decode"]()
            if sg["enc"] is None:
                sg["enc"], sg["dec"] = ops.capture_graph(sg["encode"]), ops.capture_graph(sg["decode"])

        def run(g, fn):
            g.replay() if (self.use_graph and g is not None) else fn()

        for rep in range(3):                                  # eager warm-up, chain-graph capture + first replay, timed
            ev[0].record()
            run(sg["enc"], sg["encode"])
            ev[1].record()
            self.sampler.run_steps(st, None, 0.0, None)
            ev[2].record()
            run(sg["dec"], sg["decode"])
            ev[3].record()
        torch.cuda.synchronize()
        return {"encode_ms": ev[0].elapsed_time(ev[1]), "ddim_step_ms": ev[1].elapsed_time(ev[2]) / (self.ddim_steps if self.sampler_name == "ddim" else st["S"]),
                "decode_ms": ev[2].elapsed_time(ev[3])}

    # ---- stage 2 ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample_ct(self, labels: torch.Tensor, depth: int, hw: int, seed: int, max_slices: Optional[int] = None,
                  x_T_tape=None) -> torch.Tensor:
        """labels int32 [N,Dm,Hm,Wm] -> CT volume fp32 [N, depth, hw, hw] in [0,1]; slice m conditioned on slice m-1.
        `x_T_tape` (parity runs): one [N, Cz, lat, lat] start latent per generated slice, in loop order, instead of the seeded draw."""
        ldm, sampler = self.ldm, self.sampler
        dev = labels.device
        N = labels.shape[0]
        lat = hw // self.latent_factor
        Cz = ldm.channels
        g = torch.Generator(device=dev).manual_seed(seed)
        samples = torch.zeros((depth, N, hw, hw), dtype=torch.float32, device=dev)        # slice-major: one slice is contiguous
        todo = slice_window(labels, depth, max_slices)                                     # one window for the whole batch
        st = sampler.prepare_state(N, Cz, (lat, lat), dev, Cz)
        sg = self._slice_engine(N, hw, dev, st)
        cond_in, encode, decode = sg["cond_in"], sg["encode"], sg["decode"]

        t_last = time.time()
        for it, m in enumerate(todo):
            if time.time() - t_last > self.progress_every_s:
                _log(f"LDM slice {it}/{len(todo)}")
                t_last = time.time()
            mm = m % depth
            prev = samples[max(0, m - 1) % depth]
            ops.mask_to_cond_slice(labels, mm, depth, hw, hw, prev, cond_in)
            _load_x_T(st, _tape_or_randn(x_T_tape, it, (N, Cz, lat, lat), g))
            if not (self.use_graph and sampler.chain_graphable(st)):
                encode()
                sampler.run_steps(st, None, 0.0, None)
                decode()
            else:
                # ONE hipGraph per slice: cond-encode, the S DDIM steps (each reading its own rows of the bias / scalar tables) and the
                # decode; the host's share of a slice is the glue kernel, the x_T draw and this replay
                ops.replay_captured(sg, "slice", lambda: (encode(), sampler.chain(st), decode()))
            samples[mm].copy_(sg["ds"])
        return samples.permute(1, 0, 2, 3)

    def _volume_engine(self, B: int, hw: int, depth: int, lab_shape: Tuple[int, ...], dev, st, edit_margin: Optional[int] = None) -> Dict:
        """Static buffers + the ONE per-slice hipGraph of the batched slice loop of B independent volumes: batched glue (schedule row of the
        device iteration counter), cond-encode, the S DDIM steps, decode, per-volume normalise + scatter (advances the counter).
        edit_margin (an int): the engine of the editing loop, under its own key -- `st` is then an inpainting state; the
        known / keep volumes, the first-stage input and the edit glue + first-stage encode join the iteration, and the scatter composites."""
        ldm = self.ldm
        Cz = ldm.channels
        edit = edit_margin is not None
        key = (B, hw, depth, tuple(lab_shape), str(dev)) + ((("edit", int(edit_margin)),) if edit else ())

        def finish(ve, encode_head, decode_head):
            ve.update(labels=torch.zeros(tuple(lab_shape), dtype=torch.int32, device=dev),
                      samples=torch.zeros((depth, B, hw, hw), dtype=torch.float32, device=dev),
                      sched=torch.zeros((depth + 1, B, 3), dtype=torch.int32, device=dev),  # a window has at most depth + 1 iterations
                      it=torch.zeros(1, dtype=torch.int32, device=dev), ws=torch.empty(2 * B, dtype=torch.float32, device=dev), graph=None)
            if edit:
                ve.update(known=torch.zeros((depth, B, hw, hw), dtype=torch.float32, device=dev),
                          keep=torch.zeros((depth, B, hw, hw), dtype=torch.uint8, device=dev),
                          fs_in=torch.empty((B, 1, hw, hw, 32), dtype=torch.bfloat16, device=dev))

            def glue():
                ops.mask_to_cond_slices(ve["labels"], depth, hw, hw, ve["sched"], ve["it"], ve["samples"], ve["cond_in"])
                if edit:                               # the known slice as first-stage input, the latent keep mask into the chain's state
                    ops.ct_edit_glue(ve["known"], ve["keep"], ve["sched"], ve["it"], int(edit_margin), ve["fs_in"], st["ip_mask"].view(-1, 1))

            def encode():
                encode_head()
                if edit:                               # x0 = scale_factor * posterior mean: the mode, no draw
                    mom = ldm.first_stage_model.encode_moments_cl(CL(ve["fs_in"], 1))
                    st["ip_x0"].copy_(mom.t[..., :Cz] * ldm.scale_factor)

            def decode():
                decode_head()
                if not edit:
                    ops.minmax_normalise_scatter(ve["ds"], ve["sched"], ve["it"], ve["samples"], advance=True, workspace=ve["ws"])
                else:
                    ops.minmax_normalise_keep_scatter(ve["ds"], ve["sched"], ve["it"], ve["known"], ve["keep"], ve["samples"], advance=True,
                                                      workspace=ve["ws"])

            ve["glue"], ve["encode"], ve["decode"] = glue, encode, decode

        return self._engine(self._volume_graphs, key, B, hw, dev, st, finish)

    def _check_edit(self, B: int, depth: int, hw: int, known_ct, keep, edit_margin, q_noise_tapes) -> None:
        """Host-side refusals of the editing loop, by name, before any launch."""
        who = "sample_ct_volumes"
        ldm = self.ldm
        if (known_ct is None) != (keep is None):
            raise ValueError(f"{who}: known_ct= and keep= go together (got only {'known_ct' if keep is None else 'keep'})")
        if known_ct is None:
            if q_noise_tapes is not None or edit_margin != 0:
                raise ValueError(f"{who}: edit_margin / q_noise_tapes edit a known CT: give known_ct= and keep=")
            return
        if hasattr(ldm, "split_input_params"):
            raise NotImplementedError(f"{who}: CT editing with split_input_params (patch-wise evaluation) is not supported")
        if getattr(ldm, "dims", 2) != 2 or getattr(ldm.first_stage_model, "dims", 2) != 2:
            raise NotImplementedError(f"{who}: CT editing is a 2-D slice loop; 3-D latents (dims = 3) are not supported")
        if ldm.model.conditioning_key != "concat":
            raise NotImplementedError(f"{who}: CT editing needs conditioning_key 'concat', got '{ldm.model.conditioning_key}'")
        if type(self.sampler) is not DDIMSampler or any(float(s) != 0.0 for s in self.sampler.ddim_sigmas):
            raise NotImplementedError(f"{who}: CT editing runs the DDIM sampler at eta = 0, got {type(self.sampler).__name__} with "
                                      f"sigmas up to {max(float(s) for s in self.sampler.ddim_sigmas):g}")
        shape = (B, depth, hw, hw)
        if not isinstance(known_ct, torch.Tensor) or tuple(known_ct.shape) != shape or known_ct.dtype != torch.float32:
            raise ValueError(f"{who}: known_ct must be an fp32 {shape} tensor, got {getattr(known_ct, 'dtype', type(known_ct).__name__)} "
                             f"{tuple(getattr(known_ct, 'shape', ()))}")
        if not isinstance(keep, torch.Tensor) or tuple(keep.shape) != shape or keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"{who}: keep must be a bool or uint8 {shape} tensor, got {getattr(keep, 'dtype', type(keep).__name__)} "
                             f"{tuple(getattr(keep, 'shape', ()))}")
        if not isinstance(edit_margin, int) or isinstance(edit_margin, bool) or edit_margin < 0:
            raise ValueError(f"{who}: edit_margin must be an int >= 0, got {edit_margin!r}")
        if hw % self.latent_factor or self.latent_factor * (2 * edit_margin + 1) > hw:
            raise ValueError(f"{who}: edit_margin = {edit_margin}: the window of {self.latent_factor * (2 * edit_margin + 1)} pixels is wider "
                             f"than the {hw} x {hw} slice")
        if q_noise_tapes is not None and len(q_noise_tapes) != B:
            raise ValueError(f"{who}: q_noise_tapes holds {len(q_noise_tapes)} lists, the batch has {B} volumes")
        lo, hi = torch.stack([known_ct.min(), known_ct.max()]).tolist()                # the one host check of the values
        if not (lo >= 0.0 and hi <= 1.0):
            raise ValueError(f"{who}: known_ct holds values {lo:g}..{hi:g} outside [0, 1]")

    @torch.no_grad()
    def sample_ct_volumes(self, labels: torch.Tensor, depth: int, hw: int, seeds: Sequence[int], max_slices: Optional[int] = None,
                          x_T_tapes=None, known_ct: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None, edit_margin: int = 0,
                          q_noise_tapes=None) -> torch.Tensor:
        """labels int32 [B,Dm,Hm,Wm] of B INDEPENDENT volumes -> CT fp32 [B, depth, hw, hw]: volume i is sample_ct(labels[i:i+1], depth,
        hw, seeds[i], max_slices) -- its own slice window, its own min-max normalisation, its own x_T generator -- up to the bf16 rounding
        of batch-size-dependent kernel plans, and bit for bit independent of the other volumes at a fixed B.  The batch is static: a volume
        whose window has ended keeps computing on a discarded row.  One graph replay per slice iteration; the host's share is one x_T
        draw per ACTIVE volume (so every volume's generator stream is its solo one).  `x_T_tapes` (parity runs): per volume, one
        [1, Cz, lat, lat] start latent per generated slice in loop order.  self.stats["wasted_slot_fraction"] reports the discarded work.
        CT editing: known_ct fp32 [B, depth, hw, hw] in [0, 1] (the loop's own output convention) with keep bool / uint8
        of that shape (1 keeps the known voxel, 0 is generated).  Kept voxels come back bit for bit; a slice of the window all of whose
        pixels are kept is not visited (it feeds the next slice as the previous one); a visited slice with kept pixels ("mixed") runs the
        DDIM chain with the sampler's inpainting blend around x0 = scale_factor * mean of the first stage's encoding of the known slice
        (the mode, no draw), the latent keep mask being 1 where every pixel of the cell's window, grown by `edit_margin` cells on each
        side, is kept; the decoded slice is normalised as always and composited per pixel.  A mixed slice draws, after its x_T, one
        [S, 1, Cz, lat, lat] of q-sample noise from the volume's generator (`q_noise_tapes`: per volume, one such tensor per mixed slice in
        loop order); a slice with no kept pixel draws nothing more, so an all-zero keep leaves the volume's stream, and its result, those
        of its un-edited run.  self.stats gains slices_visited / slices_skipped_kept / slices_mixed / unkept_outside_window (un-kept
        pixels on slices outside the window stay 0).  A call without known_ct takes the state, graph and launches it took before."""
        ldm, sampler, S = self.ldm, self.sampler, self.ddim_steps
        dev = labels.device
        B = labels.shape[0]
        if len(seeds) != B or (x_T_tapes is not None and len(x_T_tapes) != B):
            raise ValueError(f"sample_ct_volumes: {B} volumes need {B} seeds (and {B} tapes)")
        self._check_edit(B, depth, hw, known_ct, keep, edit_margin, q_noise_tapes)
        edit = known_ct is not None
        lat, Cz = hw // self.latent_factor, ldm.channels
        if edit:
            known_d = known_ct.to(dev).permute(1, 0, 2, 3).contiguous()               # slice-major, as `samples`
            keep_d = (keep.to(dev) != 0).permute(1, 0, 2, 3).contiguous()
            windows, mixed, counters, start = plan_ct_edit(labels, depth, max_slices, known_d, keep_d, (S, 1, Cz, lat, lat), x_T_tapes,
                                                           q_noise_tapes)
            self.stats.update(counters)
            if not any(windows):                                                       # every slice of every window is kept: no iteration
                self.stats["wasted_slot_fraction"] = 0.0
                return start.permute(1, 0, 2, 3).contiguous()
        else:
            windows = [slice_window(labels[i], depth, max_slices) for i in range(B)]
        sched, wasted = volume_schedule(windows, depth)
        iters = sched.shape[0]
        self.stats["wasted_slot_fraction"] = wasted
        gens = [torch.Generator(device=dev).manual_seed(int(s)) for s in seeds]
        x_tapes, q_tapes = ([None] * B if t is None else t for t in (x_T_tapes, q_noise_tapes))
        st = sampler.prepare_state(B, Cz, (lat, lat), dev, Cz, mask_C=1 if edit else 0)
        ve = self._volume_engine(B, hw, depth, tuple(labels.shape), dev, st, edit_margin=edit_margin if edit else None)
        ve["labels"].copy_(labels)
        if edit:
            ve["known"].copy_(known_d)
            ve["keep"].copy_(keep_d)
            ve["samples"].copy_(start)
            q_used = [0] * B
        else:
            ve["samples"].zero_()
        ve["sched"].zero_()
        ve["sched"][:iters].copy_(sched)                                               # uploaded once per batch
        ve["it"].zero_()
        glue, encode, decode = ve["glue"], ve["encode"], ve["decode"]

        t_last = time.time()
        for it in range(iters):
            if time.time() - t_last > self.progress_every_s:
                _log(f"LDM {'edited ' if edit else ''}slice {it}/{iters} (batch of {B})")
                t_last = time.time()
            x_T = torch.zeros((B, Cz, lat, lat), dtype=torch.float32, device=dev)
            if edit:
                q = torch.zeros((S, B, Cz, lat, lat), dtype=torch.float32, device=dev) # rows of free or inactive volumes stay zero
            for i in range(B):
                if it < len(windows[i]):                                               # the x_T draw of sample_ct, then the q-sample noise
                    x_T[i] = _tape_or_randn(x_tapes[i], it, (1, Cz, lat, lat), gens[i]).reshape(Cz, lat, lat)
                    if edit and mixed[i][it]:
                        q[:, i] = _tape_or_randn(q_tapes[i], q_used[i], (S, 1, Cz, lat, lat), gens[i])[:, 0]
                        q_used[i] += 1
            _load_x_T(st, x_T)
            if edit:
                st["ip_noise"].copy_(q.permute(0, 1, 3, 4, 2).reshape(st["ip_noise"].shape))
            if not (self.use_graph and sampler.chain_graphable(st)):
                glue()
                encode()
                sampler.run_steps(st, None, 0.0, None)
                decode()
            else:
                ops.replay_captured(ve, "graph", lambda: (glue(), encode(), sampler.chain(st), decode()))
        return ve["samples"].clone().permute(1, 0, 2, 3)

    @torch.no_grad()
    def clean_masks(self, labels: torch.Tensor, largest="all", min_size=0, connectivity: int = 6, background: int = 0,
                    fill: Optional[int] = None):
        """postprocess.clean on sampled masks [B, Dm, Hm, Wm] with the CCDM's class count: keep the largest component of the listed
        classes and drop components below min_size voxels.  Returns (cleaned labels, kept uint8 -- shaped as keep= of mask editing --,
        scores before, scores after); the scores also go to self.stats["mask_cleanup"]."""
        from . import postprocess
        out, kept, before, after = postprocess.clean(labels, self.ccdm.diffusion.num_classes, largest=largest, min_size=min_size,
                                                     connectivity=connectivity, background=background, fill=fill)
        self.stats["mask_cleanup"] = dict(before=before, after=after)
        return out, kept, before, after

    @torch.no_grad()
    def run_volumes(self, seeds: Sequence[int], mask_size=(128, 128, 128), depth: int = 256, hw: int = 512,
                    ccdm_init_t: Optional[int] = None, max_slices: Optional[int] = None, clean: Optional[dict] = None):
        """B independent volumes in one batch: volume i is run_volume(N=1, seed=seeds[i]) (seed for the CCDM stage, seed + 1 for the
        LDM stage) up to the bf16 rounding of batch-size-dependent kernel plans.  Returns (labels [B, Dm, Hm, Wm], ct [B, depth, hw, hw]).
        clean: options of clean_masks (a dict; {} = its defaults), applied to the sampled masks before the slice loop, which is then
        conditioned on the cleaned masks, the labels returned.  None (the default): the raw samples, and nothing new is launched."""
        t0 = time.time()
        labels = self.sample_masks(seeds, mask_size, ccdm_init_t)
        if clean is not None:
            from .postprocess import CLEAN_OPTIONS
            unknown = sorted(set(clean) - set(CLEAN_OPTIONS))
            if unknown:
                raise ValueError(f"run_volumes: clean options {unknown} ({', '.join(CLEAN_OPTIONS)})")
            labels = self.clean_masks(labels, **clean)[0]
        torch.cuda.synchronize()
        t1 = time.time()
        ct = self.sample_ct_volumes(labels, depth, hw, [int(s) + 1 for s in seeds], max_slices)
        torch.cuda.synchronize()
        self.stats.update({"ccdm_s": t1 - t0, "ldm_s": time.time() - t1})
        _log(f"{len(seeds)} volumes done: CCDM {t1 - t0:.1f}s, LDM {time.time() - t1:.1f}s, "
             f"wasted slots {self.stats['wasted_slot_fraction']:.3f}")
        return labels, ct

    @torch.no_grad()
    def ct_keep_from_labels(self, old_labels: torch.Tensor, new_labels: torch.Tensor, depth: int, hw: int) -> torch.Tensor:
        """The CT keep volume of an edited mask: uint8 [B, depth, hw, hw], 1 where the stage glue's zoomed, rotated label of new_labels
        equals that of old_labels (both int [B, Dm, Hm, Wm]), i.e. where the slice loop is conditioned as the known CT was."""
        if old_labels.shape != new_labels.shape or old_labels.dim() != 4:
            raise ValueError(f"ct_keep_from_labels: two label volumes [B, Dm, Hm, Wm] of one shape, got {tuple(old_labels.shape)} and "
                             f"{tuple(new_labels.shape)}")
        dev = new_labels.device
        keep = ops.label_keep_volume(old_labels.to(device=dev, dtype=torch.int32).contiguous(), new_labels.to(torch.int32).contiguous(), depth, hw, hw)
        return keep.permute(1, 0, 2, 3).contiguous()

    @torch.no_grad()
    def edit_volumes(self, known_labels: torch.Tensor, known_ct: torch.Tensor, seeds: Sequence[int], label_keep: Optional[torch.Tensor] = None,
                     keep_classes: Optional[Sequence[int]] = None, resample: int = 1, edit_margin: int = 0, ccdm_init_t: Optional[int] = None,
                     max_slices: Optional[int] = None):
        """Edit B known volumes through both stages: known_labels int [B, Dm, Hm, Wm] with exactly one of label_keep (bool / uint8 of that
        shape, 1 keeps the known label) and keep_classes (keep the voxels whose known label is listed); known_ct fp32 [B, depth, hw, hw].
        Stage 1 samples the un-kept labels (sample_masks(known=, keep=, resample=), seed seeds[i]); the CT keep volume is where the new
        labels condition the slice loop as the old ones did (ct_keep_from_labels); stage 2 regenerates the rest of the CT
        (sample_ct_volumes(known_ct=, keep=, edit_margin=), seed seeds[i] + 1).  Returns (labels, ct, ct_keep)."""
        if (label_keep is None) == (keep_classes is None):
            raise ValueError("edit_volumes: give exactly one of label_keep= and keep_classes=")
        if known_labels.dim() != 4 or known_ct.dim() != 4 or known_ct.shape[0] != known_labels.shape[0] or len(seeds) != known_labels.shape[0]:
            raise ValueError(f"edit_volumes: known_labels [B, Dm, Hm, Wm], known_ct [B, depth, hw, hw] and B seeds, got "
                             f"{tuple(known_labels.shape)}, {tuple(known_ct.shape)} and {len(seeds)} seeds")
        dev = self.ccdm.diffusion.betas.device
        depth, hw = int(known_ct.shape[1]), int(known_ct.shape[2])
        known_labels = known_labels.to(device=dev, dtype=torch.int32).contiguous()
        if keep_classes is not None:
            label_keep = torch.isin(known_labels, torch.tensor([int(c) for c in keep_classes], dtype=torch.int32, device=dev))
        t0 = time.time()
        labels = self.sample_masks(seeds, tuple(known_labels.shape[1:]), ccdm_init_t, known=known_labels, keep=label_keep.to(dev), resample=resample)
        ct_keep = self.ct_keep_from_labels(known_labels, labels, depth, hw)
        torch.cuda.synchronize()
        t1 = time.time()
        ct = self.sample_ct_volumes(labels, depth, hw, [int(s) + 1 for s in seeds], max_slices, known_ct=known_ct, keep=ct_keep,
                                    edit_margin=edit_margin)
        torch.cuda.synchronize()
        self.stats.update({"ccdm_s": t1 - t0, "ldm_s": time.time() - t1})
        return labels, ct, ct_keep

    @torch.no_grad()
    def run_volume(self, N: int = 1, mask_size=(128, 128, 128), depth: int = 256, hw: int = 512, seed: int = 1024,
                   ccdm_init_t: Optional[int] = None, max_slices: Optional[int] = None):
        t0 = time.time()
        labels = self.sample_mask(N, mask_size, seed, ccdm_init_t)
        torch.cuda.synchronize()
        t1 = time.time()
        ct = self.sample_ct(labels, depth, hw, seed + 1, max_slices)
        torch.cuda.synchronize()
        self.stats = {"ccdm_s": t1 - t0, "ldm_s": time.time() - t1}
        _log(f"volume done: CCDM {t1 - t0:.1f}s, LDM {time.time() - t1:.1f}s")
        return labels, ct


def main(argv=None) -> None:
    """Sharded full-pipeline entry point (volume_id -> rank = volume_id mod world_size, no collective on the data path)."""
    from . import distributed as ggd
    from .io import write_nifti
    ap = argparse.ArgumentParser(description="GuideGen volumes: CCDM mask -> LDM CT, sharded over the ranks")
    ap.add_argument("--volumes", type=int, required=True, help="number of volumes of the whole job")
    ap.add_argument("--out", default="guidegen_out")
    ap.add_argument("--mask-size", type=int, nargs=3, default=(128, 128, 128))
    ap.add_argument("--depth", type=int, default=256)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--classes", type=int, default=14)
    ap.add_argument("--ccdm-steps", type=int, default=250)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1024)
    ap.add_argument("--max-slices", type=int, default=None, help="DEV ONLY: truncate the slice loop")
    ap.add_argument("--volumes-per-gpu", type=int, default=1, help="independent volumes per batch (groups of a rank's shard)")
    ap.add_argument("--sampler", choices=SAMPLERS, default="ddim", help="latent sampler: DDIM at eta 0, or DPM-Solver++ 2M (about 20 steps)")
    ap.add_argument("--discretize", choices=("uniform", "quad", "logsnr"), default=None,
                    help="step grid (default: uniform for ddim, logsnr for dpmpp_2m; logsnr is the solver's own)")
    args = ap.parse_args(argv)
    if args.volumes_per_gpu < 1:
        ap.error("--volumes-per-gpu must be >= 1")
    try:
        check_sampler_options(args.sampler, args.discretize)
    except ValueError as e:
        ap.error(str(e))
    rank, local, world = ggd.env_rank_world()
    dry = os.environ.get("GG_PIPELINE_DRY") == "1"          # CPU rehearsal of the sharding (tests): no model, no GPU
    os.makedirs(args.out, exist_ok=True)
    mine = ggd.shard(args.volumes, rank, world)
    if dry:
        ggd.init("gloo")
        pipe = None
    else:
        assert torch.cuda.is_available(), "the GuideGen engine needs an MI355X (no CPU fallback)"
        dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
        ggd.init("nccl", dev)
        pipe = GuideGenPipeline(build_ccdm(args.classes, args.ccdm_steps, 1024, dev), build_ldm(1024, dev), ddim_steps=args.ddim_steps,
                                sampler=args.sampler, discretize=args.discretize)
        _log(f"latent sampler {pipe.sampler_name} on the {pipe.discretize} grid: {pipe.steps} steps per slice")
    t0 = time.time()
    B = args.volumes_per_gpu
    if B == 1:
        for vid in mine:
            seed = args.seed + 1000 * vid
            if dry:
                with open(os.path.join(args.out, f"ct_{vid:04d}.txt"), "w") as f:
                    f.write(f"rank {rank} world {world} seed {seed}\n")
                continue
            labels, ct = pipe.run_volume(N=1, mask_size=tuple(args.mask_size), depth=args.depth, hw=args.hw, seed=seed, max_slices=args.max_slices)
            write_nifti(os.path.join(args.out, f"mask_{vid:04d}.nii.gz"), labels[0].to(torch.uint8).cpu().numpy())
            write_nifti(os.path.join(args.out, f"ct_{vid:04d}.nii.gz"), ct[0].float().cpu().numpy())
    else:
        for gi, g0 in enumerate(range(0, len(mine), B)):
            group = mine[g0:g0 + B]
            seeds = [args.seed + 1000 * vid for vid in group]
            if dry:
                for vid, seed in zip(group, seeds):
                    with open(os.path.join(args.out, f"ct_{vid:04d}.txt"), "w") as f:
                        f.write(f"rank {rank} world {world} seed {seed} group {gi} volumes {','.join(str(v) for v in group)}\n")
                continue
            labels, ct = pipe.run_volumes(seeds, mask_size=tuple(args.mask_size), depth=args.depth, hw=args.hw, max_slices=args.max_slices)
            for i, vid in enumerate(group):
                write_nifti(os.path.join(args.out, f"mask_{vid:04d}.nii.gz"), labels[i].to(torch.uint8).cpu().numpy())
                write_nifti(os.path.join(args.out, f"ct_{vid:04d}.nii.gz"), ct[i].float().cpu().numpy())
    print(f"[rank {rank}/{world}] volumes {mine} in {time.time() - t0:.1f}s -> {args.out}", file=sys.stderr)
    ggd.finalize()


if __name__ == "__main__":
    main(sys.argv[1:])

"""DPM-Solver++ (2M) on its log-SNR grid against DDIM on the full-size latent chain, two pipelines on the same models in
one process:

    python tools/bench_dpm_solver.py [--ddim-steps 50] [--dpm-steps 20] [--rounds 7] [--volumes] [--reference-steps 200]

1. `time_slice_stages()` of the two pipelines (N = 1, 512^2 slice, 64x64 latent), alternating for --rounds rounds: the median per-step
   time of each captured chain, and of the whole chain.
2. ODE accuracy on the synthetic weights: from one x_T and one conditioning, the latent of DDIM at --reference-steps against the latents
   of DDIM at --ddim-steps and of the solver at --dpm-steps (max and rms distance relative to the reference latent).  The weights are
   untrained: this says how closely each sampler follows the SAME ODE, nothing about image quality.
3. With --volumes: the wall time of one whole C5 volume (`run_volumes`, B = 1: 128^3 mask, 250 CCDM steps, 256 slices of 512^2) on each
   pipeline, after an untimed warm-up, in voxels/s as bench.py counts them.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from jointimagegeneration_amd.dpm_solver import DPMSolverSampler  # noqa: E402
from jointimagegeneration_amd.ldm import DDIMSampler  # noqa: E402
from jointimagegeneration_amd.pipeline import GuideGenPipeline, build_ccdm, build_ldm  # noqa: E402


def distance(a: torch.Tensor, ref: torch.Tensor) -> dict:
    d = (a - ref).double()
    return {"max_rel": round(float(d.abs().max() / ref.abs().max()), 5),
            "rms_rel": round(float(torch.sqrt((d ** 2).mean()) / torch.sqrt((ref.double() ** 2).mean())), 5)}


def timed_volume(pipe: GuideGenPipeline, seed: int) -> dict:
    size, depth, hw = (128, 128, 128), 256, 512
    pipe.run_volumes([seed], size, depth, hw, ccdm_init_t=10005, max_slices=3)            # warm-up: repacks, captures
    torch.cuda.synchronize()
    t0 = time.time()
    pipe.run_volumes([seed], size, depth, hw)
    torch.cuda.synchronize()
    dt = time.time() - t0
    return {"seconds": round(dt, 2), "voxels_per_s": round((size[0] * size[1] * size[2] + depth * hw * hw) / dt, 1),
            "ccdm_s": round(pipe.stats["ccdm_s"], 2), "ldm_s": round(pipe.stats["ldm_s"], 2)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--dpm-steps", type=int, default=20)
    ap.add_argument("--reference-steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--volumes", action="store_true")
    ap.add_argument("--seed", type=int, default=1024)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dpm_solver needs an MI355X"
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    ccdm = build_ccdm(14, 250, 1024, dev) if args.volumes else None
    ldm = build_ldm(1024, dev)
    pipes = {"ddim": GuideGenPipeline(ccdm, ldm, ddim_steps=args.ddim_steps),
             "dpmpp_2m": GuideGenPipeline(ccdm, ldm, ddim_steps=args.dpm_steps, sampler="dpmpp_2m")}
    res = {"metric": "DPM-Solver++ 2M (logsnr grid) vs DDIM (uniform grid), full-size latent chain, batch 1",
           "config": {"ddim_steps": args.ddim_steps, "dpm_steps_asked": args.dpm_steps, "dpm_steps": pipes["dpmpp_2m"].steps,
                      "weights": "random-init (seed recipe)"}}
    # 1. per-step and per-chain time
    t = {k: [] for k in pipes}
    for r in range(args.rounds + 1):                                  # the first round warms up and captures
        for name in (("ddim", "dpmpp_2m") if r % 2 == 0 else ("dpmpp_2m", "ddim")):
            ms = pipes[name].time_slice_stages(N=1, hw=512)["ddim_step_ms"]
            if r:
                t[name].append(ms)
    for name, pipe in pipes.items():
        step = statistics.median(t[name])
        res[name] = {"steps": pipe.steps, "step_ms_median": round(step, 4), "step_ms_min": round(min(t[name]), 4),
                     "step_ms_max": round(max(t[name]), 4), "chain_ms": round(step * pipe.steps, 2), "fused_head": bool(pipe.sampler.last_step_fused)}
    res["step_ms_difference"] = round(res["dpmpp_2m"]["step_ms_median"] - res["ddim"]["step_ms_median"], 4)
    res["chain_ratio"] = round(res["ddim"]["chain_ms"] / res["dpmpp_2m"]["chain_ms"], 3)
    # 2. ODE accuracy on the synthetic weights
    gen = torch.Generator().manual_seed(args.seed)
    c = torch.randn(1, 4, 64, 64, generator=gen).to(dev)
    x_T = torch.randn(1, 4, 64, 64, generator=gen).to(dev)
    run = lambda s, S: s.sample(S=S, batch_size=1, shape=(4, 64, 64), conditioning=c, verbose=False, x_T=x_T)[0]
    ref = run(DDIMSampler(ldm), args.reference_steps)
    res["ode_accuracy_vs_ddim_%d" % args.reference_steps] = {
        "ddim_%d" % args.ddim_steps: distance(run(DDIMSampler(ldm), args.ddim_steps), ref),
        "ddim_%d" % args.dpm_steps: distance(run(DDIMSampler(ldm), args.dpm_steps), ref),
        "dpmpp_2m_%d" % args.dpm_steps: distance(run(DPMSolverSampler(ldm), args.dpm_steps), ref),
        "dpmpp_1_%d" % args.dpm_steps: distance(run(DPMSolverSampler(ldm, order=1), args.dpm_steps), ref),
        "note": "untrained weights: an indicator of how closely each sampler follows the same ODE, not an image-quality result"}
    # 3. whole volumes
    if args.volumes:
        res["volume"] = {name: timed_volume(pipe, args.seed) for name, pipe in pipes.items()}
        res["volume"]["ratio"] = round(res["volume"]["dpmpp_2m"]["voxels_per_s"] / res["volume"]["ddim"]["voxels_per_s"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

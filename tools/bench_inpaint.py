"""Cost of latent inpainting on the deterministic DDIM chain: full-size latent UNet (LDM_FULL, 64x64 latent of a 512^2 slice, concat
conditioning), 50 DDIM steps, one captured graph per chain, with and without a mask (centre hole, x0 = a sampled latent).

    python tools/bench_inpaint.py [--batch 1 8] [--steps 50] [--rounds 15]

Each configuration is warmed up (eager chain, capture, one replay), then the replays of the two graphs of a batch size ALTERNATE for
--rounds rounds, each replay timed alone with device events.  Reports the median and the min / max per configuration, and the median
of the per-round differences (masked - mask-free) over the number of steps: the cost of one blend launch in the chain.  Prints one JSON
line per batch size.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from jointimagegeneration_amd.ldm import DDIMSampler, LatentDiffusion  # noqa: E402
from jointimagegeneration_amd.synth import randomize_parameters  # noqa: E402

LDM_FULL = dict(dims=2, image_size=512, in_channels=8, out_channels=4, model_channels=160, attention_resolutions=[8, 4, 2],
                num_res_blocks=2, channel_mult=[1, 2, 4, 4, 5], num_head_channels=32)


def replay_ms(graph) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    m = LatentDiffusion(first_stage_config="__is_no_first_stage__", cond_stage_config=dict(target="ldm.modules.encoders.modules.IdentityEncoder"),
                        unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(LDM_FULL)),
                        linear_start=0.0015, linear_end=0.0195, timesteps=1000, image_size=64, channels=4, dims=2, use_ema=False,
                        first_stage_key="image", cond_stage_key="mask", num_timesteps_cond=1).eval()
    randomize_parameters(m.model.diffusion_model, 1024, "ldm.")
    m = m.to(dev)
    for N in args.batch:
        gen = torch.Generator().manual_seed(N)
        c = torch.randn(N, 4, 64, 64, generator=gen).to(dev)
        x_T = torch.randn(N, 4, 64, 64, generator=gen).to(dev)
        s = DDIMSampler(m)
        run = lambda **kw: s.sample(S=args.steps, batch_size=N, shape=(4, 64, 64), conditioning=c, verbose=False, x_T=x_T, dims=2, **kw)[0]
        x0 = run()
        hole = torch.ones(N, 1, 64, 64, device=dev)
        hole[:, :, 16:48, 16:48] = 0.0
        for _ in range(3):
            run()
            run(mask=hole, x0=x0)
        graphs = {}
        for key, st in s._graphs.items():
            graphs["masked" if any(isinstance(e, tuple) and e[0] == "inpaint" for e in key) else "mask_free"] = st["graph"]
        assert set(graphs) == {"masked", "mask_free"} and all(g is not None for g in graphs.values())
        t = {"mask_free": [], "masked": []}
        for r in range(args.rounds):
            order = ("mask_free", "masked") if r % 2 == 0 else ("masked", "mask_free")
            for name in order:
                t[name].append(replay_ms(graphs[name]))
        diff = [b - a for a, b in zip(t["mask_free"], t["masked"])]
        res = {"batch": N, "steps": args.steps, "rounds": args.rounds}
        for name, v in t.items():
            res[name] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
        res["overhead_median_ms"] = round(statistics.median(diff), 3)
        res["overhead_per_step_us"] = round(1000.0 * statistics.median(diff) / args.steps, 2)
        res["overhead_fraction"] = round(statistics.median(diff) / statistics.median(t["mask_free"]), 5)
        print(json.dumps(res), flush=True)
        del s, graphs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

"""Records tests/golden/aeloss.npz and aeloss_surface.json from the REFERENCE's LPIPSWithDiscriminator
(ldm/modules/losses/contperceptual.py) and DiagonalGaussianDistribution, on the CPU.  Only data is written.

    python tests/golden/make_golden_aeloss.py <path to the reference's latentdiffusion directory>

The reference module imports taming, torchvision, requests and tqdm and fetches the LPIPS checkpoint; stubs of our own stand in:
`taming.modules.discriminator.model.weights_init` (a no-op: the weights are seeded below), `taming.modules.util.ActNorm` (never built),
the torchvision stub of make_golden_lpips.py, and `get_ckpt_path` returning the local lin file.  Weights are NOT stored: both sides
rebuild them from the seed recipes of tests/lpips_ref.py (VGG16) and tests/aeloss_ref.py (discriminators), with the per-discriminator
gains written to aeloss_surface.json.  Block outputs are stored as strided samples (the GPU tests compare with the restatement, the CPU
test checks the restatement against these samples); the distance of every fp32 reference value from the fp64 restatement is reduced to
one `tol_<kind>` per kind of value: the largest over all cases.
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import aeloss_ref as A  # noqa: E402
import lpips_ref  # noqa: E402
from make_golden_lpips import stub_modules  # noqa: E402

DISC_START = 5
BASE = dict(disc_start=DISC_START, logvar_init=1.0, kl_weight=1e-6, disc_num_layers=3, disc_in_channels=1, disc_factor=1.0,
            perceptual_weight=1.0, disc_loss="hinge", pixel_loss="l1", gan_feat_weight=0.0)
CASES = [
    dict(name="d2_base", dims=2, step=DISC_START),
    dict(name="d2_before_start", dims=2, step=DISC_START - 1),
    dict(name="d2_vanilla", dims=2, step=DISC_START, disc_loss="vanilla"),
    dict(name="d2_no_lpips", dims=2, step=DISC_START, perceptual_weight=0.0),
    dict(name="d2_layers2_logvar", dims=2, step=DISC_START, disc_num_layers=2, logvar_init=-0.7),
    dict(name="d3_base", dims=3, step=DISC_START),
    dict(name="d3_l2_vanilla", dims=3, step=DISC_START, pixel_loss="l2", disc_loss="vanilla"),
    dict(name="d3_no_lpips_before_start", dims=3, step=DISC_START - 1, perceptual_weight=0.0),
    dict(name="d3_layers2", dims=3, step=DISC_START, disc_num_layers=2),
]
GAINS = (1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0, 24.0)
SAMPLE = 2048                     # values kept per block output


def stub_taming():
    for name in ("taming", "taming.modules", "taming.modules.discriminator", "taming.modules.discriminator.model", "taming.modules.util"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["taming.modules.discriminator.model"].weights_init = lambda m: None
    sys.modules["taming.modules.util"].ActNorm = type("ActNorm", (nn.Module,), {})


def fields(dims):
    """inputs: a smoothed random field in [-1, 1]; reconstructions: inputs plus seeded noise, clamped; moments with both clamp edges."""
    g = torch.Generator().manual_seed(31 + dims)
    shape = (2, 2, 16, 20) if dims == 2 else (2, 1, 4, 16, 20)
    x = torch.rand(shape, generator=g)
    k = torch.ones(1, 1, 3, 5) / 15
    x = torch.nn.functional.conv2d(x.reshape(-1, 1, 16, 20), k, padding=(1, 2)).reshape(shape)
    x = 2 * (x - x.min()) / (x.max() - x.min()) - 1
    y = (x + 0.25 * torch.randn(shape, generator=g)).clamp(-1, 1)
    mom = torch.randn((2, 8) + ((4, 5) if dims == 2 else (1, 4, 5)), generator=g)
    lv = mom[:, 4:].reshape(-1).clone()                  # (a slice of dim 1 does not reshape to a view)
    lv[3], lv[17], lv[40] = -40.0, 25.0, -40.0
    lv[77] = 25.0
    mom[:, 4:] = lv.reshape(mom[:, 4:].shape)
    assert int((mom[:, 4:] < -30).sum()) == 2 and int((mom[:, 4:] > 20).sum()) == 2
    return x.contiguous(), y.contiguous(), mom.contiguous()


def rel(a32, a64):
    a32, a64 = np.asarray(a32, dtype=np.float64), np.asarray(a64, dtype=np.float64)
    return float(np.abs(a32 - a64).max() / max(np.abs(a64).max(), 1e-300))


def spread_ok(l):
    l = l.reshape(-1)
    fr = [float((l < -1).float().mean()), float((l.abs() <= 1).float().mean()), float((l > 1).float().mean())]
    return min(fr) >= 0.05, fr


def main(ref_root):
    stub_modules()
    stub_taming()
    sys.path.insert(0, ref_root)
    lin_path = os.path.join(ref_root, "taming", "modules", "autoencoder", "lpips", "vgg.pth")
    import ldm.modules.losses.lpips as RL
    RL.get_ckpt_path = lambda name, root=None, check=False: lin_path
    import ldm.modules.losses.contperceptual as RC
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution

    vgg_sd = lpips_ref.seeded_vgg_state_dict()
    data = {d: fields(d) for d in (2, 3)}
    out, meta, tol = {}, dict(cases=[], gains={}, surfaces={}, disc_start=DISC_START, base=BASE), {}

    def bump(kind, v):
        tol[kind] = max(tol.get(kind, 0.0), v)

    for d in (2, 3):
        x, y, mom = data[d]
        out[f"x{d}"], out[f"y{d}"], out[f"mom{d}"] = x.numpy(), y.numpy(), mom.numpy()
        # the posterior: kl and a seeded draw
        post = DiagonalGaussianDistribution(mom)
        torch.manual_seed(100 + d)
        z = post.sample()
        torch.manual_seed(100 + d)
        noise = torch.randn(post.mean.shape)
        out[f"noise{d}"], out[f"z{d}"], out[f"kl{d}"] = noise.numpy(), z.numpy(), post.kl().numpy()
        bump("sample", rel(z.numpy(), A.gauss_sample(mom.double(), noise.double()).numpy()))
        bump("kl", rel(post.kl().double().sum().numpy(), A.gauss_kl(mom.double()).sum().numpy()))

    # gains: per discriminator (dims of the loss, which one, layers), the first candidate that spreads the logits of inputs AND reconstructions
    def pick_gain(dims, which, nl):
        x, y, _ = data[dims]
        n = x.shape[0] * x.shape[1]
        xs = [t.reshape((n, 1) + tuple(t.shape[2:])) for t in (x, y)]
        if which == "frame" and dims == 3:
            xs = [t.reshape((-1, 1) + tuple(t.shape[3:])) for t in xs]
        for gain in GAINS:
            sd = A.seeded_disc_state_dict(3 if which == "ct" else 2, 1, nl, dims == 3 or which == "ct", seed_of(dims, which, nl), gain)
            oks = [spread_ok(A.disc_forward(t, sd, nl, dims == 3 or which == "ct")[-1]) for t in xs]
            if all(o[0] for o in oks):
                print(f"gain dims={dims} {which} layers={nl}: {gain}  fractions {oks}")
                return gain
        raise AssertionError(f"no gain spreads the logits of dims={dims} {which} layers={nl}")

    def seed_of(dims, which, nl):
        return 1000 * dims + 100 * (which == "ct") + nl

    lins = None
    results = {}
    for case in CASES:
        cfg = dict(BASE, **{k: v for k, v in case.items() if k not in ("name", "dims", "step")})
        dims, nl, name = case["dims"], cfg["disc_num_layers"], case["name"]
        loss = RC.LPIPSWithDiscriminator(dims=dims, **cfg).eval()
        assert isinstance(loss.frame_discriminator.state_dict(), dict)
        meta["surfaces"][f"dims{dims}_layers{nl}"] = [[k, list(v.shape)] for k, v in loss.state_dict().items()]
        loss.perceptual_loss.net.load_state_dict({f"slice{k}.{i}.{kind}": vgg_sd[f"features.{i}.{kind}"] for k, idxs in
                                                  enumerate(((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28)), 1)
                                                  for i in idxs for kind in ("weight", "bias")})
        lins = [getattr(loss.perceptual_loss, f"lin{k}").model[1].weight.detach().reshape(-1).numpy().copy() for k in range(5)]
        sds = {}
        for which, disc in (("frame", loss.frame_discriminator), ("ct", loss.ct_discriminator)):
            if which == "ct" and dims == 2:
                continue                                                    # built, never called by forward_2d
            gk = f"dims{dims}_{which}_layers{nl}"
            if gk not in meta["gains"]:
                meta["gains"][gk] = pick_gain(dims, which, nl)
            sds[which] = A.seeded_disc_state_dict(3 if which == "ct" else 2, 1, nl, dims == 3 or which == "ct", seed_of(dims, which, nl), meta["gains"][gk])
            disc.load_state_dict(sds[which])
            assert all(isinstance(m, nn.SyncBatchNorm) for m in disc.modules() if "BatchNorm" in type(m).__name__)
        x, y, mom = data[dims]
        post = DiagonalGaussianDistribution(mom)
        with torch.no_grad():
            # last_layer: validation_step hands over the decoder's last weight; under no_grad autograd.grad raises on any tensor, and the
            # reference takes its except branch (d_weight = 0.0)
            last = torch.zeros(1)
            _, r0 = loss(x, y, post, 0, case["step"], last_layer=last, split="val")
            _, r1 = loss(x, y, post, 1, case["step"], last_layer=last, split="val")
            n = x.shape[0] * x.shape[1]
            xf, yf = x.reshape((n, 1) + tuple(x.shape[2:])), y.reshape((n, 1) + tuple(y.shape[2:]))
            fx = xf.reshape((-1, 1) + tuple(xf.shape[3:])) if dims == 3 else xf
            fy = yf.reshape((-1, 1) + tuple(yf.shape[3:])) if dims == 3 else yf
            p32 = loss.perceptual_loss(fx.contiguous(), fy.contiguous()).reshape(-1)
        p64 = A.lpips_images64(fx, fy, lins)
        out[f"p{dims}_ref"], out[f"p{dims}_f64"] = p32.numpy(), p64.numpy()
        d0, d1, parts = A.loss_dicts(dict(cfg, dims=dims), x.double(), y.double(), mom.double(), p64 if cfg["perceptual_weight"] > 0 else None,
                                     sds["frame"], sds.get("ct"), case["step"])
        assert list(r0) == list(d0) and list(r1) == list(d1), (list(r0), list(d0), list(r1), list(d1))
        assert float(r0["val/d_weight"]) == 0.0
        for tag, r, dd in (("0", r0, d0), ("1", r1, d1)):
            out[f"{name}_ref{tag}"] = np.array([float(v) for v in r.values()], dtype=np.float32)
            out[f"{name}_f64_{tag}"] = np.array([float(v) for v in dd.values()], dtype=np.float64)
            for k, v in r.items():
                kind = A.KEY_KIND[k.split("/")[1]]
                want = float(dd[k])
                if kind == "exact":
                    assert float(v) == np.float32(want), (name, k, float(v), want)
                else:
                    bump(kind, abs(float(v) - want) / abs(want) if want else abs(float(v)))
        # block outputs of each discriminator on the reconstructions: strided samples, and the fp32-to-fp64 distance of the full tensors
        with torch.no_grad():
            for which, disc, inp in (("frame", loss.frame_discriminator, fy), ("ct", loss.ct_discriminator, yf)):
                if which not in sds:
                    continue
                key = f"dims{dims}_{which}_layers{nl}"
                if f"{key}_logits" in out:
                    continue
                interm = dims == 3 or which == "ct"
                res = disc(inp.contiguous())
                blocks32 = res[1] if interm else None
                logits32 = res[0] if interm else res
                blocks64 = A.disc_forward(inp.double(), sds[which], nl, interm)
                ok, fr = spread_ok(logits32)
                assert ok, (key, fr)
                out[f"{key}_logits"] = logits32.numpy()
                bump("block", rel(logits32.numpy(), blocks64[-1].numpy()))
                if blocks32 is not None:
                    for i, (b32, b64) in enumerate(zip(blocks32, blocks64)):
                        step = max(1, b32.numel() // SAMPLE)
                        out[f"{key}_block{i}"] = b32.reshape(-1)[::step].numpy()
                        bump("block", rel(b32.numpy(), b64.numpy()))
        meta["cases"].append(dict(name=name, dims=dims, step=case["step"], cfg=cfg, keys0=list(r0), keys1=list(r1)))
        results[name] = (r0, r1)
        print(name, {k: float(v) for k, v in {**r0, **r1}.items()})

    # the conditions the cases must meet
    assert float(results["d2_base"][1]["val/disc_loss"]) != float(results["d2_before_start"][1]["val/disc_loss"]) == 0.0
    assert float(results["d3_base"][1]["val/disc_loss"]) != 0.0 and float(results["d3_no_lpips_before_start"][1]["val/disc_loss"]) == 0.0
    # l1 against l2 with the perceptual term off (fp64 restatement of the 3-D pixel means)
    x, y, _ = data[3]
    l1, l2 = float((x - y).abs().double().mean()), float(((x - y).double() ** 2).mean())
    assert abs(l1 - l2) / max(l1, l2) > 0.05, (l1, l2)
    for k in range(5):
        out[f"lin{k}"] = lins[k]
    for kind, v in tol.items():
        out[f"tol_{kind}"] = np.float64(v)
    print("tolerances", tol)
    np.savez_compressed(os.path.join(HERE, "aeloss.npz"), **out)
    with open(os.path.join(HERE, "aeloss_surface.json"), "w") as f:
        json.dump(meta, f, indent=0)
    sizes = [os.path.getsize(os.path.join(HERE, n)) for n in ("aeloss.npz", "aeloss_surface.json")]
    print("wrote aeloss.npz, aeloss_surface.json:", sizes, "bytes")
    assert sum(sizes) < 300 * 1024


if __name__ == "__main__":
    main(sys.argv[1])

"""Records tests/golden/lpips.npz from the REFERENCE's LPIPS (ldm/modules/losses/lpips.py) and the three-view / segment loop of its
compute_metrics (latentdiffusion/sample_diffusion.py:446-475), on the CPU.  Only data is written.

    python tests/golden/make_golden_lpips.py <path to the reference's latentdiffusion directory>

The reference module imports torchvision, requests and tqdm and fetches its checkpoint; none of that is wanted here, so stubs of our own
stand in: `torchvision.models.vgg16(...).features` builds the standard 13-convolution nn.Sequential, and `get_ckpt_path` returns the
local lpips checkpoint (taming/modules/autoencoder/lpips/vgg.pth, the five linear heads, about 7 KB: stored in the fixture as plain
arrays).  The VGG16 weights (59 MB) are NOT stored: both sides rebuild them from the seed recipe below (restated in tests/lpips_ref.py).
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")
B, D, H, W = 2, 16, 20, 40            # three unequal extents; 16 is the minimum (last tap 1 x 1); 20 -> 10 -> 5 -> 2 -> 1 pools an odd extent


def stub_modules():
    def vgg16(pretrained=False, **_):
        layers, cin = [], 3
        for v in CFG:
            if v == "M":
                layers.append(nn.MaxPool2d(2, 2))
            else:
                layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        m = nn.Module()
        m.features = nn.Sequential(*layers)
        return m
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg16 = vgg16
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
    for name in ("requests", "tqdm"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.tqdm = lambda x=None, **k: x
            sys.modules[name] = m


def seed_vgg(features, seed=1024):
    """Kaiming-normal (fan-out, ReLU) weights, biases normal(0, 0.05), in layer order from torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    with torch.no_grad():
        for i in CONV_IDX:
            nn.init.kaiming_normal_(features[i].weight, mode="fan_out", nonlinearity="relu")
            nn.init.normal_(features[i].bias, 0.0, 0.05)


def volumes():
    """gt: a random field smoothed along H and W; pred: gt plus an anisotropic difference.  Both in [0, 1]."""
    g = torch.Generator().manual_seed(7)
    gt = torch.rand(B, 1, D, H, W, generator=g)
    k = torch.ones(1, 1, 1, 5, 9) / 45
    gt = torch.nn.functional.conv3d(gt, k, padding=(0, 2, 4))
    gt = (gt - gt.min()) / (gt.max() - gt.min())
    # the difference is anisotropic, so that the three views score differently: stripes across D, weaker ones across W, a little white noise
    noise = 0.30 * torch.randn(B, 1, D, 1, 1, generator=g) + 0.12 * torch.randn(B, 1, 1, 1, W, generator=g) + 0.03 * torch.randn(B, 1, D, H, W, generator=g)
    pred = (gt + noise).clamp(0, 1)
    return pred.contiguous(), gt.contiguous()


def main(ref_root):
    stub_modules()
    lin_path = os.path.join(ref_root, "taming", "modules", "autoencoder", "lpips", "vgg.pth")
    # the file itself, not the package: ldm/modules/losses/__init__.py pulls in the discriminator and taming, which LPIPS does not use
    import importlib.util
    spec = importlib.util.spec_from_file_location("reference_lpips", os.path.join(ref_root, "ldm", "modules", "losses", "lpips.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    R.get_ckpt_path = lambda name, root=None, check=False: lin_path
    model = R.LPIPS().eval()
    slices = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
    seed_vgg({i: getattr(getattr(model.net, f"slice{k}"), str(i)) for k, idxs in enumerate(slices, 1) for i in idxs})
    lins = [getattr(model, f"lin{k}").model[1].weight.detach().reshape(-1).numpy().copy() for k in range(5)]

    # the reference's forward with the per-tap terms kept (its own functions, its own order)
    def forward_taps(x, y):
        a, b = model.net(model.scaling_layer(x)), model.net(model.scaling_layer(y))
        res = []
        for kk in range(5):
            d = (R.normalize_tensor(a[kk]) - R.normalize_tensor(b[kk])) ** 2
            res.append(R.spatial_average(getattr(model, f"lin{kk}").model(d), keepdim=True).reshape(-1))
        return torch.stack(res)

    from einops import rearrange
    pred, gt = volumes()
    out = dict(pred=pred.numpy(), gt=gt.numpy(), **{f"lin{k}": w for k, w in enumerate(lins)})
    pats = ("b c d h w -> (b d) c h w", "b c d h w -> (b h) c d w", "b c d h w -> (b w) c d h")
    with torch.no_grad():
        means = []
        for v, pat in enumerate(pats):
            x, y = rearrange(pred, pat), rearrange(gt, pat)
            val = model(x, y).reshape(-1)
            taps = forward_taps(x, y)
            assert torch.allclose(taps.sum(0), val, rtol=1e-5, atol=1e-7)
            out[f"taps_view{v}"], out[f"images_view{v}"] = taps.numpy(), val.numpy()
            means.append(float(val.mean()))
        out["view_means"] = np.array(means, dtype=np.float64)
        print("view means", means)
        lo, mid, hi = sorted(means)
        assert mid / lo > 1.05 and hi / mid > 1.05, "the three view means must differ by more than 5 %"

        def compute(p, g, bps=None):                      # the "lpips" branch of compute_metrics: three view means, averaged, weighted per segment
            b = p.shape[0]
            if bps is None:
                bps = b
            res = 0
            for segment in range(0, b, bps):
                _p, _g = p[segment: segment + bps], g[segment: segment + bps]
                lx = model(rearrange(_p, pats[0]), rearrange(_g, pats[0])).mean()
                ly = model(rearrange(_p, pats[1]), rearrange(_g, pats[1])).mean()
                lz = model(rearrange(_p, pats[2]), rearrange(_g, pats[2])).mean()
                res = res + (lx + ly + lz) / 3 * bps / b
            return float(res)
        out["score"] = np.float64(compute(pred, gt))
        out["score_bps1"] = np.float64(compute(pred, gt, 1))
        out["score_bps3"] = np.float64(compute(pred, gt, 3))       # one short segment of 2 volumes, weighted 3 / 2
        g = torch.Generator().manual_seed(11)
        x4, y4 = torch.rand(2, 3, H, W, generator=g), torch.rand(2, 3, H, W, generator=g)
        out["x4"], out["y4"], out["out4"] = x4.numpy(), y4.numpy(), model(x4, y4).numpy()
    print({k: float(out[k]) for k in ("score", "score_bps1", "score_bps3")}, out["out4"].reshape(-1))
    np.savez_compressed(os.path.join(HERE, "lpips.npz"), **out)
    print("wrote", os.path.join(HERE, "lpips.npz"), os.path.getsize(os.path.join(HERE, "lpips.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])

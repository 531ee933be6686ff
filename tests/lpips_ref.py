"""Plain-torch restatement of the LPIPS the reference computes (ldm/modules/losses/lpips.py in eval mode, and the three-view / segment
loop of latentdiffusion/sample_diffusion.py:446-475), and the seed recipe of the VGG16 weights that tests/golden/lpips.npz was recorded
with.  Test infrastructure: fp32 (or fp64) torch on whatever device the tensors are on."""
import torch
import torch.nn.functional as F

CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)           # torchvision vgg16().features
CONV_OUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
TAP_AFTER = (2, 7, 14, 21, 28)                                         # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 follow these convolutions
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def seeded_vgg_state_dict(seed: int = 1024) -> dict:
    """features.N.weight / .bias: Kaiming-normal (fan-out, ReLU) weights and NON-ZERO biases normal(0, 0.05), drawn in layer order
    (weight, then bias) from torch.manual_seed(seed).  The biases put ReLU cut-offs in play."""
    torch.manual_seed(seed)
    sd, cin = {}, 3
    for i, cout in zip(CONV_IDX, CONV_OUT):
        w = torch.empty(cout, cin, 3, 3)
        torch.nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")
        b = torch.empty(cout)
        torch.nn.init.normal_(b, 0.0, 0.05)
        sd[f"features.{i}.weight"], sd[f"features.{i}.bias"] = w, b
        cin = cout
    return sd


def scaling(x: torch.Tensor) -> torch.Tensor:
    """ScalingLayer for 1- or 3-channel input: a 1-channel image broadcasts to three differently scaled channels."""
    shift = torch.tensor(SHIFT, dtype=torch.float32, device=x.device)[None, :, None, None].to(x.dtype)
    scale = torch.tensor(SCALE, dtype=torch.float32, device=x.device)[None, :, None, None].to(x.dtype)
    return (x - shift) / scale


def vgg_taps(x: torch.Tensor, sd: dict) -> list:
    taps = []
    for i in CONV_IDX:
        if i in (5, 10, 17, 24):
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, sd[f"features.{i}.weight"].to(x), sd[f"features.{i}.bias"].to(x), padding=1))
        if i in TAP_AFTER:
            taps.append(x)
    return taps


def tap_distance(a: torch.Tensor, b: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """a, b [n, C, h, w] (ReLU'd), w [C] -> [n]: mean_hw sum_c w_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2."""
    na = a / (torch.sqrt(torch.sum(a ** 2, 1, keepdim=True)) + 1e-10)
    nb = b / (torch.sqrt(torch.sum(b ** 2, 1, keepdim=True)) + 1e-10)
    return (((na - nb) ** 2) * w.to(a)[None, :, None, None]).sum(1).mean((1, 2))


def lpips_images(x: torch.Tensor, y: torch.Tensor, sd: dict, lins: list):
    """x, y [n, 1 or 3, h, w] -> (per-image LPIPS [n], per-tap terms [5, n])."""
    ta, tb = vgg_taps(scaling(x), sd), vgg_taps(scaling(y), sd)
    taps = torch.stack([tap_distance(a, b, w) for a, b, w in zip(ta, tb, lins)])
    val = taps[0].clone()
    for k in range(1, 5):
        val = val + taps[k]
    return val, taps


def views(v: torch.Tensor) -> list:
    """[b, 1, D, H, W] -> the three stacks "(b d) 1 h w", "(b h) 1 d w", "(b w) 1 d h"."""
    b, c, D, H, W = v.shape
    return [v.permute(0, 2, 1, 3, 4).reshape(b * D, c, H, W), v.permute(0, 3, 1, 2, 4).reshape(b * H, c, D, W),
            v.permute(0, 4, 1, 2, 3).reshape(b * W, c, D, H)]


def lpips_3view(pred: torch.Tensor, gt: torch.Tensor, sd: dict, lins: list, batch_per_segment=None) -> float:
    b = pred.shape[0]
    bps = b if batch_per_segment is None else batch_per_segment
    res = 0.0
    for s in range(0, b, bps):
        means = [float(lpips_images(x, y, sd, lins)[0].mean()) for x, y in zip(views(pred[s:s + bps]), views(gt[s:s + bps]))]
        res = res + (means[0] + means[1] + means[2]) / 3 * bps / b
    return res

"""Three-view LPIPS of generated CT volumes, on the device: `compute_metrics(pred, gt, ["lpips"])` of
latentdiffusion/sample_diffusion.py:436-475 with the LPIPS of ldm/modules/losses/lpips.py in eval mode.

    python -m jointimagegeneration_amd.lpips --pred DIR --gt DIR --vgg PATH --lin PATH

The 13 VGG16 convolutions are `ops.conv` calls (channels-last 3x3 MFMA kernels, or the fp32 kernels inside `ops.fp32_validation()`);
`gg_volume_views_cl` cuts a volume into the scaled three-channel images of one axis view, `gg_relu_cl` is the ReLU after the 8
convolutions no tap follows, `gg_lpips_tap` reads each tap tensor once for ReLU, distance and 2x2 max-pool (csrc/gg_lpips.hip).

The reference's behaviour is kept, quirks included: a 1-channel slice broadcasts to three DIFFERENTLY scaled channels (ScalingLayer);
inputs are used as given ([0, 1] from the slice loop, never rescaled to [-1, 1]); a 5-D input is scored as the mean of the three axis
views' means; with batch_per_segment a short last segment still weighs batch_per_segment / b.  FVD is refused: it needs an I3D network
and a `scripts.fvd` the reference does not ship.  Weights are never fetched: LPIPS.load reads two local files.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from .io import load_checkpoint, read_nifti

CHNS = (64, 128, 256, 512, 512)
# torchvision's vgg16().features indices of the convolutions of each slice; a 2x2 max-pool stands in front of slices 2..5, a ReLU
# behind every convolution, the tap behind the last ReLU of a slice (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3)
VGG_SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
MIN_EXTENT = 16                      # four floor-halvings must leave a pixel: below, the reference's fourth max-pool raises
CHUNK_BYTES = 512 << 20              # bound on the 64-channel full-resolution activation of one chunk (pred and gt images together)


def vgg_conv_shapes() -> Dict[str, Tuple[int, ...]]:
    """`net.sliceK.N.weight` / `.bias` -> shape, for the 13 convolutions."""
    out, cin = {}, 3
    for k, (idxs, cout) in enumerate(zip(VGG_SLICES, CHNS), 1):
        for i in idxs:
            out[f"net.slice{k}.{i}.weight"] = (cout, cin, 3, 3)
            out[f"net.slice{k}.{i}.bias"] = (cout,)
            cin = cout
    return out


def map_vgg_state_dict(sd: Dict[str, torch.Tensor], what: str = "VGG16 state dict") -> Dict[str, torch.Tensor]:
    """A VGG16 feature state dict under torchvision's names (`features.N.*`, or bare `N.*`) or the reference's (`net.sliceK.N.*`,
    or `sliceK.N.*`) -> the `net.sliceK.N.*` names.  A missing key or a wrong shape raises, naming it."""
    out = {}
    for name, shape in vgg_conv_shapes().items():
        _, sl, idx, kind = name.split(".")
        for cand in (name, f"{sl}.{idx}.{kind}", f"features.{idx}.{kind}", f"{idx}.{kind}"):
            if cand in sd:
                t = sd[cand]
                if tuple(t.shape) != shape:
                    raise ValueError(f"{what}: {cand} has shape {tuple(t.shape)}, expected {shape}")
                out[name] = t
                break
        else:
            raise KeyError(f"{what}: no {name} (nor features.{idx}.{kind})")
    return out


def map_lin_state_dict(sd: Dict[str, torch.Tensor], what: str = "lpips checkpoint") -> Dict[str, torch.Tensor]:
    out = {}
    for k, c in enumerate(CHNS):
        name = f"lin{k}.model.1.weight"
        if name not in sd:
            raise KeyError(f"{what}: no {name}")
        if tuple(sd[name].shape) != (1, c, 1, 1):
            raise ValueError(f"{what}: {name} has shape {tuple(sd[name].shape)}, expected {(1, c, 1, 1)}")
        out[name] = sd[name]
    return out


class _Conv(nn.Module):
    """Parameter holder of one 3x3 convolution (the arithmetic is ops.conv)."""

    def __init__(self, cin: int, cout: int, k: int = 3, bias: bool = True):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, cin, k, k), requires_grad=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.tensor([.458, .448, .450])[None, :, None, None])
        self.shift_p = nn.Parameter(torch.tensor([-.1])[None, :, None, None], requires_grad=False)
        self.scale_p = nn.Parameter(torch.tensor([.45])[None, :, None, None], requires_grad=False)


class LPIPS(nn.Module):
    """state_dict names and shapes of the reference's LPIPS: net.slice1.0.weight ... net.slice5.28.bias, lin0.model.1.weight ...
    lin4.model.1.weight, scaling_layer.shift / scale / shift_p / scale_p."""

    def __init__(self):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.net = nn.Module()
        cin = 3
        for k, (idxs, cout) in enumerate(zip(VGG_SLICES, CHNS), 1):
            sl = nn.Module()
            for i in idxs:
                sl.add_module(str(i), _Conv(cin, cout))
                cin = cout
            self.net.add_module(f"slice{k}", sl)
        for k, c in enumerate(CHNS):
            lin = nn.Module()
            lin.model = nn.Module()
            lin.model.add_module("1", _Conv(c, 1, k=1, bias=False))
            self.add_module(f"lin{k}", lin)
        self.chunk_images: Optional[int] = None      # tests: force the number of images per chunk (None: the CHUNK_BYTES rule)
        self._packs = {}

    @classmethod
    def load(cls, vgg_path: str, lin_path: str) -> "LPIPS":
        """vgg_path: a VGG16 feature state dict (torchvision's `features.N.*` names or `net.sliceK.N.*`); lin_path: an lpips checkpoint
        with `linK.model.1.weight`.  Local files only; everything is checked before the device is touched."""
        for p in (vgg_path, lin_path):
            if not p or not os.path.isfile(p):
                raise FileNotFoundError(f"LPIPS.load: {p!r} is not a file (weights are never fetched: give local paths)")
        sd = dict(map_vgg_state_dict(load_checkpoint(vgg_path), vgg_path))
        sd.update(map_lin_state_dict(load_checkpoint(lin_path), lin_path))
        m = cls()
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.startswith("scaling_layer.") for k in missing), (missing, unexpected)
        return m.eval()

    # ------------------------------------------------------------------------------------------- device side
    def _convs(self) -> List[List[_Conv]]:
        return [[getattr(getattr(self.net, f"slice{k}"), str(i)) for i in idxs] for k, idxs in enumerate(VGG_SLICES, 1)]

    def _pack_key(self):
        """The precision mode, the weights' token and the identity of the scaling layer's shift / scale: those two are buffers, which
        `ops.weights_token` does not count, and the pack holds copies of them."""
        sc = self.scaling_layer
        return (ops.FP32, ops.weights_token(self)) + tuple((b.data_ptr(), b._version) for b in (sc.shift, sc.scale))

    def _packed(self):
        """Per precision mode: ([[(packed weight, padded bias, cout)]], [lin weights fp32 [C]], shift[3], scale[3]); rebuilt when the
        weights or the scaling buffers change."""
        key = self._pack_key()
        hit = self._packs.get(ops.FP32)
        if hit is None or hit[0] != key:
            convs = [[(ops.pack_conv_weight(c.weight, ops.pad32(c.weight.shape[1])), ops.pad_bias(c.bias, c.weight.shape[0], c.weight.device),
                       int(c.weight.shape[0])) for c in sl] for sl in self._convs()]
            lins = [getattr(self, f"lin{k}").model.get_submodule("1").weight.detach().float().reshape(-1).contiguous() for k in range(5)]
            sc = self.scaling_layer
            hit = (key, (convs, lins, sc.shift.detach().float().reshape(-1).contiguous(), sc.scale.detach().float().reshape(-1).contiguous()))
            self._packs[ops.FP32] = hit
        return hit[1]

    def prepare(self) -> "LPIPS":
        """Pack the weights for the current precision mode now (otherwise the first call does it).  The packs are the only device memory
        the module keeps between calls."""
        self._packed()
        return self

    def chunk_size(self, hh: int, ww: int) -> int:
        """Images of EACH input per chunk: the 64-channel activation at full resolution of the chunk's 2 m images stays within
        CHUNK_BYTES (it is the largest tensor of the network; two of them and the 32-channel input are alive at once)."""
        if self.chunk_images is not None:
            return max(1, int(self.chunk_images))
        return max(1, CHUNK_BYTES // (2 * hh * ww * 64 * (4 if ops.FP32 else 2)))

    @torch.no_grad()
    def score_view(self, pred: torch.Tensor, gt: torch.Tensor, view: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """pred, gt: contiguous fp32 [B, D, H, W] on the device; view as in ops.volume_views_cl.  Returns (per-image LPIPS fp32 [n],
        per-tap per-image terms fp32 [5, n]) for the n images of the view."""
        B, D, H, W = (int(v) for v in pred.shape)
        n, hh, ww = ((B * D, H, W), (B * H, D, W), (B * W, D, H), (B, H, W))[view]
        convs, lins, shift, scale = self._packed()
        dev = pred.device
        total = torch.empty(n, dtype=torch.float32, device=dev)
        taps = torch.empty((5, n), dtype=torch.float32, device=dev)
        dt = torch.float32 if ops.FP32 else torch.bfloat16
        step = self.chunk_size(hh, ww)
        for n0 in range(0, n, step):
            n1 = min(n, n0 + step)
            m = n1 - n0
            x = torch.empty((2 * m, 1, hh, ww, 32), dtype=dt, device=dev)         # pred's images, then gt's: one batch per convolution
            ops.volume_views_cl(pred, view, n0, n1, shift, scale, x[:m])
            ops.volume_views_cl(gt, view, n0, n1, shift, scale, x[m:])
            h = ops.CL(x, 3)
            for k, sl in enumerate(convs):
                for j, (pw, pb, cout) in enumerate(sl):
                    h = ops.conv(h, pw, pb, cout, k=(1, 3, 3), stride=1, pad=1)
                    if j + 1 < len(sl):
                        ops.relu_cl(h)
                _, pooled = ops.lpips_tap(h.t[:m], h.t[m:], lins[k], pool=k < 4, tap_out=taps[k, n0:n1], total=total[n0:n1], accumulate=k > 0)
                if k < 4:
                    h = ops.CL(pooled, cout)
        return total, taps

    def _check_pair(self, a: torch.Tensor, b: torch.Tensor, what: str) -> None:
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"{what}: pred.shape != gt.shape ({tuple(a.shape)} and {tuple(b.shape)})")
        ops.require_gpu(a, what)
        ops.require_gpu(b, what)
        if next(self.parameters()).device != a.device:
            raise RuntimeError(f"{what}: the LPIPS weights are on {next(self.parameters()).device}, the input on {a.device}")

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """4-D NCHW tensors on the device -> per-image [n, 1, 1, 1], unreduced, as the reference returns it."""
        if input.dim() != 4:
            raise ValueError(f"LPIPS.forward: 4-D NCHW input, got {tuple(input.shape)}")
        self._check_pair(input, target, "LPIPS.forward")
        n, c, h, w = (int(v) for v in input.shape)
        if min(h, w) < MIN_EXTENT:
            raise ValueError(f"LPIPS.forward: image extent {h} x {w} below {MIN_EXTENT}: the fourth max-pool would produce nothing (the reference raises too)")
        if c not in (1, 3):
            # ScalingLayer takes the shift_p / scale_p branch for such input and hands c channels to a 3-channel convolution
            raise ValueError(f"LPIPS.forward: {c}-channel input: ScalingLayer would scale it with shift_p / scale_p and VGG16's first convolution "
                             "takes 3 channels (the reference raises there); give 1- or 3-channel images")
        a, b = input.detach().float().contiguous(), target.detach().float().contiguous()
        if c == 1:
            total, _ = self.score_view(a.reshape(1, n, h, w), b.reshape(1, n, h, w), 0)
        else:
            total, _ = self.score_view(a, b, 3)
        return total.reshape(n, 1, 1, 1)

    @torch.no_grad()
    def view_means(self, pred: torch.Tensor, gt: torch.Tensor) -> List[float]:
        """[b, 1, D, H, W] -> the means of the per-image scores of the three axis views (fp64 mean of the fp32 per-image values, in
        image order)."""
        p, g = pred.detach().float().contiguous()[:, 0], gt.detach().float().contiguous()[:, 0]
        return [float(self.score_view(p.contiguous(), g.contiguous(), v)[0].double().cpu().mean()) for v in range(3)]


def check_metrics(metrics) -> None:
    for m in metrics:
        if m == "fvd":
            raise NotImplementedError("metric 'fvd' is not supported: it needs an I3D network and a scripts.fvd module that the reference does not ship")
        if m != "lpips":
            raise ValueError(f"unknown metric {m!r} (supported: 'lpips')")


def lpips_3view(pred: torch.Tensor, gt: torch.Tensor, batch_per_segment: Optional[int] = None, model: Optional[LPIPS] = None) -> float:
    """The `_compute` / segment loop of compute_metrics (sample_diffusion.py:446-475) for "lpips": pred, gt [b, c, D, H, W] on the device; c != 1 is flattened to (b c) 1 ... first; each segment adds value * batch_per_segment / b."""
    if model is None:
        raise ValueError("lpips_3view: give model=LPIPS.load(vgg_path, lin_path) (weights are never fetched)")
    if pred.dim() != 5:
        raise ValueError(f"lpips_3view: [b, c, D, H, W] volumes, got {tuple(pred.shape)} (4-D images: call the LPIPS module, which returns the "
                         "per-image tensor as the reference does)")
    model._check_pair(pred, gt, "lpips_3view")
    if min(pred.shape[2:]) < MIN_EXTENT:
        raise ValueError(f"lpips_3view: extent {tuple(pred.shape[2:])} below {MIN_EXTENT}: the fourth max-pool would produce nothing (the reference raises too)")
    b, c = int(pred.shape[0]), int(pred.shape[1])
    if batch_per_segment is None:
        batch_per_segment = b
    if batch_per_segment < 1:
        raise ValueError(f"lpips_3view: batch_per_segment={batch_per_segment}")
    if c != 1:
        pred = pred.reshape((b * c, 1) + tuple(pred.shape[2:]))
        gt = gt.reshape((b * c, 1) + tuple(gt.shape[2:]))
    result = 0.0
    for seg in range(0, b, batch_per_segment):
        vx, vy, vz = model.view_means(pred[seg:seg + batch_per_segment], gt[seg:seg + batch_per_segment])
        result = result + (vx + vy + vz) / 3 * batch_per_segment / b
    return float(result)


def compute_metrics(pred, gt, metrics=("lpips",), batch_per_segment=None, model: Optional[LPIPS] = None) -> dict:
    """compute_metrics of the reference for the metrics this engine has ("lpips"); "fvd" is refused by name."""
    check_metrics(metrics)
    if not len(metrics):
        return {}
    return {"lpips": lpips_3view(pred, gt, batch_per_segment, model)}


def load_volume(path: str) -> torch.Tensor:
    """A NIfTI volume [D, H, W] as a host fp32 tensor [1, 1, D, H, W]."""
    return torch.from_numpy(read_nifti(path).astype("float32"))[None, None]


def score_directory(model: LPIPS, pred_files: List[str], gt_dir: str, device) -> dict:
    """Each volume against the same-named volume of gt_dir -> the metrics.json document.  Every pair is checked before the first launch."""
    pairs = []
    for p in pred_files:
        g = os.path.join(gt_dir, os.path.basename(p))
        if not os.path.isfile(g):
            raise FileNotFoundError(f"no ground truth {g} for {p}")
        pairs.append((p, g))
    vols = []
    for p, g in pairs:
        a, b = load_volume(p), load_volume(g)
        if a.shape != b.shape:
            raise ValueError(f"{p}: prediction {tuple(a.shape[2:])} and ground truth {tuple(b.shape[2:])} differ in shape")
        vols.append(dict(name=os.path.basename(p), shape=list(a.shape[2:]), lpips=lpips_3view(a.to(device), b.to(device), model=model)))
    return dict(metric="lpips (mean of three axis views)", mean_lpips=sum(v["lpips"] for v in vols) / len(vols), volumes=vols)


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description="three-view LPIPS of the volumes of --pred against the same-named volumes of --gt")
    ap.add_argument("--pred", required=True, help="directory of *.nii.gz / *.nii volumes")
    ap.add_argument("--gt", required=True, help="directory holding a volume of the same name for each")
    ap.add_argument("--vgg", required=True, help="VGG16 feature state dict (torchvision's names or net.sliceK.N.*)")
    ap.add_argument("--lin", required=True, help="lpips checkpoint with linK.model.1.weight")
    ap.add_argument("--out", default=None, help="metrics.json path (default: PRED/metrics.json)")
    args = ap.parse_args(argv)
    files = sorted(f for f in glob.glob(os.path.join(args.pred, "*.nii*")) if f.endswith((".nii", ".nii.gz")))
    if not files:
        raise FileNotFoundError(f"{args.pred}: no *.nii / *.nii.gz volumes")
    model = LPIPS.load(args.vgg, args.lin)
    assert torch.cuda.is_available(), "the GuideGen engine needs an MI355X (no CPU fallback)"
    dev = torch.device("cuda", 0)
    doc = score_directory(model.to(dev), files, args.gt, dev)
    out = args.out or os.path.join(args.pred, "metrics.json")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(f"mean LPIPS {doc['mean_lpips']:.5f} over {len(doc['volumes'])} volume(s) -> {out}", file=sys.stderr)
    return doc


if __name__ == "__main__":
    main(sys.argv[1:])

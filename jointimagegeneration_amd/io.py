"""Minimal volume / checkpoint IO for the entry points (SimpleITK/nibabel are not dependencies).

write_nifti / read_nifti: single-file NIfTI-1 (.nii / .nii.gz), enough for the label and CT volumes the reference writes with
SimpleITK (ccdm/ddpm/evaluator.py:147-148, latentdiffusion/sample_diffusion.py:248-250) and reads back with nibabel when the
stage-1 masks are handed to the CT generator (README.md:21; recipe latentdiffusion/sample_diffusion.py:199-200).
write_png: the 8-bit RGB PNG of a rendered slice grid (render.py), on zlib + struct (PIL is not a dependency).
Checkpoints are read with torch.load(weights_only=True) only.
"""
from __future__ import annotations

import gzip
import json
import os
import struct
import zlib

import numpy as np
import torch

_NIFTI_DTYPES = {np.dtype("uint8"): (2, 8), np.dtype("int16"): (4, 16), np.dtype("int32"): (8, 32), np.dtype("float32"): (16, 32)}


def write_nifti(path: str, arr: np.ndarray, spacing=(1.0, 1.0, 1.0)) -> None:
    """arr is [D, H, W] (SimpleITK GetImageFromArray convention: stored as x=W fastest)."""
    arr = np.ascontiguousarray(arr)
    if arr.dtype not in _NIFTI_DTYPES:
        arr = arr.astype(np.float32)
    code, bits = _NIFTI_DTYPES[arr.dtype]
    D, H, W = arr.shape
    hdr = bytearray(348)
    struct.pack_into("<i", hdr, 0, 348)
    struct.pack_into("<8h", hdr, 40, 3, W, H, D, 1, 1, 1, 1)
    struct.pack_into("<h", hdr, 70, code)
    struct.pack_into("<h", hdr, 72, bits)
    struct.pack_into("<8f", hdr, 76, 1.0, spacing[0], spacing[1], spacing[2], 1.0, 1.0, 1.0, 1.0)
    struct.pack_into("<f", hdr, 108, 352.0)                 # vox_offset
    struct.pack_into("<f", hdr, 112, 1.0)                   # scl_slope
    struct.pack_into("<h", hdr, 254, 1)                     # sform_code
    struct.pack_into("<4f", hdr, 280, spacing[0], 0, 0, 0)
    struct.pack_into("<4f", hdr, 296, 0, spacing[1], 0, 0)
    struct.pack_into("<4f", hdr, 312, 0, 0, spacing[2], 0)
    hdr[344:348] = b"n+1\0"
    payload = bytes(hdr) + b"\0\0\0\0" + arr.tobytes()
    if path.endswith(".gz"):
        with gzip.open(path, "wb", compresslevel=1) as f:
            f.write(payload)
    else:
        with open(path, "wb") as f:
            f.write(payload)


_NIFTI_CODES = {2: np.uint8, 4: np.int16, 8: np.int32, 16: np.float32, 64: np.float64, 256: np.int8, 512: np.uint16, 768: np.uint32}


def read_nifti(path: str) -> np.ndarray:
    """Inverse of write_nifti: a single-file NIfTI-1 volume (.nii / .nii.gz, little endian) as an array [D, H, W] -- what
    `nibabel.load(path).dataobj[:].transpose(2, 1, 0)` gives (latentdiffusion/sample_diffusion.py:199).  scl_slope / scl_inter are
    applied when they are set to something other than identity (then the result is float32)."""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        raw = f.read()
    if len(raw) < 352 or struct.unpack_from("<i", raw, 0)[0] != 348:
        raise ValueError(f"{path}: not a little-endian single-file NIfTI-1 volume (sizeof_hdr != 348)")
    if raw[344:348] not in (b"n+1\0", b"ni1\0"):
        raise ValueError(f"{path}: NIfTI-1 magic missing")
    dims = struct.unpack_from("<8h", raw, 40)
    if dims[0] < 3 or any(d != 1 for d in dims[4:1 + dims[0]]):
        raise ValueError(f"{path}: expected a 3-D volume, header dim = {dims}")
    code = struct.unpack_from("<h", raw, 70)[0]
    if code not in _NIFTI_CODES:
        raise ValueError(f"{path}: unsupported NIfTI datatype code {code}")
    W, H, D = dims[1], dims[2], dims[3]
    off = int(struct.unpack_from("<f", raw, 108)[0]) or 352
    dt = np.dtype(_NIFTI_CODES[code]).newbyteorder("<")
    n = D * H * W
    if len(raw) < off + n * dt.itemsize:
        raise ValueError(f"{path}: truncated voxel data ({len(raw) - off} bytes for {n} voxels of {dt})")
    arr = np.frombuffer(raw, dtype=dt, count=n, offset=off).reshape(D, H, W)
    slope, inter = struct.unpack_from("<2f", raw, 112)
    if slope not in (0.0, 1.0) or inter != 0.0:
        arr = arr.astype(np.float32) * np.float32(slope) + np.float32(inter)
    return np.ascontiguousarray(arr)


def write_png(path: str, img: np.ndarray) -> None:
    """An 8-bit RGB PNG of a uint8 [H, W, 3] array (what `PIL.Image.fromarray(grid).save(path)` stores, latentdiffusion/
    sample_diffusion.py:252-261): signature, IHDR, one IDAT of the zlib-compressed scanlines (filter type 0 on every row), IEND."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"write_png: a uint8 [H, W, 3] array, got {img.dtype} {img.shape}")
    H, W = img.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)          # a filter byte (0: none) in front of every scanline
    rows[:, 1:] = img.reshape(H, 3 * W)

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)))      # 8 bits, colour type 2 (RGB), no interlace
        f.write(chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        f.write(chunk(b"IEND", b""))


def load_checkpoint(path: str) -> dict:
    """Safe loader only (executes nothing from the file)."""
    return torch.load(path, map_location="cpu", weights_only=True)


# ----------------------------------------------------------------------------------------------- local Hugging Face model directory
# What FrozenBERTEmbedder needs of a directory saved by transformers' save_pretrained (config.json, vocab.txt, tokenizer_config.json and
# model.safetensors or pytorch_model.bin), read without transformers, tokenizers or safetensors.
_SAFETENSORS_DTYPES = {"F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16}
_SAFETENSORS_HEADER_MAX = 100 * 1024 * 1024


def read_safetensors(path: str) -> dict:
    """{name: tensor} of a .safetensors file: 8-byte little-endian header length, a JSON header {name: {dtype, shape, data_offsets}}
    (plus "__metadata__"), then the tensors' raw little-endian bytes.  F32 / F16 / BF16 only; every offset is checked against the file."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 8:
        raise ValueError(f"{path}: too short for a safetensors header")
    (n,) = struct.unpack("<Q", raw[:8])
    if n > _SAFETENSORS_HEADER_MAX or 8 + n > len(raw):
        raise ValueError(f"{path}: safetensors header length {n} does not fit the file ({len(raw)} bytes)")
    header = json.loads(raw[8:8 + n].decode("utf-8"))
    data = memoryview(raw)[8 + n:]
    out = {}
    for name, e in header.items():
        if name == "__metadata__":
            continue
        if e["dtype"] not in _SAFETENSORS_DTYPES:
            raise NotImplementedError(f"{path}: tensor {name!r} has dtype {e['dtype']} (F32, F16 and BF16 are supported)")
        dt = _SAFETENSORS_DTYPES[e["dtype"]]
        shape = [int(v) for v in e["shape"]]
        b0, b1 = (int(v) for v in e["data_offsets"])
        numel = int(np.prod(shape, dtype=np.int64)) if shape else 1
        if not (0 <= b0 <= b1 <= len(data)) or b1 - b0 != numel * dt.itemsize:
            raise ValueError(f"{path}: tensor {name!r} {shape} {e['dtype']} does not match its byte range [{b0}, {b1}) of {len(data)}")
        # little-endian host assumed, as everywhere in this package (NIfTI writer above)
        out[name] = torch.frombuffer(bytearray(data[b0:b1]), dtype=dt).reshape(shape) if numel else torch.zeros(shape, dtype=dt)
    return out


def load_hf_dir(path: str):
    """(config dict, state_dict, vocab list, tokenizer config dict) of a local Hugging Face model directory.  Weights come from
    model.safetensors if present, else from pytorch_model.bin through the safe loader; nothing outside `path` is touched."""
    if not os.path.isdir(path):
        raise FileNotFoundError(f"{path}: not a directory (a local Hugging Face model directory is expected; nothing is downloaded)")

    def need(name):
        p = os.path.join(path, name)
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p}: missing from the model directory")
        return p

    with open(need("config.json"), "r", encoding="utf-8") as f:
        config = json.load(f)
    with open(need("vocab.txt"), "r", encoding="utf-8") as f:
        vocab = [line.rstrip("\n") for line in f]
    while vocab and vocab[-1] == "":
        vocab.pop()
    tok_cfg = {}
    p = os.path.join(path, "tokenizer_config.json")
    if os.path.exists(p):
        with open(p, "r", encoding="utf-8") as f:
            tok_cfg = json.load(f)
    st = os.path.join(path, "model.safetensors")
    sd = read_safetensors(st) if os.path.exists(st) else load_checkpoint(need("pytorch_model.bin"))
    return config, sd, vocab, tok_cfg

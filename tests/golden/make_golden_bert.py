"""Generates tests/golden/bert.npz and tests/golden/bert_surface.json from the REFERENCE FrozenBERTEmbedder, both copies
(ccdm/ddpm/models/encoder.py:21-100 and latentdiffusion/ldm/modules/encoders/modules.py:205-284), on CPU, from the synthetic model
directory tests/golden/bert_tiny (config.json, vocab.txt, tokenizer_config.json: our own files) plus seed-recipe weights written into a
temporary copy of it; and one 3-step eta = 0 DDIM chain of the reference LatentDiffusion with that cond stage (crossattn, the small
SpatialTransformer UNet, context_dim 64).

Run only in the build container (needs the reference tree and transformers, like make_golden.py):
    python tests/golden/make_golden_bert.py [OUT_DIR]
The fixture holds the state_dict surface, the tokenizer's ids and masks for STRINGS, last_hidden_state for x = bert_encode_batch = 1
(a batch of 3) and x = 2 (use_text_split), and the chain.  Weights are regenerated from the seed recipe by the tests (prefixes
"bert_tiny." and "ldm_bert.").  The LDM copy never imports `reduce` (modules.py:266): its text splitting raises NameError, which is
asserted here; its x = 2 output is recorded with functools.reduce supplied to that module.
"""
from __future__ import annotations

import contextlib
import functools
import io
import json
import os
import shutil
import sys
import tempfile
import unittest.mock as mock

import numpy as np
import torch
from transformers import BertConfig, BertModel  # noqa: F401  (before the stub torchvision of make_golden.import_ldm)
from transformers import AutoModel, AutoTokenizer  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import bert_ref  # noqa: E402

from jointimagegeneration_amd.synth import randomize_parameters  # noqa: E402
from jointimagegeneration_amd.tokenizer import BertWordPieceTokenizer  # noqa: E402

torch.set_grad_enabled(False)
TINY_DIR = os.path.join(HERE, "bert_tiny")
N_TOK = 16                                  # bert_max_length as the tests set it
STRINGS = [
    "",
    "CT: Liver TUMOR 3cm，左肾 résumé (Café)! unseen",                         # CJK + Latin, accents, upper case, punctuation
    "x" * 101 + " liver",                                                                 # a word of more than 100 characters: [UNK]
    "the liver tumor in the left lobe of the right kidney with no lesion 肝脏肿瘤左右肾",     # more than 14 tokens: truncated
    "seg\u200bmentation [SEP] [MASK] unknownword 25mm\tno\x07 lesions.",          # specials, ## pieces, digits, control characters: 15 tokens
]
BATCH3 = (1, 0, 3)
SPLIT = (1, 2)
CHAIN = (1, 3)
CHAIN_T = 999
UNET = dict(MG.LDM_SMALL, in_channels=4, use_spatial_transformer=True, transformer_depth=1, context_dim=64)


def surface(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def main(out_dir):
    import importlib
    MG.import_ldm()
    di = importlib.import_module("ldm.models.diffusion.ddim")
    dm = importlib.import_module("ldm.models.diffusion.ddpm")
    ut = importlib.import_module("ldm.modules.diffusionmodules.util")
    enc_ldm = importlib.import_module("ldm.modules.encoders.modules")
    MG.import_ccdm()
    enc_ccdm = importlib.import_module("ddpm.models.encoder")
    quiet = contextlib.redirect_stdout(io.StringIO())
    out, surf = {}, {}

    with open(os.path.join(TINY_DIR, "config.json")) as f:
        cfg = json.load(f)
    tmp = tempfile.mkdtemp(prefix="bert_tiny_")
    try:
        hf = BertModel(BertConfig(**cfg)).eval()
        randomize_parameters(hf, MG.SEED, "bert_tiny.")
        hf.save_pretrained(tmp)
        for name in ("vocab.txt", "tokenizer_config.json"):
            shutil.copy(os.path.join(TINY_DIR, name), tmp)
        sd = MG.sd_of(hf)
        assert [[k, list(v.shape)] for k, v in sd.items()] == bert_ref.surface(cfg)
        mine = bert_ref.seeded_state_dict(cfg, "bert_tiny.")
        assert all(torch.equal(mine[k], sd[k]) for k in sd)

        # ---- the tokenizer call of forward(), per string
        with open(os.path.join(TINY_DIR, "vocab.txt"), encoding="utf-8") as f:
            vocab = [line.rstrip("\n") for line in f]
        ours = BertWordPieceTokenizer(vocab, do_lower_case=True)
        for name, enc in (("ccdm", enc_ccdm), ("ldm", enc_ldm)):
            m = enc.FrozenBERTEmbedder(ckpt_path=tmp, device="cpu").eval()
            assert (m.bert_max_length, m.bert_encode_batch, m.use_text_split) == (512, 1, False)
            m.bert_max_length = N_TOK
            surf[name] = surface(m)
            be = m.tokenizer(STRINGS, truncation=True, max_length=N_TOK, return_length=True, return_overflowing_tokens=False,
                             padding="max_length", return_tensors="pt")
            ids, mask = be["input_ids"], be["attention_mask"]
            if name == "ccdm":
                out["ids"], out["mask"] = ids.numpy().astype(np.int32), mask.numpy().astype(np.int32)
                oi, om = ours.encode(STRINGS, N_TOK)
                for s, a, b in zip(STRINGS, oi, ids.tolist()):
                    assert a == b, f"the product tokenizer differs on {s!r}:\n {a}\n {b}"
                assert om == mask.tolist()
            else:
                assert np.array_equal(out["ids"], ids.numpy()) and np.array_equal(out["mask"], mask.numpy())
            lengths = mask.sum(1)

            # x = 1, a batch of 3
            z = m([STRINGS[i] for i in BATCH3])
            assert tuple(z.shape) == (3, N_TOK, cfg["hidden_size"])
            sel = torch.tensor(BATCH3)
            ref = bert_ref.forward(sd, ids[sel].long(), lengths[sel], cfg)
            e32 = MG.close(ref, z, 2e-5, f"{name} x=1")
            sd64 = {k: v.double() for k, v in sd.items()}
            e64 = float((bert_ref.forward(sd64, ids[sel].long(), lengths[sel], cfg) - z.double()).abs().max())
            print(f"{name}: bert_ref vs reference, x = 1: fp32 {e32:.3e}, fp64 {e64:.3e} (max |ref| {float(z.abs().max()):.3f})")
            out[f"{name}_x1"] = z.numpy()

            # x = 2 with use_text_split: every text becomes [text, ""]
            m.bert_encode_batch, m.use_text_split = 2, True
            texts = [STRINGS[i] for i in SPLIT]
            if name == "ldm":
                try:
                    m(texts)
                    raise AssertionError("the LDM copy's text splitting ran: the NameError deviation no longer holds")
                except NameError as e:
                    assert "reduce" in str(e)
                enc.reduce = functools.reduce
            merged = m._merge_text_list(*texts)
            assert merged == [texts[0], "", texts[1], ""]
            z2 = m(texts)
            assert tuple(z2.shape) == (2, 2 * N_TOK, cfg["hidden_size"])
            i2, m2 = ours.encode(merged, N_TOK)
            ref2 = bert_ref.interleave(bert_ref.forward(sd, torch.tensor(i2), torch.tensor(m2).sum(1), cfg), 2)
            MG.close(ref2, z2, 2e-5, f"{name} x=2")
            out[f"{name}_x2"] = z2.numpy()
            if name == "ccdm":
                surf["merged_x2"] = merged
                for bad_x, texts_bad in ((3, texts), (2, ["y" * 512])):                  # what the reference cannot run (refused by the product)
                    m.bert_encode_batch = bad_x
                    try:
                        m(texts_bad)
                        ran = True
                    except Exception as e:                                                # einops / list + tuple
                        ran = False
                        print(f"ccdm: use_text_split x = {bad_x}, {len(texts_bad[0])} characters: {type(e).__name__}")
                    assert not ran, f"the reference ran use_text_split with x = {bad_x}, {len(texts_bad[0])} characters"
        assert np.array_equal(out["ccdm_x1"], out["ldm_x1"]) and np.array_equal(out["ccdm_x2"], out["ldm_x2"])

        # ---- chain: reference LatentDiffusion, FrozenBERTEmbedder cond stage (crossattn), small SpatialTransformer UNet, 3 DDIM steps
        cfg_unet = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(UNET))
        cfg_ae = dict(target="ldm.models.autoencoder.AutoencoderKL",
                      params=dict(embed_dim=4, dims=2, ddconfig=dict(MG.AE_SMALL), lossconfig=dict(target="torch.nn.Identity")))
        cfg_cond = dict(target="ldm.modules.encoders.modules.FrozenBERTEmbedder", params=dict(ckpt_path=tmp, device="cpu"))
        with quiet:
            ld = dm.LatentDiffusion(first_stage_config=cfg_ae, cond_stage_config=cfg_cond, unet_config=cfg_unet, conditioning_key="crossattn",
                                    linear_start=0.0015, linear_end=0.0195, timesteps=CHAIN_T, image_size=8, channels=4, dims=2,
                                    first_stage_key="image", cond_stage_key="caption", num_timesteps_cond=1).eval()
        ld.cond_stage_model.bert_max_length = N_TOK
        randomize_parameters(ld, MG.SEED, "ldm_bert.")
        gen = MG.g(778)
        x_T = torch.randn(2, 4, 8, 8, generator=gen)
        c = ld.get_learned_conditioning([STRINGS[i] for i in CHAIN])
        assert tuple(c.shape) == (2, N_TOK, 64)
        sampler = di.DDIMSampler(ld)
        with mock.patch.object(ut.torch, "randn", lambda *a, **k: torch.zeros(2, 4, 8, 8)), quiet:
            z, _ = sampler.sample(S=3, batch_size=2, shape=(4, 8, 8), conditioning=c, verbose=False, x_T=x_T, dims=2, eta=0.0)
            z_other, _ = sampler.sample(S=3, batch_size=2, shape=(4, 8, 8), conditioning=c.flip(0).contiguous(), verbose=False, x_T=x_T, dims=2, eta=0.0)
        rms = float(torch.sqrt(((z - z_other) ** 2).mean()) / torch.sqrt((z ** 2).mean()))
        print(f"chain: the samples' contexts swapped moves z by rms {rms:.3e} of its own")
        assert rms > 5 * 1.5e-2                                                        # the context matters: 5 x the GPU suite's rms bound
        out.update(chain_x_T=x_T.numpy(), chain_c=c.numpy(), chain_z=z.numpy(), chain_timesteps=np.array(CHAIN_T),
                   chain_ddim_timesteps=np.asarray(sampler.ddim_timesteps))
        surf["chain_cond_stage"] = [e for e in surface(ld) if e[0].startswith("cond_stage_model.")]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    surf["strings"] = STRINGS
    surf["batch3"], surf["split"], surf["chain"], surf["n_tok"] = list(BATCH3), list(SPLIT), list(CHAIN), N_TOK
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "bert.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(out_dir, "bert_surface.json"), "w") as f:
        json.dump(surf, f, indent=1, ensure_ascii=True)
        f.write("\n")
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB) and bert_surface.json")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else MG.OUT)
